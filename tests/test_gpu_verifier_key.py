"""GPU checks of the verifier key that is loaded from its bytes: SpartanSNARK.vk_to_bytes, hip.Shape.from_wire (the device decode of kernels_wire_decode.hpp
and the host decode beside it) and host.SpartanVerifier. Nothing expected comes from the code under test: key bytes and digests are the CPU oracle's
(OracleSpartan.vk_bytes / export_keys), products are orc_shape_multiply_vec or Python integers, verdicts are OracleSpartan.verify_words, and the crafted
streams are written by the small bincode writer below (model: tests/pywire.py)."""
import ctypes
import re
import struct

import numpy as np
import pytest

import oracle_lib as ol
from spartan2_amd import frontend, hip, host
from spartan2_amd.host import pad_shape

pytestmark = pytest.mark.gpu
P = ol.MODULI[0]
RINV = pow(ol.R, -1, P)
FORMS = [True, False]  # device decode, host decode
FORM_IDS = ["device", "host"]
# the decode kernels' block and scan-tile sizes, named here and pinned to the library's by tests/test_verifier_key_cpu.py
WIRE_BLOCK = 256
WIRE_SCAN_TILE = 1024
ROW_COUNTS = [1, WIRE_BLOCK - 1, WIRE_BLOCK, WIRE_BLOCK + 1, WIRE_SCAN_TILE - 1, WIRE_SCAN_TILE, WIRE_SCAN_TILE + 1, 2 * WIRE_SCAN_TILE + 1]
SPMV_LONG_ROW = 24  # k_spmv3 walks rows longer than this with the whole wave (capi_sparse.hip)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _circuit(which):
    return {"cubic": frontend.cubic_circuit, "synthetic_segments": lambda: frontend.synthetic_circuit(60, 9, num_public=3, shared_permille=200, precommitted_permille=500),
            "sha256_1block": lambda: frontend.sha256_circuit(b"abc"), "sha256_64B": lambda: frontend.sha256_circuit(bytes(range(64)))}[which]()


CIRCUITS = ["cubic", "synthetic_segments", "sha256_1block"]
_oracles = {}


def oracle(which):
    """the oracle's key of a circuit, made once: (instance, OracleSpartan, key bytes, digest bytes)"""
    if which not in _oracles:
        inst = _circuit(which)
        osp = ol.OracleSpartan(inst)
        _oracles[which] = (inst, osp, osp.vk_bytes(), osp.export_keys()[4].tobytes())
    return _oracles[which]


# ---- a bincode reader / writer of the key, in Python -------------------------------------------------------------------------------------------------------
DIM_ORDER = ("num_cons", "num_cons_unpadded", "num_shared_unpadded", "num_precommitted_unpadded", "num_rest_unpadded", "num_shared", "num_precommitted", "num_rest",
             "num_public", "num_challenges")  # field order of SplitR1CSShape (src/r1cs/mod.rs:743-755)


def u64(v):
    return struct.pack("<Q", int(v))


def split_key(vk):
    """the structural boundaries of a key's bytes: -> (offset of ck_s, offset of S, [every boundary inside S])"""
    o = 0
    offs = []
    for _ in range(2):
        n = struct.unpack_from("<Q", vk, o + 8)[0]
        o += 16 + 64 * n + 96
        offs.append(o)
    marks = [o + 80]
    q = o + 80
    for _ in range(3):
        for width in (32, 8, 8):
            n = struct.unpack_from("<Q", vk, q)[0]
            q += 8
            marks.append(q)
            q += width * n
            marks.append(q)
        q += 8
        marks.append(q)
    assert q == len(vk)
    return offs[0], offs[1], marks


def matrix_bytes(data, idx, ptr, cols, len_data=None, len_idx=None, len_ptr=None):
    """SparseMatrix { data, indices, indptr, cols } (src/r1cs/sparse.rs:383-394); the len_* override a Vec's length prefix"""
    out = [u64(len(data) if len_data is None else len_data)] + [int(v).to_bytes(32, "little") for v in data]
    out += [u64(len(idx) if len_idx is None else len_idx)] + [u64(v) for v in idx]
    out += [u64(len(ptr) if len_ptr is None else len_ptr)] + [u64(v) for v in ptr]
    return b"".join(out) + u64(cols)


def shape_bytes(dims, mats, cols=None):
    """dims: dict over DIM_ORDER; mats: 3 x (coefficients as canonical integers, column indices, indptr)"""
    if cols is None:
        cols = dims["num_shared"] + dims["num_precommitted"] + dims["num_rest"] + 1 + dims["num_public"] + dims["num_challenges"]
    return b"".join(u64(dims[k]) for k in DIM_ORDER) + b"".join(matrix_bytes(d, i, p_, cols) for d, i, p_ in mats)


def plain_dims(rows, cols):
    d = dict.fromkeys(DIM_ORDER, 0)
    d.update(num_cons=rows, num_cons_unpadded=rows, num_rest=cols - 1, num_rest_unpadded=cols - 1)
    return d


def raw_ints(limbs):
    b = np.ascontiguousarray(limbs, dtype="<u8").tobytes()
    return [int.from_bytes(b[32 * i: 32 * i + 32], "little") for i in range(len(b) // 32)]


def raw_limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def random_residues(rng, n):
    raw = rng.bytes(32 * n)
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") % P for i in range(n)]


def products(shape, ctx, zlimbs, rows):
    outs = [hip.Table.zeros(ctx, rows) for _ in range(3)]
    z = hip.Table.from_host(ctx, zlimbs)
    shape.multiply_vec(z, *outs)
    got = [o.read() for o in outs]
    for t in outs + [z]:
        t.free()
    return got


# ---- 1. writing --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CIRCUITS + ["sha256_64B"])
def test_vk_to_bytes_equals_the_oracle(ctx, which):
    inst, osp, vk, dig = oracle(which)
    sn = host.SpartanSNARK(ctx, inst)
    got = sn.vk_to_bytes()
    assert len(got) == len(vk) and got == vk
    assert sn.vk_digest.tobytes() == dig
    if which == "cubic":  # the circuit is handed over again: another one than the key's is refused
        sn.inst = _circuit("synthetic_segments")
        with pytest.raises(hip.SpartanHipError, match="not the one this key was set up from"):
            sn.vk_to_bytes()
    sn.close()


# ---- 2. the decode against the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("which", CIRCUITS)
def test_decoded_shape_equals_the_oracle(ctx, which, device):
    inst, osp, vk, _ = oracle(which)
    _, off_S, _ = split_key(vk)
    oshape = osp.shape
    N, ncols = oshape.num_cons, oshape.num_vars + oshape.num_extra
    rng = np.random.default_rng(20261020 + len(which))
    z = ol.random_field_array(rng, ncols)
    want = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
    assert ol.lib().orc_shape_multiply_vec(oshape.h, ol.p64(z), *(ol.p64(w) for w in want)) == 0
    x, y = random_residues(rng, N), random_residues(rng, ncols)
    ylimbs = raw_limbs(y)
    prods = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
    assert ol.lib().orc_shape_multiply_vec(oshape.h, ol.p64(ylimbs), *(ol.p64(w) for w in prods)) == 0
    want_evals = [sum(xi * ai for xi, ai in zip(x, raw_ints(w))) % P * RINV % P for w in prods]  # (see tests/test_gpu_verify_batch.py kernel_case)
    mats, dims = pad_shape(inst)
    full = hip.Shape(ctx, mats, dims)
    tx, ty = hip.Table.from_host(ctx, raw_limbs(x)), hip.Table.from_host(ctx, ylimbs)
    results = []
    for _ in range(2):
        shape = hip.Shape.from_wire(ctx, vk[off_S:], device_decode=device)
        assert shape.stages["device"] == (1.0 if device else 0.0)
        assert shape.dims == dims
        info = shape.info()
        assert info["nnz"] == full.info()["nnz"]
        assert info["nnz_filtered"] == [0, 0, 0] and info["long_columns"] == 0 and info["short_columns"] == 0  # a row-only shape
        got = products(shape, ctx, z, N)
        for g, w in zip(got, want):
            assert (g == w).all()
        ev = shape.matrix_evals_batched([tx], [ty])
        assert raw_ints(ev[0]) == want_evals
        results.append((got, ev))
    assert all((a == b).all() for a, b in zip(results[0][0], results[1][0])) and (results[0][1] == results[1][1]).all()
    # what a row-only shape does not hold is refused by name, not dereferenced
    rx, out = hip.Table.zeros(ctx, N), hip.Table.zeros(ctx, ncols)
    tabs = [hip.Table.zeros(ctx, N) for _ in range(8)]
    zt = hip.Table.from_host(ctx, z)
    with pytest.raises(hip.SpartanHipError, match="row-only shape"):
        shape.poly_abc(rx, raw_limbs([3])[0], ncols, out)
    with pytest.raises(hip.SpartanHipError, match="row-only shape"):
        shape.poly_abc_batch(raw_limbs([0] * (N.bit_length() - 1)), raw_limbs([3]), ncols, [out])
    with pytest.raises(hip.SpartanHipError, match="row-only shape"):
        shape.multiply_vec_incremental(zt, *tabs[:6])
    with pytest.raises(hip.SpartanHipError, match="row-only shape"):
        shape.multiply_vec_incremental_round0(zt, *tabs)
    shape.is_sat(zt)  # ... and is_sat serves it
    for t in [tx, ty, rx, out, zt] + tabs:
        t.free()


def test_full_shape_from_wire(ctx):
    """full=True: the shape of hip.Shape(ctx, *pad_shape(inst)) through the host decode"""
    inst, osp, vk, _ = oracle("synthetic_segments")
    _, off_S, _ = split_key(vk)
    mats, dims = pad_shape(inst)
    ref, shape = hip.Shape(ctx, mats, dims), hip.Shape.from_wire(ctx, vk[off_S:], full=True)
    assert shape.info() == ref.info() and shape.info()["short_columns"] > 0
    with pytest.raises(hip.SpartanHipError, match="exclude each other"):
        hip.Shape.from_wire(ctx, vk[off_S:], device_decode=True, full=True)


# ---- 3. hand-written matrices ------------------------------------------------------------------------------------------------------------------------------
SMALL = [k for k in range(1, 8)] + [P - k for k in range(1, 8)]  # the fourteen coded values: +-1 .. +-7
GENERAL = [8, P - 8, 0, 1 << 64]


def _coeffs(rng, n, kind):
    if kind == "small":
        return [SMALL[int(i)] for i in rng.integers(0, len(SMALL), n)]
    if kind == "general":
        return [(GENERAL + random_residues(rng, 4))[int(i)] for i in rng.integers(0, len(GENERAL) + 4, n)]
    pool = SMALL + GENERAL + random_residues(rng, 6)
    return [pool[int(i)] for i in rng.integers(0, len(pool), n)]


def build_matrix(rng, rows, cols, lengths, kinds):
    data, idx, ptr = [], [], [0]
    for r in range(rows):
        n = lengths[r]
        data += _coeffs(rng, n, kinds[r])
        idx += [int(c) for c in rng.integers(0, cols, n)]
        ptr.append(len(data))
    return data, idx, ptr


def hand_written(rows, long_rows, seed):
    """A: one row each of 1, 63, 64, 65 and 300 entries among short ones (long_rows; otherwise every row stays at or below SPMV_LONG_ROW), each coded value
    and each general one at least once; B: a row of small codes only, a row of general coefficients only, alternating; C: empty rows at the start, in the
    middle and at the end."""
    rng = np.random.default_rng(seed)
    cols = 37
    la = [int(v) for v in rng.integers(0, 4, rows)]
    if long_rows:
        specials = [1, 63, 64, 65, 300]
        for k, n in enumerate(specials if rows >= 5 else specials[3:4]):
            la[(k * rows) // 5] = n
    assert len(SMALL) + len(GENERAL) <= SPMV_LONG_ROW
    la[rows - 1] = max(la[rows - 1], len(SMALL) + len(GENERAL))  # every class value once, in the last row
    A = build_matrix(rng, rows, cols, la, ["mixed"] * rows)
    lo = A[2][rows - 1]
    A[0][lo: lo + len(SMALL) + len(GENERAL)] = SMALL + GENERAL
    B = build_matrix(rng, rows, cols, [int(v) for v in rng.integers(1, 4, rows)], ["small" if r % 2 == 0 else "general" for r in range(rows)])
    lc = [int(v) for v in rng.integers(1, 4, rows)]
    for r in {0, 1, rows // 2 - 1, rows // 2, rows - 2, rows - 1}:
        if 0 <= r < rows:
            lc[r] = 0
    C = build_matrix(rng, rows, cols, lc, ["mixed"] * rows)
    return cols, [A, B, C]


def expected_products(mats, rows, z):
    """Python integers. With z~ the limbs of the table as they are, a coefficient c (held as c R, or as the code of a small one) contributes c z~[col]."""
    out = []
    for data, idx, ptr in mats:
        out.append([sum(data[k] * z[idx[k]] for k in range(ptr[r], ptr[r + 1])) % P for r in range(rows)])
    return out


def check_hand_written(ctx, rows, cols, mats, device, seed):
    z = random_residues(np.random.default_rng(seed), cols)
    want = expected_products(mats, rows, z)
    blob = shape_bytes(plain_dims(rows, cols), mats)
    shape = hip.Shape.from_wire(ctx, blob, device_decode=device)
    assert shape.info()["nnz"] == [len(m[0]) for m in mats]
    got = products(shape, ctx, raw_limbs(z), rows)
    for m in range(3):
        g = raw_ints(got[m])
        bad = [r for r in range(rows) if g[r] != want[m][r]]
        assert not bad, f"matrix {'ABC'[m]}: rows {bad[:8]} differ (of {len(bad)})"
    return got


@pytest.mark.parametrize("device", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("long_rows", [True, False], ids=["long_rows", "short_rows"])
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_hand_written_matrices(ctx, rows, long_rows, device):
    cols, mats = hand_written(rows, long_rows, 1000 + rows)
    longest = max(p_[r + 1] - p_[r] for _, _, p_ in mats for r in range(rows))
    assert (longest > SPMV_LONG_ROW) == long_rows  # both forms of k_spmv3 are reached through max_len
    first = check_hand_written(ctx, rows, cols, mats, device, 7 + rows)
    again = check_hand_written(ctx, rows, cols, mats, device, 7 + rows)
    assert all((a == b).all() for a, b in zip(first, again))


@pytest.mark.parametrize("device", FORMS, ids=FORM_IDS)
def test_hand_written_empty_matrices(ctx, device):
    rows, cols = 5, 9
    mats = [([], [], [0] * (rows + 1))] * 3
    got = check_hand_written(ctx, rows, cols, mats, device, 3)
    assert not any(g.any() for g in got)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def tiny():
    rows, cols = 6, 9
    rng = np.random.default_rng(99)
    mats = [build_matrix(rng, rows, cols, [2, 0, 3, 1, 0, 2], ["mixed"] * rows) for _ in range(3)]
    return rows, cols, mats


def still_usable(ctx):
    rows, cols, mats = tiny()
    check_hand_written(ctx, rows, cols, mats, True, 5)


def refused(ctx, blob, device, match):
    with pytest.raises(hip.SpartanHipError, match=match) as e:
        hip.Shape.from_wire(ctx, blob, device_decode=device)
    assert re.search(match, hip.lib().sp_last_error().decode())  # the reason is in sp_last_error
    still_usable(ctx)
    return str(e.value)


@pytest.mark.parametrize("device", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("value", [P, (1 << 256) - 1], ids=["q", "2^256-1"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_refuses_a_non_canonical_coefficient(ctx, where, value, device):
    rows, cols, mats = tiny()
    for m in range(3):
        bad = [(list(d), i, p_) for d, i, p_ in mats]
        n = len(bad[m][0])
        at = {"first": 0, "middle": n // 2, "last": n - 1}[where]
        bad[m][0][at] = value
        msg = refused(ctx, shape_bytes(plain_dims(rows, cols), bad), device, "non-canonical field element")
        if device:  # the device decode names the first offender
            assert f"entry {at} of matrix {'ABC'[m]}" in msg


@pytest.mark.parametrize("device", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("value", ["cols", 1 << 32, (1 << 32) + 3, (1 << 64) - 1])
def test_refuses_a_column_index_out_of_range(ctx, value, device):
    rows, cols, mats = tiny()
    bad = [(d, list(i), p_) for d, i, p_ in mats]
    bad[1][1][-1] = cols if value == "cols" else value  # (2^32 + 3 would pass a check made after narrowing: 3 < cols)
    refused(ctx, shape_bytes(plain_dims(rows, cols), bad), device, "column index out of range")


@pytest.mark.parametrize("device", FORMS, ids=FORM_IDS)
def test_refuses_a_bad_structure_before_any_launch(ctx, device):
    rows, cols, mats = tiny()
    dims = plain_dims(rows, cols)
    d, i, p_ = mats[2]

    def with_C(data=d, idx=i, ptr=p_, c=cols, **lens):
        return b"".join(u64(dims[k]) for k in DIM_ORDER) + matrix_bytes(*mats[0], cols) + matrix_bytes(*mats[1], cols) + matrix_bytes(data, idx, ptr, c, **lens)

    dec = list(p_)
    dec[3] = dec[2] - 1
    refused(ctx, with_C(ptr=dec), device, "indptr decreases")
    refused(ctx, with_C(ptr=[1] + list(p_[1:])), device, "indptr does not start at 0")
    refused(ctx, with_C(ptr=list(p_[:-1]) + [p_[-1] - 1]), device, "indptr does not end at the entry count")
    refused(ctx, with_C(ptr=list(p_[:-1]) + [p_[-1] + 1]), device, "indptr does not end at the entry count")
    refused(ctx, with_C(ptr=list(p_) + [p_[-1]]), device, "num_cons \\+ 1 offsets")
    refused(ctx, with_C(ptr=list(p_[:-1])), device, "num_cons \\+ 1 offsets")
    refused(ctx, with_C(idx=list(i) + [0]), device, "data and indices differ in length")
    refused(ctx, with_C(c=cols + 1), device, "cols is not")
    refused(ctx, with_C(len_data=1 << 62), device, "length prefix exceeds the input")
    refused(ctx, with_C(len_idx=1 << 62), device, "length prefix exceeds the input")
    refused(ctx, with_C(len_ptr=1 << 62), device, "length prefix exceeds the input")
    over = dict(dims, num_cons_unpadded=rows + 1)
    refused(ctx, shape_bytes(over, mats, cols=cols), device, "num_cons_unpadded exceeds num_cons")
    refused(ctx, shape_bytes(dict(dims, num_rest_unpadded=cols), mats, cols=cols), device, "unpadded variable count exceeds")
    refused(ctx, shape_bytes(dict(dims, num_public=1 << 32), mats, cols=cols), device, "2\\^32 or more")
    good = shape_bytes(dims, mats)
    refused(ctx, good + b"\0", device, "trailing bytes")
    refused(ctx, good[:-1], device, "unexpected end of input|length prefix exceeds the input")
    for cut in (0, 8, 79, 80, 87, 88):
        refused(ctx, good[:cut], device, "unexpected end of input|length prefix exceeds the input")


def key_refused(ctx, blob, device, match):
    with pytest.raises(hip.SpartanHipError, match=match):
        host.SpartanVerifier.from_bytes(ctx, blob, device_decode=device)
    assert re.search(match, host.lib().ss_last_error().decode())


@pytest.mark.parametrize("device", FORMS, ids=FORM_IDS)
def test_refuses_bytes_that_are_not_a_key(ctx, device):
    inst, osp, vk, dig = oracle("cubic")
    off_s, off_S, marks = split_key(vk)
    # an off-curve generator (the lowest bit of a y coordinate), in each key
    for at in (16 + 32, 16 + 64 * 1000 + 32, off_s + 16 + 32):
        bad = bytearray(vk)
        bad[at] ^= 1
        key_refused(ctx, bytes(bad), device, "not on the curve")
    bad = bytearray(vk)
    bad[16 + 64 * 2048 + 64] ^= 3  # h of vk_ee: z = 1 -> 2 leaves the curve as well
    key_refused(ctx, bytes(bad), device, "not on the curve")
    # a generator count other than num_cols, either way round
    key_refused(ctx, u64(2047) + vk[8:], device, "generators for num_cols")
    key_refused(ctx, vk[:8] + u64(2047) + vk[16:], device, "generators for num_cols|not on the curve|non-canonical")
    key_refused(ctx, u64(2047) + u64(2047) + vk[16:16 + 64 * 2047] + vk[16 + 64 * 2048:], device, "this build's is 2048")
    # the ten dimensions: an unpadded count above its padded one, and a set that SplitR1CSShape::new does not produce
    dims = list(struct.unpack_from("<10Q", vk, off_S))
    over = list(dims)
    over[1] = dims[0] + 1
    key_refused(ctx, vk[:off_S] + struct.pack("<10Q", *over) + vk[off_S + 80:], device, "num_cons_unpadded exceeds num_cons")
    odd = list(dims)
    assert dims[0] >= 2
    odd[1] = dims[0] // 2  # an unpadded count that SplitR1CSShape::new pads to half as many rows
    key_refused(ctx, vk[:off_S] + struct.pack("<10Q", *odd) + vk[off_S + 80:], device, "ten dimensions")
    # cut at every structural boundary, one byte short, one byte long
    for cut in sorted(set([0, 8, 16, off_s - 96, off_s, off_s + 8, off_S, off_S + 8] + marks[:-1] + [len(vk) - 1])):
        key_refused(ctx, vk[:cut], device, "unexpected end of input|length prefix exceeds the input|no bytes")
    key_refused(ctx, vk + b"\0", device, "trailing bytes")
    # a coefficient equal to the modulus reaches the verifier's loader as the shape's refusal
    bad = bytearray(vk)
    bad[marks[1]: marks[1] + 32] = P.to_bytes(32, "little")
    key_refused(ctx, bytes(bad), device, "non-canonical field element")
    v = host.SpartanVerifier.from_bytes(ctx, vk, device_decode=device)  # the context still serves a good key
    assert v.vk_digest.tobytes() == dig
    v.close()


# ---- 5. the verifier -------------------------------------------------------------------------------------------------------------------------------------
_proofs = {}


def proofs_of(ctx, which):
    """one good proof of the product's prover and one tampered proof per failed-check code, with the oracle's verdicts: made once per circuit"""
    if which in _proofs:
        return _proofs[which]
    inst, osp, vk, dig = oracle(which)
    sn = host.SpartanSNARK(ctx, inst)
    tape = ol.make_tape(4321, 4096)
    sn.prep_prove(tape)
    words, _, _ = sn.prove(ol.make_tape(4322, 4096))
    d = sn.dims
    rows = (((d["num_shared"] + 2047) // 2048) if d["num_shared_unpadded"] else 0) + (((d["num_precommitted"] + 2047) // 2048) if d["num_precommitted_unpadded"] else 0) \
        + (d["num_rest"] + 2047) // 2048
    lx = (d["num_cons"] - 1).bit_length()
    off_pub = 8 * rows
    off_outer = off_pub + 4 * d["num_public"]
    off_claims = off_outer + 12 * lx
    off_inner = off_claims + 12
    n = len(words)
    # the tamperings of tests/test_gpu_verify.py: publics, an outer polynomial, a claim, an inner polynomial, eval_W, z_vec, z_beta
    positions = [p for p in (off_pub if d["num_public"] else None, off_outer + 5, off_claims + 1, off_inner + 2,
                             n - 8 - 4 * min(2048, d["num_shared"] + d["num_precommitted"] + d["num_rest"]) - 16 - 8, n - 8 - 3, n - 1) if p is not None]
    items = [(words, 0)]
    assert osp.verify_words(words) == 0
    for pos in positions:
        bad = words.copy()
        bad[pos] ^= np.uint64(1)
        want = osp.verify_words(bad)
        assert want != 0 and sn.verify(bad) == want
        items.append((bad, want))
    _proofs[which] = (sn, items)
    return _proofs[which]


@pytest.mark.parametrize("device", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("which", CIRCUITS)
def test_verifier_agrees_with_the_oracle_and_the_prover_key(ctx, which, device):
    inst, osp, vk, dig = oracle(which)
    sn, items = proofs_of(ctx, which)
    v = host.SpartanVerifier.from_bytes(ctx, vk, device_decode=device)
    assert v.stages["device"] == (1.0 if device else 0.0)
    assert v.vk_digest.tobytes() == dig and v.dims == sn.dims
    assert v.shape_info["nnz"] == sn.shape_info["nnz"] and v.shape_info["nnz_filtered"] == [0, 0, 0]
    for words, want in items:
        assert v.verify(words) == want
        assert v.verify_bytes(sn.proof_to_bytes(words)) == want
    assert v.verify_bytes(b"") == 1 and v.verify(items[0][0][:-1]) == 1
    for K in (1, 3, 9):
        pick = [items[(2 * k + K) % len(items)] for k in range(K)]
        if K > 1:
            pick[K // 2] = items[0]  # good and bad mixed
        want = [w for _, w in pick]
        assert v.verify_batch([p for p, _ in pick]) == want
        assert v.verify_bytes_batch([sn.proof_to_bytes(p) for p, _ in pick], seed=bytes(range(32))) == want
        assert sn.verify_batch([p for p, _ in pick]) == want
    other = CIRCUITS[(CIRCUITS.index(which) + 1) % len(CIRCUITS)]
    vo = host.SpartanVerifier.from_bytes(ctx, oracle(other)[2], device_decode=device)
    assert vo.verify(items[0][0]) != 0 and vo.verify_bytes(sn.proof_to_bytes(items[0][0])) != 0  # another circuit's key rejects a good proof
    vo.close()
    v.close()


def test_every_prover_entry_point_refuses_a_verifier_only_key(ctx):
    inst, osp, vk, dig = oracle("cubic")
    v = host.SpartanVerifier.from_bytes(ctx, vk)
    L = host.lib()
    L.ss_vk_to_bytes.restype = ctypes.c_long
    tape = ol.make_tape(1, 64)
    w = np.zeros(64, dtype=np.uint64)
    used, out, one = ctypes.c_size_t(0), ctypes.c_void_p(), ctypes.c_size_t(1)
    words = np.zeros(1 << 16, dtype=np.uint64)
    pubs = np.zeros(256, dtype=np.uint64)
    fake = ctypes.c_void_p(words.ctypes.data)  # a non-null stand-in for handles that must not be reached
    tapes, blocks, wits, outs = (hip.c_u8p * 1)(hip.p8(tape)), (ctypes.c_size_t * 1)(64), (hip.c_u64p * 1)(hip.p64(w)), (ctypes.c_void_p * 1)()
    pks, pss = (ctypes.c_void_p * 1)(v.pk), (ctypes.c_void_p * 1)(fake)
    args, keep = host._inst_args(inst)
    calls = {
        "ss_prep_prove": lambda: L.ss_prep_prove(v.pk, hip.p64(w), one, 1, hip.p8(tape), ctypes.c_size_t(64), ctypes.byref(used), ctypes.byref(out)),
        "ss_prep_prove_sha256": lambda: L.ss_prep_prove_sha256(v.pk, fake, hip.p8(tape), ctypes.c_size_t(3), 1, hip.p8(tape), ctypes.c_size_t(64), ctypes.byref(used),
                                                               ctypes.byref(out), hip.p64(pubs)),
        "ss_prep_prove_batch": lambda: L.ss_prep_prove_batch(v.pk, wits, one, one, 1, tapes, blocks, None, outs, None),
        "ss_prep_prove_sha256_batch": lambda: L.ss_prep_prove_sha256_batch(v.pk, fake, hip.p8(tape), ctypes.c_size_t(3), one, 1, tapes, blocks, None, outs, hip.p64(pubs), None),
        "ss_prep_is_sat": lambda: L.ss_prep_is_sat(v.pk, fake, None, ctypes.c_size_t(0), None, None, None, None, None, None, ctypes.c_size_t(0), None),
        "ss_prove": lambda: L.ss_prove(v.pk, fake, None, ctypes.c_size_t(0), hip.p8(tape), ctypes.c_size_t(64), ctypes.byref(used), hip.p64(words), ctypes.c_size_t(len(words)), None),
        "ss_prove_batch": lambda: L.ss_prove_batch(v.pk, pss, one, None, ctypes.c_size_t(0), tapes, blocks, None, hip.p64(words), ctypes.c_size_t(len(words)), None),
        "ss_prove_multiplexed": lambda: L.ss_prove_multiplexed(pks, pss, one, None, ctypes.c_size_t(0), hip.p8(tape), ctypes.c_size_t(64), one, one, hip.p64(words),
                                                               ctypes.c_size_t(len(words)), None),
        "ss_vk_to_bytes": lambda: L.ss_vk_to_bytes(v.pk, *args, None, ctypes.c_size_t(0)),
    }
    for name, call in calls.items():
        host.lib().ss_set_error(b"")
        rc = call()
        assert rc < 0, name
        assert "verifier-only key" in L.ss_last_error().decode(), (name, L.ss_last_error().decode())
    assert v.verify(proofs_of(ctx, "cubic")[1][0][0]) == 0  # the key still verifies
    v.close()


# ---- 6. mid-size -------------------------------------------------------------------------------------------------------------------------------------------
def test_mid_size_key_loads_and_verifies(ctx):
    inst, osp, vk, dig = oracle("sha256_64B")  # 65536 constraints
    sn = host.SpartanSNARK(ctx, inst)
    tape = ol.make_tape(88, 4096)
    used = sn.prep_prove(tape)
    words, _, _ = sn.prove(tape[used:])
    for device in FORMS:
        v = host.SpartanVerifier.from_bytes(ctx, vk, device_decode=device)
        assert v.vk_digest.tobytes() == dig and v.shape_info["nnz"] == sn.shape_info["nnz"]
        assert v.verify(words) == 0
        bad = words.copy()
        bad[len(bad) // 2] ^= np.uint64(4)
        assert v.verify(bad) == sn.verify(bad) != 0
        v.close()
    sn.close()
