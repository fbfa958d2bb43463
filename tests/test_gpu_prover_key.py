"""GPU checks of the prover key that is loaded from its bytes: the full R1CS shape built on the device (hip.Shape.from_wire(.., full_device=True):
kernels_wire_full.hpp), SpartanSNARK.pk_to_bytes and host.SpartanProver. Nothing expected comes from the code under test: the reference structure is
sp_shape_from_csr's (hip.Shape over the same matrices, through sp_shape_compare), key bytes and digests are the CPU oracle's, field sums are
orc_shape_* or Python integers, proofs are OracleSpartan's, verdicts tests/pyverify.py's; the crafted streams are written by the small bincode writer below
(model: tests/test_gpu_verifier_key.py)."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import pyverify
from spartan2_amd import frontend, hip, host
from spartan2_amd.host import pad_shape

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ol.MODULI[0]
RINV = pow(ol.R, -1, P)
# the sort kernels' tile and digit width and the scan tile, named here and pinned to the library's by tests/test_prover_key_cpu.py
FULL_SORT_TILE = 2048
FULL_SORT_BITS = 8
WIRE_SCAN_TILE = 1024
LONG_COLUMN = 512  # a column with this many entries over A, B, C is walked by blocks (capi_sparse.hip)
# column counts: one, two and three 8-bit digits of a walk position, both sides of a scan tile of the column pointers and of every digit boundary
COLUMN_COUNTS = sorted({1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 65537, (1 << FULL_SORT_BITS) - 1, 1 << FULL_SORT_BITS, (1 << FULL_SORT_BITS) + 1,
                        (1 << 2 * FULL_SORT_BITS) - 1, 1 << 2 * FULL_SORT_BITS, (1 << 2 * FULL_SORT_BITS) + 1, WIRE_SCAN_TILE - 1, WIRE_SCAN_TILE, WIRE_SCAN_TILE + 1})
ENTRY_COUNTS = [FULL_SORT_TILE - 1, FULL_SORT_TILE, FULL_SORT_TILE + 1, 2 * FULL_SORT_TILE - 1, 2 * FULL_SORT_TILE, 2 * FULL_SORT_TILE + 1]


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
    """the oracle's key of a circuit, made once: (instance, OracleSpartan, verifier key bytes, digest bytes)"""
    if which not in _oracles:
        inst = _circuit(which)
        osp = ol.OracleSpartan(inst)
        _oracles[which] = (inst, osp, osp.vk_bytes(), osp.export_keys()[4].tobytes())
    return _oracles[which]


def shape_offset(vk):
    o = 0
    for _ in range(2):
        o += 16 + 64 * struct.unpack_from("<Q", vk, o + 8)[0] + 96
    return o


# ---- a bincode writer of SplitR1CSShape ----------------------------------------------------------------------------------------------------------------
DIM_ORDER = ("num_cons", "num_cons_unpadded", "num_shared_unpadded", "num_precommitted_unpadded", "num_rest_unpadded", "num_shared", "num_precommitted", "num_rest",
             "num_public", "num_challenges")  # field order of SplitR1CSShape (src/r1cs/mod.rs:743-755)


def u64(v):
    return struct.pack("<Q", int(v))


def matrix_bytes(data, idx, ptr, cols):
    return (u64(len(data)) + b"".join(int(v).to_bytes(32, "little") for v in data) + u64(len(idx)) + np.asarray(idx, dtype="<u8").tobytes() + u64(len(ptr))
            + np.asarray(ptr, dtype="<u8").tobytes() + u64(cols))


def shape_bytes(dims, mats):
    cols = dims["num_shared"] + dims["num_precommitted"] + dims["num_rest"] + 1 + dims["num_public"] + dims["num_challenges"]
    return b"".join(u64(dims[k]) for k in DIM_ORDER) + b"".join(matrix_bytes(d, i, p_, cols) for d, i, p_ in mats)


def make_dims(rows, cols, rows_used=None, shared=0, precommitted=0, public=0):
    """cols = shared + precommitted + rest + 1 + public; the filter keeps columns >= shared + precommitted"""
    d = dict.fromkeys(DIM_ORDER, 0)
    rest = cols - 1 - public - shared - precommitted
    assert rest >= 0
    d.update(num_cons=rows, num_cons_unpadded=rows if rows_used is None else rows_used, num_shared=shared, num_shared_unpadded=shared, num_precommitted=precommitted,
             num_precommitted_unpadded=precommitted, num_rest=rest, num_rest_unpadded=rest, num_public=public)
    return d


def raw_ints(limbs):
    b = np.ascontiguousarray(limbs, dtype="<u8").tobytes()
    return [int.from_bytes(b[32 * i: 32 * i + 32], "little") for i in range(len(b) // 32)]


def raw_limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def random_residues(rng, n):
    raw = rng.bytes(32 * n)
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") % P for i in range(n)]


SMALL = [k for k in range(1, 8)] + [P - k for k in range(1, 8)]  # the fourteen coded values: +-1 .. +-7
GENERAL = [8, P - 8, 0, 1 << 64]


def coeffs(rng, n, kind):
    if kind == "small":
        pool = SMALL
    elif kind == "general":
        pool = GENERAL + random_residues(rng, 4)
    else:
        pool = SMALL + GENERAL + random_residues(rng, 6)
    return [pool[int(i)] for i in rng.integers(0, len(pool), n)]


def matrix_of(rows, entries):
    """entries: (row, column, coefficient) in any order of rows; inside a row the order given is the order of the stream -> (data, idx, indptr)"""
    by_row = sorted(range(len(entries)), key=lambda k: entries[k][0])  # (stable)
    data, idx, ptr = [], [], [0] * (rows + 1)
    for k in by_row:
        r, c, v = entries[k]
        data.append(v)
        idx.append(c)
        ptr[r + 1] += 1
    for r in range(rows):
        ptr[r + 1] += ptr[r]
    return data, idx, ptr


def random_entries(rng, rows, cols, n, kind="mixed", hit=()):
    cs = [int(c) for c in rng.integers(0, cols, n)]
    for k, c in enumerate(hit):  # columns that must occur
        if k < n:
            cs[k] = c
    rs = [int(r) for r in rng.integers(0, rows, n)]
    return list(zip(rs, cs, coeffs(rng, n, kind)))


def expected_poly_abc(dims, mats, cols, x, r):
    """Python integers. With x~, r~ the limbs of the tables as they are: a coefficient c contributes c x~[row] to its column, and a product by r~ is a
    Montgomery product, r~ R^-1. Rows at and past num_cons_unpadded contribute nothing."""
    rho = r * RINV % P
    out = [0] * cols
    for m, (data, idx, ptr) in enumerate(mats):
        w = pow(rho, m, P)
        for row in range(dims["num_cons_unpadded"]):
            for k in range(ptr[row], ptr[row + 1]):
                out[idx[k]] = (out[idx[k]] + w * data[k] * x[row]) % P
    return out


def check_stream(ctx, dims, mats, seed=1, host_form=False):
    """the stream's full device shape == sp_shape_from_csr's over the same matrices (every array), twice, and poly_abc == Python integers"""
    rows = dims["num_cons"]
    cols = dims["num_shared"] + dims["num_precommitted"] + dims["num_rest"] + 1 + dims["num_public"] + dims["num_challenges"]
    blob = shape_bytes(dims, mats)
    ref = hip.Shape(ctx, [(ol.mont_array(d) if len(d) else np.zeros((0, 4), dtype=np.uint64), np.asarray(i, dtype=np.uint32), np.asarray(p_, dtype=np.uint64)) for d, i, p_ in mats],
                    dims)
    dev = hip.Shape.from_wire(ctx, blob, full_device=True)
    assert dev.compare(ref) == "" and ref.compare(dev) == ""
    assert dev.info() == ref.info()
    again = hip.Shape.from_wire(ctx, blob, full_device=True, timed=True)
    assert again.compare(dev) == ""
    want_passes = max(1, -(-(cols - 1).bit_length() // FULL_SORT_BITS))
    assert again.full_stages["sort_passes"] == want_passes
    if host_form:
        assert hip.Shape.from_wire(ctx, blob, full=True).compare(dev) == ""
    rng = np.random.default_rng(seed)
    x, r = random_residues(rng, rows), random_residues(rng, 1)[0]
    want = expected_poly_abc(dims, mats, cols, x, r)
    rx, out = hip.Table.from_host(ctx, raw_limbs(x)), hip.Table.from_host(ctx, raw_limbs(random_residues(rng, 1) * cols))  # (a dirty output)
    dev.poly_abc(rx, raw_limbs([r])[0], cols, out)
    got = raw_ints(out.read(0, cols))
    bad = [c for c in range(cols) if got[c] != want[c]]
    assert not bad, f"poly_abc: columns {bad[:8]} differ (of {len(bad)})"
    rx.free()
    out.free()
    return dev, ref


# ---- 1. the circuits' shapes against sp_shape_from_csr and the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CIRCUITS)
def test_full_device_shape_equals_from_csr_and_the_oracle(ctx, which):
    inst, osp, vk, _ = oracle(which)
    blob = vk[shape_offset(vk):]
    mats, dims = pad_shape(inst)
    ref = hip.Shape(ctx, mats, dims)
    dev = hip.Shape.from_wire(ctx, blob, full_device=True)
    assert dev.compare(ref) == ""
    assert hip.Shape.from_wire(ctx, blob, full_device=True).compare(dev) == ""  # two loads of the same bytes
    assert dev.dims == dims and dev.info() == ref.info() and dev.info()["short_columns"] > 0
    assert hip.Shape.from_wire(ctx, blob).compare(dev).startswith("row_only")  # a row-only shape differs from a full one by name
    assert hip.Shape.from_wire(ctx, blob).compare(hip.Shape.from_wire(ctx, blob, device_decode=False)) == ""  # ... and compares its row[] alone
    oshape = osp.shape
    N, M, ncols = oshape.num_cons, oshape.num_vars, oshape.num_vars + oshape.num_extra
    rng = np.random.default_rng(20261021 + len(which))
    z = ol.random_field_array(rng, ncols)
    want = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
    assert ol.lib().orc_shape_multiply_vec(oshape.h, ol.p64(z), *(ol.p64(w) for w in want)) == 0
    outs = [hip.Table.zeros(ctx, N) for _ in range(3)]
    zt = hip.Table.from_host(ctx, z)
    dev.multiply_vec(zt, *outs)
    for o, w in zip(outs, want):
        assert (o.read() == w).all()
    zc = z.copy()
    zc[oshape.num_shared + oshape.num_precommitted:] = 0
    cached = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
    assert ol.lib().orc_shape_multiply_vec(oshape.h, ol.p64(zc), *(ol.p64(w) for w in cached)) == 0
    want = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
    assert ol.lib().orc_shape_multiply_vec_incremental(oshape.h, ol.p64(z), *(ol.p64(c) for c in cached), *(ol.p64(w) for w in want)) == 0
    ct = [hip.Table.from_host(ctx, c) for c in cached]
    dev.multiply_vec_incremental(zt, *ct, *outs)
    for o, w in zip(outs, want):
        assert (o.read() == w).all()
    rx, r = ol.random_field_array(rng, N), ol.random_field_array(rng, 1)[0]
    rxt = hip.Table.from_host(ctx, rx)
    for out_len in (ncols, 2 * M):
        want_abc = np.zeros((out_len, 4), dtype=np.uint64)
        assert ol.lib().orc_shape_poly_abc(oshape.h, ol.p64(rx), ol.p64(r), ctypes.c_size_t(out_len), ol.p64(want_abc)) == 0
        out = hip.Table.from_host(ctx, ol.random_field_array(rng, 16).repeat((2 * M + 15) // 16, axis=0)[: 2 * M])  # dirty buffer
        dev.poly_abc(rxt, r, out_len, out)
        assert (out.read(0, out_len) == want_abc).all()
        out.free()
    for t in outs + ct + [zt, rxt]:
        t.free()


# ---- 2. hand-written streams -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", COLUMN_COUNTS)
def test_column_counts(ctx, cols):
    rng = np.random.default_rng(3000 + cols)
    rows = 33
    mats = [matrix_of(rows, random_entries(rng, rows, cols, n, hit=(cols - 1, 0, cols // 2))) for n in (700, 450, 300)]
    check_stream(ctx, make_dims(rows, cols), mats, seed=cols, host_form=cols in (1, 257))


@pytest.mark.parametrize("n", ENTRY_COUNTS)
def test_entry_counts_around_the_sort_tiles(ctx, n):
    rng = np.random.default_rng(4000 + n)
    rows, cols = 70, 300
    mats = [matrix_of(rows, random_entries(rng, rows, cols, k)) for k in (n, n - 1000, 17)]
    check_stream(ctx, make_dims(rows, cols), mats, seed=n)


@pytest.mark.parametrize("total", [LONG_COLUMN - 1, LONG_COLUMN, LONG_COLUMN + 1])
def test_a_column_at_the_long_threshold(ctx, total):
    """column 7 holds 200 + 200 + (111 | 112 | 113) entries of A, B, C: short at 511, long from 512 on; the other columns stay short"""
    rng = np.random.default_rng(5000 + total)
    rows, cols = 260, 40
    mats = []
    for m, n7 in enumerate((200, 200, total - 400)):
        es = [(r, 7, v) for r, v in zip(range(n7), coeffs(rng, n7, "mixed"))] + [e for e in random_entries(rng, rows, cols, 150) if e[1] != 7]
        mats.append(matrix_of(rows, es))
    dev, _ = check_stream(ctx, make_dims(rows, cols), mats, seed=total)
    assert dev.info()["long_columns"] == (1 if total >= LONG_COLUMN else 0)


def test_two_long_columns_and_a_matrix_in_one_column(ctx):
    """all of A in column 5 (700 entries, several to a row); B spread, with 600 entries in the last column; C empty beside the two"""
    rng = np.random.default_rng(6000)
    rows, cols = 90, 270
    A = matrix_of(rows, [(int(r), 5, v) for r, v in zip(rng.integers(0, rows, 700), coeffs(rng, 700, "mixed"))])
    B = matrix_of(rows, [(int(r), cols - 1, v) for r, v in zip(rng.integers(0, rows, 600), coeffs(rng, 600, "small"))] + random_entries(rng, rows, cols - 1, 400))
    C = ([], [], [0] * (rows + 1))
    dev, _ = check_stream(ctx, make_dims(rows, cols), [A, B, C], seed=6, host_form=True)
    assert dev.info()["long_columns"] == 2 and dev.info()["nnz"] == [700, 1000, 0]
    for order in ([B, C, A], [C, A, B]):  # the empty matrix in each place
        check_stream(ctx, make_dims(rows, cols), order, seed=7)


def test_duplicates_keep_the_order_of_the_stream(ctx):
    """the same (row, column) twice, a small and a general coefficient in either order, in a short and in a long column"""
    rng = np.random.default_rng(7000)
    rows, cols = 300, 20
    es = []
    for r in range(rows):
        pair = [(r, 3, 2), (r, 3, 11)] if r % 2 else [(r, 3, 11), (r, 3, P - 1)]
        es += pair + [(r, 9, 5), (r, 9, 5)] * (r < 4) + [(r, 11, 0), (r, 11, 3), (r, 11, 0)] * (r == 17)
    mats = [matrix_of(rows, es), matrix_of(rows, es[::-1]), matrix_of(rows, es[: len(es) // 3])]
    dev, _ = check_stream(ctx, make_dims(rows, cols), mats, seed=8)
    assert dev.info()["long_columns"] == 1


@pytest.mark.parametrize("rows_used", [0, 1, 16, 31, 32])
def test_rows_at_and_past_num_cons_unpadded_stay_in_row_only(ctx, rows_used):
    rng = np.random.default_rng(8000 + rows_used)
    rows, cols = 32, 50
    mats = [matrix_of(rows, random_entries(rng, rows, cols, n) + [(rows - 1, 4, 9), (min(rows_used, rows - 1), 4, 3)]) for n in (400, 300, 20)]
    dims = make_dims(rows, cols, rows_used=rows_used)
    dev, _ = check_stream(ctx, dims, mats, seed=rows_used)
    used = [m[2][rows_used] for m in mats]
    assert dev.info()["nnz"] == [len(m[0]) for m in mats] and dev.info()["nnz_filtered"] == used


@pytest.mark.parametrize("split", ["none", "all", "middle"])
def test_the_filter_boundary(ctx, split):
    """columns col_min - 1 and col_min, with num_shared + num_precommitted of 0, of all variables, and in between"""
    rng = np.random.default_rng(9000 + len(split))
    rows, cols, public = 40, 64, 3
    nvars = cols - 1 - public
    shared, pre = {"none": (0, 0), "all": (nvars // 2, nvars - nvars // 2), "middle": (11, 20)}[split]
    col_min = shared + pre
    hit = [c for c in (col_min - 1, col_min, col_min + 1, cols - 1, 0) if 0 <= c < cols]
    mats = [matrix_of(rows, random_entries(rng, rows, cols, n, hit=hit * 3)) for n in (500, 300, 100)]
    dims = make_dims(rows, cols, shared=shared, precommitted=pre, public=public)
    dev, _ = check_stream(ctx, dims, mats, seed=len(split))
    assert dev.info()["nnz_filtered"] == [sum(1 for c in m[1] if c >= col_min) for m in mats]


@pytest.mark.parametrize("kind", ["small", "general", "mixed", "zeros"])
def test_coefficient_classes(ctx, kind):
    rng = np.random.default_rng(10000 + len(kind))
    rows, cols = 65, 129
    if kind == "zeros":
        mats = [matrix_of(rows, [(r, c, 0) for r, c, _ in random_entries(rng, rows, cols, n)]) for n in (300, 200, 100)]
    else:
        mats = [matrix_of(rows, random_entries(rng, rows, cols, n, kind=kind)) for n in (900, 300, 100)]
    check_stream(ctx, make_dims(rows, cols), mats, seed=len(kind))


@pytest.mark.parametrize("cols", [1, 600])
def test_one_constraint(ctx, cols):
    rng = np.random.default_rng(11000 + cols)
    mats = [matrix_of(1, random_entries(rng, 1, cols, n)) for n in (520 if cols == 1 else 700, 3, 0)]
    check_stream(ctx, make_dims(1, cols), mats, seed=cols)
    check_stream(ctx, make_dims(1, cols, rows_used=0), mats, seed=cols)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def raw_from_wire(ctx, blob, flags):
    """sp_shape_from_wire with any flag word -> (rc, message); a shape that comes back is freed"""
    buf = np.frombuffer(bytes(blob), dtype=np.uint8)
    L = hip.lib()
    r, h, dd = ctypes.c_void_p(), ctypes.c_void_p(), hip._Dims()
    assert L.sp_unwire_new(hip.p8(buf), ctypes.c_size_t(len(buf)), ctypes.byref(r)) == 0
    rc = L.sp_shape_from_wire(ctx.h, r, ctypes.c_uint(flags), ctypes.byref(dd), ctypes.byref(h))
    L.sp_unwire_free(r)
    if h:
        L.sp_shape_free(h)
    return rc, L.sp_last_error().decode()


def tiny():
    rows, cols = 6, 9
    rng = np.random.default_rng(99)
    return rows, cols, [matrix_of(rows, random_entries(rng, rows, cols, n)) for n in (8, 5, 7)]


def test_flag_combinations(ctx):
    rows, cols, mats = tiny()
    blob = shape_bytes(make_dims(rows, cols), mats)
    D, H, F, T, FD = hip.SHAPE_WIRE_DEVICE, hip.SHAPE_WIRE_HOST, hip.SHAPE_WIRE_FULL, hip.SHAPE_WIRE_TIMED, hip.SHAPE_WIRE_FULL_DEVICE
    assert (D, H, F, T, FD) == (1, 2, 4, 8, 16)
    today = "flags that exclude each other (the device decode builds the row-only shape; the full shape takes the host decode)"
    for flags in (D | F, D | H, D | H | F, 32, 64 | FD, 1 << 16, D | F | T):  # refused before this change, with the same words
        rc, msg = raw_from_wire(ctx, blob, flags)
        assert rc == -1 and today in msg, flags
    for flags in (FD | D, FD | H, FD | F, FD | D | T, FD | F | H):
        rc, msg = raw_from_wire(ctx, blob, flags)
        assert rc == -1 and "exclude each other" in msg, flags
    for flags in (FD, FD | T, F, F | H, F | T, 0, D, H, T):
        assert raw_from_wire(ctx, blob, flags)[0] == 0, flags
    with pytest.raises(hip.SpartanHipError, match="exclude each other"):
        hip.Shape.from_wire(ctx, blob, full=True, full_device=True)
    assert hip.Shape.from_wire(ctx, blob, full=True).stages["device"] == 0.0  # SP_SHAPE_WIRE_FULL alone stays the host decode
    assert hip.Shape.from_wire(ctx, blob, full_device=True).stages["device"] == 1.0


def free_bytes():
    import torch

    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_full_device_refusals_are_the_row_decodes_and_leak_nothing(ctx):
    rows, cols, mats = tiny()
    dims = make_dims(rows, cols)
    good = shape_bytes(dims, mats)
    FD = hip.SHAPE_WIRE_FULL_DEVICE
    assert raw_from_wire(ctx, good, FD)[0] == 0  # (the allocator's pools are warm before the first reading)
    bad_coeff = [(list(d), i, p_) for d, i, p_ in mats]
    bad_coeff[1][0][2] = P
    bad_index = [(d, list(i), p_) for d, i, p_ in mats]
    bad_index[2][1][-1] = cols
    before = free_bytes()
    for blob, match, m, at in ((shape_bytes(dims, bad_coeff), "non-canonical field element at entry", "B", 2),
                               (shape_bytes(dims, bad_index), "column index out of range at entry", "C", len(mats[2][0]) - 1)):
        for _ in range(3):
            rc, msg = raw_from_wire(ctx, blob, FD)
            assert rc == -1 and f"sp_shape_from_wire: {match} {at} of matrix {m}" == msg
            assert raw_from_wire(ctx, blob, hip.SHAPE_WIRE_DEVICE)[1] == msg  # word for word the row-only decode's
    for cut in (0, 79, 80, len(good) - 1):
        assert raw_from_wire(ctx, good[:cut] if cut else b"\0", FD)[0] == -1
    assert free_bytes() == before
    check_stream(ctx, dims, mats)  # the context still serves a good stream


# ---- 4. the three SPARTAN_POLYABC_* settings, in child processes -----------------------------------------------------------------------------------------------
CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import test_gpu_prover_key as t
from spartan2_amd import hip
ctx = hip.Context(0)
rng = np.random.default_rng(12000)
rows, cols = 120, 3000
es = [(r, 9, 3) for r in range(rows)] * 5
mats = [t.matrix_of(rows, t.random_entries(rng, rows, cols, n) + es[: k]) for n, k in ((2500, 600), (1500, 0), (300, 40))]
dev, ref = t.check_stream(ctx, t.make_dims(rows, cols, rows_used=rows - 3, shared=100, precommitted=50, public=2), mats, seed=12, host_form=True)
info = dev.info()
assert info["long_columns"] == 1 and info["short_columns"] == cols - 1
print("POLYABC_CHILD_OK", dev.compare(ref) == "")
"""
SETTINGS = ["SPARTAN_POLYABC_LAYOUT=natural", "SPARTAN_POLYABC_ORDER=natural", "SPARTAN_POLYABC_ORDER=window", "SPARTAN_POLYABC_ORDER=window SPARTAN_POLYABC_WINDOW=1",
            "SPARTAN_POLYABC_ORDER=window SPARTAN_POLYABC_WINDOW=777", "SPARTAN_POLYABC_LAYOUT=natural SPARTAN_POLYABC_ORDER=window SPARTAN_POLYABC_WINDOW=777"]


@pytest.mark.parametrize("setting", SETTINGS)
def test_polyabc_settings_give_from_csrs_arrays(setting):
    env = dict(os.environ)
    for kv in setting.split():
        k, v = kv.split("=", 1)
        env[k] = v
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "POLYABC_CHILD_OK True" in p.stdout, (setting, p.stdout[-2000:], p.stderr[-4000:])


# ---- 5. the prover -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gens():
    return host.from_label(b"ck", 2049), host.from_label(b"ck_s", 2)


@pytest.mark.parametrize("which", CIRCUITS + ["sha256_64B"])
def test_pk_to_bytes_is_the_oracles_key_and_digest(ctx, which):
    inst, osp, vk, dig = oracle(which)
    sn = host.SpartanSNARK(ctx, inst)
    got = sn.pk_to_bytes()
    assert len(got) == len(vk) + 32 and got == vk + dig
    sn.close()


def python_verdict(inst, gens, prover, words):
    g, g_s = gens
    return pyverify.verify_bytes(inst, g[:2048], g[2048], g_s[0], g_s[1], prover.proof_to_bytes(words), vk_digest=prover.vk_digest.tobytes())


@pytest.mark.parametrize("full_device", [True, False, None], ids=["device", "host", "default"])
@pytest.mark.parametrize("which", CIRCUITS)
def test_loaded_prover_proves_what_the_oracle_and_setup_prove(ctx, gens, which, full_device):
    inst, osp, vk, dig = oracle(which)
    pr = host.SpartanProver.from_bytes(ctx, vk + dig, full_device=full_device)
    sn = host.SpartanSNARK(ctx, inst)
    assert pr.vk_digest.tobytes() == dig and pr.dims == sn.dims and pr.shape_info == sn.shape_info
    if full_device is not None:
        assert pr.load_stages["full_device"] == (1.0 if full_device else 0.0)
    assert pr.load_stages["digest_hashed"] == 1.0
    prep, tape = ol.make_tape(500 + len(which), 4096), ol.make_tape(600 + len(which), 4096)
    want_used = osp.prep_prove(prep)
    want, want_pused, _ = osp.prove(tape)
    assert pr.prep_prove(prep, inst.witness, inst.publics) == want_used == sn.prep_prove(prep)
    words, used, _ = pr.prove(tape)
    words_setup, _, _ = sn.prove(tape)
    assert used == want_pused and (words == want).all() and (words == words_setup).all()
    assert pr.is_sat().ok
    # accepted by the loaded prover, by a verifier loaded from the first len - 32 bytes, and by the Python-integer verifier
    v = host.SpartanVerifier.from_bytes(ctx, (vk + dig)[:-32])
    assert pr.verify(words) == 0 and v.verify(words) == 0 and v.verify_bytes(pr.proof_to_bytes(words)) == 0
    assert python_verdict(inst, gens, pr, words) == [int(x) for x in inst.publics]
    bad = words.copy()
    bad[len(bad) // 2] ^= np.uint64(1)
    assert pr.verify(bad) == v.verify(bad) != 0
    # the batch: two states of the same witness on two tapes
    preps = [ol.make_tape(700 + k, 4096) for k in range(2)]
    tapes = [ol.make_tape(800 + k, 4096) for k in range(2)]
    prep_used = pr.prep_prove_batch(preps, witnesses=[inst.witness] * 2, publics=[inst.publics] * 2)
    assert prep_used == sn.prep_prove_batch(preps)
    got, _ = pr.prove_batch(tapes)
    ref, _ = sn.prove_batch(tapes)
    for k in range(2):
        o = ol.OracleSpartan(inst)
        assert o.prep_prove(preps[k]) == prep_used[k]
        want_k, want_used_k, _ = o.prove(tapes[k])
        assert got[k][1] == want_used_k == ref[k][1] and (got[k][0] == want_k).all() and (got[k][0] == ref[k][0]).all()
        assert v.verify(got[k][0]) == 0
    # a wrong witness is found
    wrong = np.array(inst.witness, dtype=np.uint64).copy()
    wrong[0] ^= np.uint64(1)
    pr.prep_prove(prep, wrong, inst.publics)
    rep = pr.is_sat()
    assert not rep.ok
    # the byte forms refuse a loaded key: the caller holds the bytes
    L = host.lib()
    L.ss_pk_to_bytes.restype = L.ss_vk_to_bytes.restype = ctypes.c_long
    args, keep = host._inst_args(inst)
    out = np.zeros(len(vk) + 32, dtype=np.uint8)
    for fn in (L.ss_pk_to_bytes, L.ss_vk_to_bytes):
        assert fn(pr.pk, *args, None, ctypes.c_size_t(0)) < 0 and "keep those" in L.ss_last_error().decode()  # the sizing pass already
        assert fn(pr.pk, *args, hip.p8(out), ctypes.c_size_t(len(out))) < 0 and "keep those" in L.ss_last_error().decode()
    for o in (v, pr, sn):
        o.close()


def test_loaded_prover_generates_sha256_witnesses(ctx, gens):
    """prep_prove_sha256 and prep_prove_batch(msgs=) on the loaded key: no instance, the message bytes alone"""
    inst0, osp0, vk, dig = oracle("sha256_1block")
    pr = host.SpartanProver.from_bytes(ctx, vk + dig)
    msgs = [b"abc", b"xyz", b"\0\1\2"]
    insts = [frontend.sha256_circuit(m) for m in msgs]
    prep, tape = ol.make_tape(901, 4096), ol.make_tape(902, 8192)
    osp = ol.OracleSpartan(insts[1])
    want_used = osp.prep_prove(prep)
    want, want_pused, _ = osp.prove(tape)
    assert pr.prep_prove_sha256(msgs[1], prep) == want_used
    assert (pr.publics == insts[1].publics).all()
    words, used, _ = pr.prove(tape)
    assert used == want_pused and (words == want).all() and pr.verify(words) == 0
    assert python_verdict(insts[1], gens, pr, words) == [int(x) for x in insts[1].publics]
    preps = [ol.make_tape(910 + k, 4096) for k in range(3)]
    tapes = [ol.make_tape(920 + k, 8192) for k in range(3)]
    pr.prep_prove_batch(preps, msgs=msgs)
    got, _ = pr.prove_batch(tapes)
    for k in range(3):
        o = ol.OracleSpartan(insts[k])
        o.prep_prove(preps[k])
        want_k, want_used_k, _ = o.prove(tapes[k])
        assert got[k][1] == want_used_k and (got[k][0] == want_k).all()
    pr.close()


def key_refused(ctx, blob, match, **kw):
    with pytest.raises(hip.SpartanHipError, match=match):
        host.SpartanProver.from_bytes(ctx, blob, **kw)


def test_prover_key_refusals(ctx):
    inst, osp, vk, dig = oracle("cubic")
    pkb = vk + dig
    for at in (len(pkb) - 32, len(pkb) - 1, len(pkb) - 17):
        bad = bytearray(pkb)
        bad[at] ^= 1
        key_refused(ctx, bytes(bad), "vk_digest")
        pr = host.SpartanProver.from_bytes(ctx, bytes(bad), trust_digest=True)  # as the reference's Deserialize takes it
        assert pr.load_stages["digest_hashed"] == 0.0 and pr.vk_digest.tobytes() == bytes(bad[-32:])
        if at == len(pkb) - 1:  # its proofs are rejected by the verifier with the right key
            tape = ol.make_tape(33, 4096)
            pr.prep_prove(tape, inst.witness, inst.publics)
            words, _, _ = pr.prove(ol.make_tape(34, 4096))
            v = host.SpartanVerifier.from_bytes(ctx, vk)
            assert v.verify(words) != 0 and osp.verify_words(words) != 0
            v.close()
        pr.close()
    bad = bytearray(pkb)
    bad[shape_offset(vk) + 100] ^= 1  # a byte of the key itself: the stored digest no longer matches
    key_refused(ctx, bytes(bad), "vk_digest|non-canonical|out of range|indptr|length")
    for cut in (0, 1, 31, 32, 33, len(vk) // 2, len(vk) - 1, len(vk), len(vk) + 1, len(vk) + 31):  # short bytes; a truncated digest
        key_refused(ctx, pkb[:cut], "unexpected end of input|length prefix exceeds the input|no bytes")
    key_refused(ctx, pkb + b"\0", "trailing bytes")
    key_refused(ctx, vk + b"\0" + dig, "trailing bytes")
    L = host.lib()
    out = ctypes.c_void_p()
    buf = np.frombuffer(pkb, dtype=np.uint8)
    for flags in (hip.SHAPE_WIRE_DEVICE, hip.SHAPE_WIRE_HOST):
        assert L.ss_prover_from_bytes(ctx.h, hip.p8(buf), ctypes.c_size_t(len(buf)), ctypes.c_uint(flags), ctypes.byref(out)) == -1 and not out.value
        assert "a prover's key holds the full shape" in L.ss_last_error().decode()
    assert L.ss_prover_from_bytes(ctx.h, hip.p8(buf), ctypes.c_size_t(len(buf)), ctypes.c_uint(hip.SHAPE_WIRE_FULL | hip.SHAPE_WIRE_FULL_DEVICE), ctypes.byref(out)) == -1
    assert "exclude each other" in L.ss_last_error().decode()
    pr = host.SpartanProver.from_bytes(ctx, pkb, trust_digest=True, timed=True)  # the context still serves a good key
    assert pr.vk_digest.tobytes() == dig
    pr.close()


@pytest.mark.parametrize("which", CIRCUITS + ["sha256_64B"])
def test_host_and_device_forms_give_equal_keys(ctx, which):
    inst, osp, vk, dig = oracle(which)
    blob = vk[shape_offset(vk):]
    dev, hst = hip.Shape.from_wire(ctx, blob, full_device=True), hip.Shape.from_wire(ctx, blob, full=True)
    assert dev.compare(hst) == "" and dev.info() == hst.info()
    a, b = host.SpartanProver.from_bytes(ctx, vk + dig, full_device=True), host.SpartanProver.from_bytes(ctx, vk + dig, full_device=False)
    assert a.shape_info == b.shape_info and a.dims == b.dims and a.vk_digest.tobytes() == b.vk_digest.tobytes() == dig
    if which == "sha256_64B":  # the mid-size key proves
        prep, tape = ol.make_tape(77, 4096), ol.make_tape(78, 8192)
        a.prep_prove(prep, inst.witness, inst.publics)
        b.prep_prove(prep, inst.witness, inst.publics)
        wa, _, _ = a.prove(tape)
        wb, _, _ = b.prove(tape)
        assert (wa == wb).all() and a.verify(wa) == 0
    a.close()
    b.close()
