"""GPU checks of verify_batch: (1) sp_shape_matrix_evals_batched (k_matrix_evals_batched) against the CPU oracle's products and Python integers,
(2) SpartanSNARK.verify_batch / verify_bytes_batch against the oracle's verdict on every proof of the batch, (3) one mid-size case. Nothing expected comes
from the code under test: kernel values are orc_shape_multiply_vec + a Python dot product, verdicts are OracleSpartan.verify_words per proof."""
import hashlib

import numpy as np
import pytest

import oracle_lib as ol
from spartan2_amd import frontend, hip, host
from spartan2_amd.host import pad_shape

pytestmark = pytest.mark.gpu
P = ol.MODULI[0]
RINV = pow(ol.R, -1, P)
KC = hip.matrix_evals_chunk()  # pairs per launch (tests/test_verify_batch_cpu.py pins it to the kernel's constant)
KMAX = 2 * KC + 1


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


# ---- 1. the kernel against the oracle --------------------------------------------------------------------------------------------------------------
def raw_ints(limbs):
    """(n, 4) uint64 limbs -> Python integers, as they are (no Montgomery conversion)"""
    b = np.ascontiguousarray(limbs, dtype="<u8").tobytes()
    return [int.from_bytes(b[32 * i : 32 * i + 32], "little") for i in range(len(b) // 32)]


def raw_limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def random_residues(rng, n):
    raw = rng.bytes(32 * n)
    return [int.from_bytes(raw[32 * i : 32 * i + 32], "little") % P for i in range(n)]


def _circuit(which):
    if which == "synthetic_segments":
        return frontend.synthetic_circuit(60, 9, num_public=3, shared_permille=200, precommitted_permille=500)
    if which == "cubic":
        return frontend.cubic_circuit()
    return frontend.sha256_circuit(b"abc")


_kernel_cases = {}


def kernel_case(ctx, which):
    """shape, KMAX pairs of seeded random tables on the device and the expected (KMAX, 3) values, computed once per circuit.
    The limbs ARE the Montgomery forms: with x~ = tx limbs, y~ = ty limbs the oracle's product rows are a~ = sum_col M[row, col] y~[col] (the
    coefficient's own factor R cancels in the Montgomery product) and the kernel's sum of Montgomery products x~ a~ is (sum x~ a~) R^-1 mod p."""
    if which in _kernel_cases:
        return _kernel_cases[which]
    inst = _circuit(which)
    oshape = ol.OracleShape(inst)
    mats, dims = pad_shape(inst)
    shape = hip.Shape(ctx, mats, dims)
    N, ncols = oshape.num_cons, oshape.num_vars + oshape.num_extra
    rng = np.random.default_rng(20261017 + len(which))
    txs, tys, want = [], [], []
    for _ in range(KMAX):
        x, y = random_residues(rng, N), random_residues(rng, ncols)
        ylimbs = raw_limbs(y)
        prods = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
        assert ol.lib().orc_shape_multiply_vec(oshape.h, ol.p64(ylimbs), *(ol.p64(w) for w in prods)) == 0
        want.append([sum(xi * ai for xi, ai in zip(x, raw_ints(w))) % P * RINV % P for w in prods])
        txs.append(hip.Table.from_host(ctx, raw_limbs(x)))
        tys.append(hip.Table.from_host(ctx, ylimbs))
    case = dict(shape=shape, N=N, ncols=ncols, txs=txs, tys=tys, want=want)
    _kernel_cases[which] = case
    return case


@pytest.mark.parametrize("which", ["synthetic_segments", "sha256_1block"])
@pytest.mark.parametrize("K", [0, 1, KC, KC + 1, KMAX])
def test_matrix_evals_equal_the_oracle(ctx, which, K):
    c = kernel_case(ctx, which)
    got = c["shape"].matrix_evals_batched(c["txs"][:K], c["tys"][:K])
    assert got.shape == (K, 3, 4)
    for k in range(K):
        g = raw_ints(got[k])
        print(f"{which} K={K} k={k}: got {[hex(v)[:12] for v in g]} want {[hex(v)[:12] for v in c['want'][k]]}")
        assert g == c["want"][k], (k, g, c["want"][k])
    if K:
        assert (c["shape"].matrix_evals_batched(c["txs"][:K], c["tys"][:K]) == got).all(), "two calls with the same inputs differ"


@pytest.mark.parametrize("which", ["synthetic_segments", "sha256_1block"])
def test_matrix_evals_table_lengths(ctx, which):
    c = kernel_case(ctx, which)
    N, ncols, shape = c["N"], c["ncols"], c["shape"]
    x = np.concatenate([c["txs"][1].read(0, N), raw_limbs(random_residues(np.random.default_rng(5), 7))])
    y = np.concatenate([c["tys"][1].read(0, ncols), raw_limbs(random_residues(np.random.default_rng(6), 9))])
    tx_long, ty_long = hip.Table.from_host(ctx, x), hip.Table.from_host(ctx, y)
    got = shape.matrix_evals_batched([c["txs"][0], tx_long], [c["tys"][0], ty_long])  # longer than required: the same result
    assert [raw_ints(got[k]) for k in range(2)] == c["want"][:2]
    tx_short, ty_short = hip.Table.from_host(ctx, x[: N - 1]), hip.Table.from_host(ctx, y[: ncols - 1])
    with pytest.raises(hip.SpartanHipError, match="rc=-2"):  # SP_ERR_INVALID_WITNESS_LENGTH, as multiply_vec
        shape.matrix_evals_batched([c["txs"][0], tx_short], c["tys"][:2])
    with pytest.raises(hip.SpartanHipError, match="rc=-2"):
        shape.matrix_evals_batched(c["txs"][:2], [c["tys"][0], ty_short])
    zt = hip.Table.from_host(ctx, y[: ncols - 1])
    outs = [hip.Table.zeros(ctx, N) for _ in range(3)]
    with pytest.raises(hip.SpartanHipError, match="rc=-2"):  # ... which is what multiply_vec says to the same table
        shape.multiply_vec(zt, *outs)
    for t in [tx_long, ty_long, tx_short, ty_short, zt] + outs:
        t.free()


# ---- 2. verify_batch against the oracle's per-proof verdicts --------------------------------------------------------------------------------------
NPROOFS = 5


class Batch:
    def __init__(self, ctx, which, inst=None, nproofs=NPROOFS, msg_len=3):
        self.inst = inst if inst is not None else _circuit(which)
        self.sn = host.SpartanSNARK(ctx, self.inst)
        self.osp = ol.OracleSpartan(self.inst)
        self.proofs = []
        for i in range(nproofs):
            tape = ol.make_tape(500 + 7 * i, 8192)
            if which.startswith("sha256"):  # different messages on one key, witnesses generated on the device
                used = self.sn.prep_prove_sha256(bytes([97 + i]) + bytes(range(i, i + msg_len - 1)), tape)
            else:  # different tapes
                used = self.sn.prep_prove(tape)
            self.proofs.append(self.sn.prove(tape[used:])[0])
        self._verdicts = {}
        d = self.sn.dims
        rows = (((d["num_shared"] + 2047) // 2048) if d["num_shared_unpadded"] else 0) + (((d["num_precommitted"] + 2047) // 2048) if d["num_precommitted_unpadded"] else 0) \
            + (d["num_rest"] + 2047) // 2048
        lx = (d["num_cons"] - 1).bit_length()
        n = len(self.proofs[0])
        nz = min(2048, d["num_shared"] + d["num_precommitted"] + d["num_rest"])
        off_pub = 8 * rows
        off_outer = off_pub + 4 * d["num_public"]
        off_claims = off_outer + 12 * lx
        # the section offsets tests/test_gpu_verify.py flips a bit at
        self.sections = {"publics": off_pub if d["num_public"] else None, "outer": off_outer + 5, "claim": off_claims + 1, "inner": off_claims + 12 + 2,
                         "eval_W": n - 8 - 4 * nz - 16 - 8, "z_vec": n - 8 - 3, "z_beta": n - 1}
        self.off_z_delta = n - 8

    def oracle(self, batch):
        """[OracleSpartan.verify_words(p) for p in batch], each distinct proof verified once"""
        out = []
        for p in batch:
            key = hashlib.sha256(np.ascontiguousarray(p, dtype=np.uint64).tobytes()).digest()
            if key not in self._verdicts:
                self._verdicts[key] = self.osp.verify_words(p)
            out.append(self._verdicts[key])
        return out

    def flipped(self, k, section):
        bad = self.proofs[k].copy()
        bad[self.sections[section]] ^= np.uint64(1)
        return bad


_batches = {}


@pytest.fixture(scope="module", autouse=True)
def _close_keys():
    yield
    for b in _batches.values():
        b.sn.close()
    _batches.clear()
    _kernel_cases.clear()


@pytest.fixture(params=["cubic", "synthetic_segments", "sha256_1block"])
def batch(request, ctx):
    if request.param not in _batches:
        _batches[request.param] = Batch(ctx, request.param)
    return _batches[request.param]


def test_all_valid(batch):
    want = batch.oracle(batch.proofs)
    assert want == [0] * NPROOFS
    codes, publics, info = batch.sn.verify_batch(batch.proofs, info=True)
    print(codes, info)
    assert codes == want
    # a combined equation that never held would otherwise hide behind the fallback
    assert info["opening_batched_ok"] == 1 and info["fallback_proofs"] == 0
    assert info["matrix_chunks"] == -(-NPROOFS // KC) and info["opening_proofs"] == NPROOFS
    assert NPROOFS > KC, "the batch must cross a chunk boundary"
    npub = batch.sn.dims["num_public"]
    off = batch.sections["publics"]
    for k in range(NPROOFS):
        assert publics[k].shape == (npub, 4)
        if npub:
            assert (publics[k].reshape(-1) == batch.proofs[k][off : off + 4 * npub]).all()
    assert batch.sn.verify_batch(batch.proofs) == want


def test_one_proof_tampered(batch):
    sections = [s for s, off in batch.sections.items() if off is not None]
    seen = set()
    for i, section in enumerate(sections):
        k = [0, NPROOFS - 1, 2, 1, 3, NPROOFS - 1, 0][i % 7]  # first and last among the positions
        seen.add(k)
        b = list(batch.proofs)
        b[k] = batch.flipped(k, section)
        want = batch.oracle(b)
        got = batch.sn.verify_batch(b)
        print(section, k, want, got)
        assert want[k] != 0 and got == want, (section, k, want, got)
    assert {0, NPROOFS - 1} <= seen


def test_two_proofs_tampered_with_different_codes(batch):
    b = list(batch.proofs)
    b[1] = batch.flipped(1, "claim")
    b[3] = batch.flipped(3, "z_vec")
    want = batch.oracle(b)
    codes, _, info = batch.sn.verify_batch(b, info=True)
    print(want, codes, info)
    assert want[1] != 0 and want[3] != 0 and want[1] != want[3]
    assert codes == want
    assert info["opening_batched_ok"] == 0 and info["fallback_proofs"] == NPROOFS - 1


def test_wrong_length_proof_gets_code_1(batch):
    b = list(batch.proofs)
    b[2] = b[2][:-4]
    assert batch.sn.verify_batch(b) == [0, 0, 1, 0, 0]
    b[2] = np.zeros(0, dtype=np.uint64)
    assert batch.sn.verify_batch(b) == [0, 0, 1, 0, 0]


def test_cancelling_errors_are_both_caught(batch):
    """z_delta of one proof + 1, of another - 1: an unweighted sum of the first equation is unchanged, so constant weights would accept both"""
    b = list(batch.proofs)
    o = batch.off_z_delta
    for k, step in ((1, 1), (NPROOFS - 1, -1)):
        bad = b[k].copy()
        z = ol.from_mont(bad[o : o + 4])
        bad[o : o + 4] = ol.to_mont((z + step) % P)
        b[k] = bad
    want = batch.oracle(b)
    assert want == [0, 6, 0, 0, 6]
    codes, _, info = batch.sn.verify_batch(b, info=True)
    print(codes, info)
    assert codes == want and info["opening_batched_ok"] == 0


def test_same_valid_proof_twice(batch):
    b = [batch.proofs[0], batch.proofs[1], batch.proofs[0]]
    codes, _, info = batch.sn.verify_batch(b, info=True)
    assert codes == batch.oracle(b) == [0, 0, 0]
    assert info["opening_batched_ok"] == 1 and info["fallback_proofs"] == 0


def test_k1_equals_verify_and_k0_is_empty(batch):
    for p in (batch.proofs[0], batch.flipped(0, "z_beta"), batch.flipped(0, "inner")):
        want = batch.oracle([p])
        assert batch.sn.verify_batch([p]) == want == [batch.sn.verify(p)]
    assert batch.sn.verify_batch([]) == []
    assert batch.sn.verify_batch([], info=True) == ([], [], {"matrix_chunks": 0, "opening_batched_ok": 1, "fallback_proofs": 0, "opening_proofs": 0})
    assert batch.sn.verify_bytes_batch([]) == []


def test_bytes_batch_gives_the_same_codes(batch):
    for b in (list(batch.proofs), [batch.proofs[0], batch.flipped(1, "claim"), batch.proofs[2], batch.flipped(3, "z_vec")]):
        want = batch.oracle(b)
        blobs = [batch.sn.proof_to_bytes(p) for p in b]
        assert batch.sn.verify_bytes_batch(blobs) == want
    blobs = [batch.sn.proof_to_bytes(p) for p in batch.proofs[:3]]
    blobs[1] = blobs[1][:-1]  # bytes that do not decode: check 1, as verify_bytes
    assert batch.sn.verify_bytes_batch(blobs) == [0, 1, 0] and batch.sn.verify_bytes(blobs[1]) == 1


def test_fixed_seed_is_deterministic(batch):
    b = list(batch.proofs)
    b[NPROOFS - 1] = batch.flipped(NPROOFS - 1, "z_vec")
    seed = bytes(range(32))
    first = batch.sn.verify_batch(b, seed=seed, info=True)
    second = batch.sn.verify_batch(b, seed=seed, info=True)
    assert first[0] == second[0] == batch.oracle(b) and first[2] == second[2]
    assert batch.sn.verify_batch(batch.proofs, seed=seed) == [0] * NPROOFS
    assert batch.sn.verify_batch(batch.proofs, seed=bytes(32)) == [0] * NPROOFS  # another seed, other weights, the same verdicts


# ---- 3. one mid-size case: the matrix kernel on several blocks per matrix with real eq tables ----------------------------------------------------
def test_mid_size_batch(ctx):
    bt = Batch(ctx, "sha256_2blocks", inst=frontend.sha256_circuit(bytes(64)), nproofs=3, msg_len=64)
    assert bt.sn.dims["num_cons"] > 256, "more than one block per matrix"
    b = list(bt.proofs)
    b[1] = bt.flipped(1, "inner")
    want = bt.oracle(b)
    codes, _, info = bt.sn.verify_batch(b, info=True)
    print(want, codes, info)
    assert want[0] == 0 and want[1] != 0 and want[2] == 0
    assert codes == want and info["opening_batched_ok"] == 1 and info["fallback_proofs"] == 0
    bt.sn.close()
