"""GPU: NeutronNova keys from their bytes. NeutronNovaZkSNARK.vk_to_bytes / pk_to_bytes write what tests/pynnkey.py writes from the integer circuits;
host.NeutronNovaVerifier / host.NeutronNovaProver load those bytes (nnz_verifier_from_bytes / nnz_prover_from_bytes: sp_shape_from_wire twice on one cursor,
the verifier circuit rebuilt and compared, the digest hashed from the serde bytes) and then verify and prove what setup's key verifies and proves: the
oracle's digest, the oracle's proof words bit for bit. Bytes that are not a key of the stated step count are refused, and a refused load leaves nothing on
the device."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as ol
import pynnkey
import pynnverify
from spartan2_amd import frontend, hip, host

pytestmark = pytest.mark.gpu

# (steps, groups, core_groups); the last two equalize to different precommitted | rest splits (tests/test_gpu_neutronnova_zk.py)
CASES = [(2, 8, 8), (5, 30, 30), (3, 2, 30), (3, 8, 2)]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def gens():
    return host.from_label(b"ck", 2049)


def circuits(n, groups, core_groups):
    steps = [frontend.synthetic_circuit(groups, 0xA5, num_public=1, witness_seed=50 + i) for i in range(n)]
    return steps, frontend.synthetic_circuit(core_groups, 0xA5 + (core_groups > groups), num_public=1, witness_seed=7)


class Case:
    """the circuits of one case, the oracle's proof of them on one tape, and the key bytes as pynnkey writes them - computed once, read by every test"""

    def __init__(self, n, groups, core_groups):
        self.n = n
        self.steps, self.core = circuits(n, groups, core_groups)
        self.onn = ol.OracleNeutronNova(self.steps, self.core)
        self.tape = ol.make_tape(300 + n + groups, 32768)
        self.want, self.used, _ = self.onn.prove(self.tape)
        self.digest = self.onn.digest().tobytes()
        self.vk_fields = pynnkey.vk_fields(self.steps[0], self.core, n, gens())
        self.pk_fields = pynnkey.pk_fields(self.steps[0], self.core, n, gens())
        self.vk = b"".join(b for _, b in self.vk_fields)
        self.pk = b"".join(b for _, b in self.pk_fields)
        self.voff, self.poff = pynnkey.offsets(self.vk_fields), pynnkey.offsets(self.pk_fields)

    def words(self, steps=None, core=None):
        """the caller's words for NeutronNovaProver.prep_prove"""
        steps, core = self.steps if steps is None else steps, self.core if core is None else core
        return [s.witness for s in steps], [s.publics for s in steps], core.witness, core.publics


@functools.lru_cache(maxsize=None)
def case(n, groups, core_groups):
    return Case(n, groups, core_groups)


def free_bytes():
    import torch

    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


# ---- 1. the writers ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,groups,core_groups", CASES)
def test_key_bytes_are_pynnkeys(ctx, n, groups, core_groups):
    c = case(n, groups, core_groups)
    assert pynnkey.digest_from_bytes(c.vk) == c.digest
    gnn = host.NeutronNovaZkSNARK(ctx, c.steps, c.core)
    assert gnn.vk_to_bytes() == c.vk
    assert gnn.pk_to_bytes() == c.pk
    assert host.nn_vk_digest_from_bytes(c.vk) == host.nn_vk_digest_from_bytes(c.pk, prover=True) == gnn.vk_digest.tobytes() == c.digest
    # other circuits than the key's, and a buffer that cannot hold the bytes
    other = host.NeutronNovaZkSNARK(ctx, c.steps, c.core)
    other.core = c.steps[0] if c.core.num_cons != c.steps[0].num_cons else frontend.synthetic_circuit(groups, 0xA6, num_public=1, witness_seed=7)
    with pytest.raises(hip.SpartanHipError, match="not those this key was set up from"):
        other.vk_to_bytes()
    L = host.lib()
    a1, k1 = host._inst_args(c.steps[0])
    a2, k2 = host._inst_args(c.core)
    out = np.zeros(len(c.pk), dtype=np.uint8)
    for fn, blob in ((L.nnz_vk_to_bytes, c.vk), (L.nnz_pk_to_bytes, c.pk)):
        fn.restype = ctypes.c_long
        assert fn(gnn.pk, *a1, *a2, None, ctypes.c_size_t(0)) == len(blob)
        assert fn(gnn.pk, *a1, *a2, hip.p8(out), ctypes.c_size_t(len(blob) - 1)) < 0 and "buffer too small" in L.ss_last_error().decode()
    other.close()
    gnn.close()


def test_s_core_starts_on_both_alignments():
    """S_core starts wherever S_step ends: over the cases its first byte lies at offsets = 0 and = 8 (mod 16) of the key's bytes, in both keys - the second
    sp_shape_from_wire of a load reads arrays that the Spartan loaders' single shape never placed there"""
    for which in ("voff", "poff"):
        at = {getattr(case(*cs), which)["S_core"] % 16 for cs in CASES}
        assert at == {0, 8}, (which, at)


# ---- 2. the loaded verifier -----------------------------------------------------------------------------------------------------------------------------------
def flips(got, n):
    """the seeded single-bit flips of test_verify_rejects_what_the_oracle_rejects"""
    rng = np.random.default_rng(7 + n)
    positions = sorted(set(int(x) for x in rng.integers(0, len(got), size=60)) | {0, 5, len(got) - 1, len(got) - 5, len(got) // 2})
    for pos in positions:
        bad = got.copy()
        bad[pos] ^= np.uint64(1)
        yield pos, bad


@pytest.mark.parametrize("n,groups,core_groups", CASES)
def test_loaded_verifier_is_setups(ctx, n, groups, core_groups):
    c = case(n, groups, core_groups)
    gnn = host.NeutronNovaZkSNARK(ctx, c.steps, c.core)
    v = host.NeutronNovaVerifier.from_bytes(ctx, c.vk, n)
    assert v.vk_digest.tobytes() == gnn.vk_digest.tobytes() == c.digest and v.info == gnn.info == c.onn.info
    assert v.stages()["total"] > 0 and v.stages()["digest"] > 0
    data = c.onn.proof_to_bytes(c.want)
    assert v.verify(c.want) == 0 and v.verify_bytes(data) == 0 and v.proof_to_bytes(c.want) == data and (v.proof_from_bytes(data) == c.want).all()
    if groups == core_groups:  # the two cases of test_verify_rejects_what_the_oracle_rejects
        seen = set()
        for pos, bad in flips(c.want, n):
            rc = v.verify(bad)
            assert rc == gnn.verify(bad) != 0, pos
            seen.add(rc)
        assert {2, 4, 6} <= seen
    # verify_batch in both forms: 8 proofs, three of them bad at different depths
    proofs = [c.want.copy() for _ in range(8)]
    for k, pos in ((1, 5), (4, len(c.want) // 2), (6, len(c.want) - 1)):
        proofs[k][pos] ^= np.uint64(1)
    single = [v.verify(p) for p in proofs]
    assert [rc != 0 for rc in single] == [k in (1, 4, 6) for k in range(8)] and single == [gnn.verify(p) for p in proofs]
    for per_proof in (False, True):
        assert v.verify_batch(proofs, per_proof=per_proof) == single
        assert v.verify_bytes_batch([v.proof_to_bytes(p) for p in proofs], per_proof=per_proof) == single
    # both decode forms give the same row-only shapes, and those are the rows of setup's
    dev, hst = host.NeutronNovaVerifier.from_bytes(ctx, c.vk, n, device_decode=True), host.NeutronNovaVerifier.from_bytes(ctx, c.vk, n, device_decode=False, timed=True)
    assert dev.wire_stages["device"] == 1.0 and hst.wire_stages["device"] == 0.0
    for a, b, s in zip(host.nn_key_shapes(dev), host.nn_key_shapes(hst), host.nn_key_shapes(gnn)):
        assert a.compare(b) == "" and b.compare(a) == "" and a.dims == b.dims == s.dims
        assert a.info()["nnz"] == s.info()["nnz"] and a.compare(s).startswith("row_only")
    assert hst.verify(c.want) == 0 and dev.verify(proofs[4]) == single[4]
    # every prover entry point refuses the key by name
    L = host.lib()
    sz = ctypes.c_size_t
    sw, sp, cw, cp = gnn._words(c.steps, c.core)
    used, ps = sz(0), ctypes.c_void_p()
    words = np.zeros(len(c.want), dtype=np.uint64)
    ms = (ctypes.c_double * 10)()
    tp = hip.p8(c.tape)
    one = lambda x, t: (t * 1)(x)
    blocks = np.zeros(64 * n, dtype=np.uint8)
    gnn.prep_prove(c.tape)
    calls = {
        "nnz_prep_prove": lambda: L.nnz_prep_prove(v.pk, sz(n), hip.p64(sw), sz(sw.shape[1]), hip.p64(sp), sz(sp.shape[1]), hip.p64(cw), hip.p64(cp), 1, tp, sz(len(c.tape)),
                                                   ctypes.byref(used), ctypes.byref(ps)),
        "nnz_prep_prove_sha256": lambda: L.nnz_prep_prove_sha256(v.pk, None, hip.p8(blocks), sz(n), 1, tp, sz(len(c.tape)), ctypes.byref(used), ctypes.byref(ps)),
        "nnz_prep_prove_batch": lambda: L.nnz_prep_prove_batch_opts(v.pk, sz(1), one(n, sz), one(hip.p64(sw), hip.c_u64p), one(sw.shape[1], sz), one(hip.p64(sp), hip.c_u64p),
                                                                    sz(sp.shape[1]), one(hip.p64(cw), hip.c_u64p), one(hip.p64(cp), hip.c_u64p), 1, one(tp, hip.c_u8p),
                                                                    one(len(c.tape), sz), None, ctypes.byref(ps), None, ctypes.c_uint(0)),
        "nnz_prep_prove_sha256_batch": lambda: L.nnz_prep_prove_sha256_batch_opts(v.pk, ctypes.c_void_p(1), sz(1), one(hip.p8(blocks), hip.c_u8p), one(n, sz), 1,
                                                                                  one(tp, hip.c_u8p), one(len(c.tape), sz), None, ctypes.byref(ps), None, ctypes.c_uint(0)),
        "nnz_prove": lambda: L.nnz_prove(v.pk, gnn.ps, tp, sz(len(c.tape)), ctypes.byref(used), hip.p64(words), sz(len(words)), ms),
        "nnz_prove_reference_order": lambda: L.nnz_prove_reference_order(v.pk, gnn.ps, tp, sz(len(c.tape)), ctypes.byref(used), hip.p64(words), sz(len(words)), ms),
        "nnz_prove_batch": lambda: L.nnz_prove_batch_opts(v.pk, one(gnn.ps.value, ctypes.c_void_p), sz(1), one(tp, hip.c_u8p), one(len(c.tape), sz), None,
                                                          one(hip.p64(words), hip.c_u64p), sz(len(words)), ms, ctypes.c_uint(0)),
        "nnz_prep_is_sat": lambda: L.nnz_prep_is_sat(v.pk, gnn.ps, (hip._SatReport * (n + 1))(), None, sz(0), None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.ss_last_error().decode()
        assert msg.startswith(name + ": verifier-only key (loaded by nnz_verifier_from_bytes"), (name, msg)
    assert not ps.value and not words.any()
    assert v.verify(c.want) == 0  # ... and still verifies
    for o in (dev, hst, v, gnn):
        o.close()


# ---- 3. the loaded prover -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trust_digest", [False, True], ids=["hashed", "trusted"])
@pytest.mark.parametrize("full_device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("n,groups,core_groups", CASES)
def test_loaded_prover_proves_what_the_oracle_and_setup_prove(ctx, n, groups, core_groups, full_device, trust_digest):
    c = case(n, groups, core_groups)
    pr = host.NeutronNovaProver.from_bytes(ctx, c.pk, n, trust_digest=trust_digest, full_device=full_device)
    gnn = host.NeutronNovaZkSNARK(ctx, c.steps, c.core)
    assert pr.vk_digest.tobytes() == c.digest and pr.info == gnn.info
    assert (pr.load_stages["digest"] == 0.0) == trust_digest and pr.wire_stages["device"] == (1.0 if full_device else 0.0)
    for a, s in zip(host.nn_key_shapes(pr), host.nn_key_shapes(gnn)):
        assert a.compare(s) == "" and s.compare(a) == "" and a.dims == s.dims and a.info() == s.info()
    prep, tape = c.tape, c.tape[c.used[0]:]
    assert pr.prep_prove(prep, *c.words()) == c.used[0] == gnn.prep_prove(prep)
    assert all(r.ok for r in pr.is_sat())
    words, used, _ = pr.prove(tape)
    assert used == c.used[1] and (words == c.want).all()
    # the reference-order driver on a fresh state of the same tape
    pr.prep_prove(prep, *c.words())
    again, used, _ = pr.prove(tape, reference_order=True)
    assert used == c.used[1] and (again == c.want).all()
    data = pr.proof_to_bytes(words)
    assert pr.verify(words) == 0 and pr.verify_bytes(data) == 0 and gnn.verify(words) == 0 and c.onn.verify_words(words) == 0
    assert pr.proof_to_bytes(words) == c.onn.proof_to_bytes(c.want)
    assert pynnverify.verify_bytes(c.steps[0], c.core, n, gens(), data) == ([[int(x) for x in s.publics] for s in c.steps], [int(x) for x in c.core.publics])
    # the batch: two states on two pairs of tapes equal the per-state calls (setup's key prepares beside it; the oracle's words above are the reference of
    # the proofs, so only the loaded key proves)
    preps = [ol.make_tape(700 + k, 8192) for k in range(2)]
    tapes = [ol.make_tape(800 + k, 32768) for k in range(2)]
    prep_used = pr.prep_prove_batch(preps, witnesses=[c.words()] * 2)
    assert prep_used == gnn.prep_prove_batch(preps)
    got = pr.prove_batch(tapes)
    for k in range(2):
        assert pr.prep_prove(preps[k], *c.words()) == prep_used[k]
        want_k, want_used_k, _ = pr.prove(tapes[k])
        assert got[k][1] == want_used_k and (got[k][0] == want_k).all()
        assert gnn.verify(got[k][0]) == 0 and c.onn.verify_words(got[k][0]) == 0
    # a spoiled witness is found where setup's key finds it
    spoiled = list(c.steps)
    bad = frontend.synthetic_circuit(groups, 0xA5, num_public=1, witness_seed=50 + n - 1)
    bad.witness = np.array(bad.witness, dtype=np.uint64).copy()
    bad.witness[len(bad.witness) // 3] ^= np.uint64(1)
    spoiled[n - 1] = bad
    pr.prep_prove(prep, *c.words(steps=spoiled))
    gnn.prep_prove(prep, _steps=spoiled)
    reps, want_reps = pr.is_sat(), gnn.is_sat()
    assert [r.ok for r in reps] == [True] * (n - 1) + [False, True]
    assert reps[n - 1].num_failing == want_reps[n - 1].num_failing > 0 and reps[n - 1].first_failing == want_reps[n - 1].first_failing
    assert reps[n - 1].reason == hip.REASON_UNSAT
    pr.close()
    gnn.close()


def test_one_key_proves_three_and_four_steps(ctx):
    """a key set up with 3 steps, loaded with num_steps = 4: the oracle's 4-step proof, accepted by a verifier loaded from the 3-step verifier key"""
    steps, core = circuits(4, 8, 2)
    g3 = host.NeutronNovaZkSNARK(ctx, steps[:3], core)
    pkb, vkb = g3.pk_to_bytes(), g3.vk_to_bytes()
    g3.close()
    assert pkb == pynnkey.pk_bytes(steps[0], core, 4, gens())
    onn = ol.OracleNeutronNova(steps, core)
    tape = ol.make_tape(44, 32768)
    want, used, _ = onn.prove(tape)
    pr = host.NeutronNovaProver.from_bytes(ctx, pkb, 4)
    v = host.NeutronNovaVerifier.from_bytes(ctx, vkb, 4)
    assert pr.vk_digest.tobytes() == onn.digest().tobytes() == v.vk_digest.tobytes()
    assert pr.prep_prove(tape, [s.witness for s in steps], [s.publics for s in steps], core.witness, core.publics) == used[0]
    words, used1, _ = pr.prove(tape[used[0]:])
    assert used1 == used[1] and (words == want).all() and v.verify(words) == 0 and onn.verify_words(words) == 0
    with pytest.raises(hip.SpartanHipError, match="InvalidWitnessLength"):  # the key loaded for 4 steps takes 4
        pr.prep_prove(tape, [s.witness for s in steps[:3]], [s.publics for s in steps[:3]], core.witness, core.publics)
    v3 = host.NeutronNovaVerifier.from_bytes(ctx, vkb, 3)
    assert v3.verify(words) != 0  # a 4-step proof is no 3-step proof
    for o in (pr, v, v3):
        o.close()


def test_loaded_prover_generates_sha256_witnesses(ctx):
    """prep_prove_sha256 and prep_prove_batch(blocks=) on a loaded key: key bytes, message blocks and a tape in, a proof out; a verifier that has only the
    verifier key's bytes accepts it"""
    blocks = [bytes([i + 1]) * 64 for i in range(2)]
    steps = [frontend.sha256_step_circuit(b) for b in blocks]
    core = frontend.sha256_step_circuit(bytes(64))
    gnn = host.NeutronNovaZkSNARK(ctx, steps, core)
    pkb, vkb = gnn.pk_to_bytes(), gnn.vk_to_bytes()
    assert pkb == pynnkey.pk_bytes(steps[0], core, 2, gens()) and vkb == pynnkey.vk_bytes(steps[0], core, 2, gens())
    pr = host.NeutronNovaProver.from_bytes(ctx, pkb, 2)
    v = host.NeutronNovaVerifier.from_bytes(ctx, vkb, 2)
    tape = ol.make_tape(901, 32768)
    want, want_used, _ = ol.OracleNeutronNova(steps, core).prove(tape)
    used0 = pr.prep_prove_sha256(blocks, tape)
    assert used0 == gnn.prep_prove_sha256(blocks, tape) == want_used[0]
    words, used1, _ = pr.prove(tape[used0:])
    assert used1 == want_used[1] and (words == want).all() and v.verify(words) == 0
    preps = [ol.make_tape(910 + k, 8192) for k in range(2)]
    tapes = [ol.make_tape(920 + k, 32768) for k in range(2)]
    assert pr.prep_prove_batch(preps, blocks=[blocks, blocks[::-1]]) == gnn.prep_prove_batch(preps, blocks=[blocks, blocks[::-1]])
    got = pr.prove_batch(tapes)
    for k, bl in enumerate((blocks, blocks[::-1])):
        pr.prep_prove_sha256(bl, preps[k])
        want_k, used_k, _ = pr.prove(tapes[k])
        assert got[k][1] == used_k and (got[k][0] == want_k).all() and v.verify(want_k) == 0
    with pytest.raises(ValueError, match="no instances of its own"):
        pr.prep_prove_batch(preps)
    for o in (pr, v, gnn):
        o.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def splice(fields, **changed):
    return b"".join(changed.get(k, b) for k, b in fields)


def test_refusals_raise_and_leak_nothing(ctx):
    c, c2 = case(3, 8, 2), case(2, 8, 8)
    V = lambda blob, steps=c.n, **kw: host.NeutronNovaVerifier.from_bytes(ctx, blob, steps, **kw)
    Pr = lambda blob, steps=c.n, **kw: host.NeutronNovaProver.from_bytes(ctx, blob, steps, **kw)
    for load, blob in ((V, c.vk), (Pr, c.pk)):  # (the allocator's pools are warm before the first reading)
        for form in ({}, {"device_decode": False} if load is V else {"full_device": False}):
            load(blob, **form).close()
    fv, fp = dict(c.vk_fields), dict(c.pk_fields)
    refused = []  # (loader, bytes, step count, options, the message's pattern)
    short = "unexpected end of input|length prefix exceeds the input|no bytes"
    for load, blob, off, names in ((V, c.vk, c.voff, pynnkey.VK_FIELDS), (Pr, c.pk, c.poff, pynnkey.PK_FIELDS)):
        for name in names:  # cut at each field boundary
            refused.append((load, blob[:off[name]], c.n, {}, short))
        for at in (off["S_step"] + 79, off["S_step"] + 300, off["S_core"] + 1000, off["end"] - 1):  # inside a shape; one byte short
            refused.append((load, blob[:at], c.n, {}, short))
        refused.append((load, blob + b"\0", c.n, {}, "trailing bytes"))
        refused.append((load, blob, 1, {}, "num_steps: at least two step circuits"))
        refused.append((load, blob, 5, {}, "vc_shape: not the verifier circuit of nb = 3"))
        flipped = bytearray(blob)
        flipped[off["vc_shape"] + 200] ^= 1
        refused.append((load, bytes(flipped), c.n, {}, "vc_shape: not the verifier circuit"))
        flipped = bytearray(blob)
        flipped[off["vc_shape_regular"] + 30] ^= 1
        refused.append((load, bytes(flipped), c.n, {}, "vc_shape_regular: not the verifier circuit"))
    refused.append((V, c2.vk, 5, {}, "vc_shape: not the verifier circuit of nb = 3"))  # the 2-step key loaded for 5 steps
    refused.append((Pr, c2.pk, 5, {}, "vc_shape: not the verifier circuit of nb = 3"))
    narrow = pynnkey.hyrax_key_bytes(gens(), 1024)
    other = bytearray(fv["ck"])
    other[16 + 64 * 7] ^= 1  # another generator: off the curve in vk_ee's place it is never parsed, the bytes differ
    refused.append((V, splice(c.vk_fields, vk_ee=bytes(other)), c.n, {}, "vk_ee is not ck"))
    other = bytearray(fv["vc_ck"])
    other[-1] ^= 1
    refused.append((V, splice(c.vk_fields, vc_vk=bytes(other)), c.n, {}, "vc_vk is not vc_ck"))
    refused.append((V, splice(c.vk_fields, ck=narrow, vk_ee=narrow), c.n, {}, "ck: num_cols is 1024, this build's is 2048"))
    refused.append((Pr, splice(c.pk_fields, ck=narrow), c.n, {}, "ck: num_cols is 1024, this build's is 2048"))
    refused.append((Pr, splice(c.pk_fields, vc_ck=pynnkey.hyrax_key_bytes(gens(), 64)), c.n, {}, "vc_ck: num_cols is 64, this build's is 32"))
    # a coefficient >= the modulus in S_core: entry 3 of matrix A; the device forms name it
    entry = 80 + 8 + 32 * 3
    big = fv["S_core"][:entry] + b"\xff" * 32 + fv["S_core"][entry + 32:]
    named = "S_core: sp_shape_from_wire: non-canonical field element at entry 3 of matrix A"
    refused.append((V, splice(c.vk_fields, S_core=big), c.n, {"device_decode": True}, named))
    refused.append((Pr, splice(c.pk_fields, S_core=big), c.n, {"full_device": True, "trust_digest": True}, named))
    refused.append((V, splice(c.vk_fields, S_core=big), c.n, {"device_decode": False}, "S_core: wire: non-canonical field element"))
    refused.append((Pr, splice(c.pk_fields, S_core=big), c.n, {"full_device": False}, "S_core: wire: non-canonical field element"))
    # S_core as SplitR1CSShape::new leaves it, without equalize
    alone = pynnkey.shape_bytes(pynnkey.pywire.pad_shape(c.core))
    assert alone != fv["S_core"]
    refused.append((V, splice(c.vk_fields, S_core=alone), c.n, {}, r"S_core: num_cons is \d+, S_step's is \d+ \(the shapes are not equalized\)"))
    refused.append((Pr, splice(c.pk_fields, S_core=alone), c.n, {"trust_digest": True}, r"S_core: num_cons is \d+, S_step's is \d+ \(the shapes are not equalized\)"))
    # the stored digest
    flipped = bytearray(c.pk)
    flipped[c.poff["vk_digest"] + 31] ^= 1
    refused.append((Pr, bytes(flipped), c.n, {}, "vk_digest: the stored digest is not the digest of the key's bytes"))
    flipped_key = bytearray(c.pk)
    flipped_key[c.poff["ck"] + 16] ^= 1  # a byte of the key itself: the stored digest no longer matches (or the point has left the curve)
    refused.append((Pr, bytes(flipped_key), c.n, {}, "vk_digest|not on the curve|non-canonical"))
    before = free_bytes()
    for load, blob, steps, opts, pattern in refused:
        with pytest.raises(hip.SpartanHipError, match=pattern):
            load(blob if blob else b"", steps, **opts)
    assert free_bytes() == before
    # the context still serves good keys; a key under a wrong digest that was trusted proves, and the verifier with the right key rejects its proofs
    pr = Pr(bytes(flipped), trust_digest=True)
    assert pr.vk_digest.tobytes() == bytes(flipped[c.poff["vk_digest"]:c.poff["vk_digest"] + 32]) != c.digest
    assert pr.prep_prove(c.tape, *c.words()) == c.used[0]
    words, _, _ = pr.prove(c.tape[c.used[0]:])
    v = V(c.vk)
    assert pr.verify(words) == 0 and v.verify(words) != 0 and c.onn.verify_words(words) != 0 and v.verify(c.want) == 0
    # a loaded key keeps no circuit to write itself from: the caller holds the bytes
    L = host.lib()
    a1, k1 = host._inst_args(c.steps[0])
    a2, k2 = host._inst_args(c.core)
    out = np.zeros(len(c.vk), dtype=np.uint8)
    for key in (pr, v):
        for fn in (L.nnz_vk_to_bytes, L.nnz_pk_to_bytes):
            fn.restype = ctypes.c_long
            assert fn(key.pk, *a1, *a2, None, ctypes.c_size_t(0)) < 0 and "keep those" in L.ss_last_error().decode()  # the sizing pass already
            assert fn(key.pk, *a1, *a2, hip.p8(out), ctypes.c_size_t(len(out))) < 0 and "keep those" in L.ss_last_error().decode()
    assert not hasattr(pr, "vk_to_bytes") and not hasattr(v, "pk_to_bytes")
    pr.close()
    v.close()
