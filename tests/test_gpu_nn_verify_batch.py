"""GPU: NeutronNovaZkSNARK.verify_batch against verify(), proof for proof. The contract is codes[k] == verify(proof k) for every k and every input - the
first failed check in verify()'s order - and, for every code but 1, == the oracle's verifier (oracle/neutronnova_zk.hpp) as well. Three small keys:
synthetic_circuit(8) x 2 steps, synthetic_circuit(30) x 5 steps (np = 8: the padding clones instance 0) and the (2, 30, 2) step / core pair whose
precommitted | rest rows differ. Each key is prepared once and proved K + 1 times on successive tape slices (every prove rerandomises: distinct valid
proofs). The shared form is forced by flag in these tests, so they hold wherever the default threshold between the forms lies.

Tampered proofs: positions are searched on the CPU with the oracle's verifier among the proof's scalar sections (the challenges of the verifier-circuit
instance, the relaxed Spartan proof at the end, the opening argument's z_vec), one low-bit flip for each code a flip can reach: 2, 4 and 6. Code 1 comes
from a truncated proof, a non-canonical limb and an off-curve coordinate. Code 5 (the public values of the verifier circuit) is not reachable by
tampering: the public values are bound into the fold challenge of NovaNIFS::verify, so a changed value fails the relaxed Spartan proof (check 4) first;
nothing here hunts for it."""
import numpy as np
import pytest

import oracle_lib as ol
from spartan2_amd import frontend, hip, host

pytestmark = pytest.mark.gpu
KC = hip.matrix_evals_chunk()
SIZES = (2, 3, KC + 1)
NPROOFS = KC + 2
KEYS = {"8x2": (2, 8, 8), "30x5": (5, 30, 30), "30x2_core2": (2, 30, 2)}  # steps, groups, core groups
CW = 2048  # DEFAULT_COMMITMENT_WIDTH
SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def scalar_sections(info, nwords):
    """word ranges of three all-scalar sections of a proof, from the end of the layout (host/proof_layout.hpp NNLayout::walk): the challenges of the
    verifier-circuit instance, the relaxed Spartan proof's tail, z_vec; and the word of delta's x coordinate"""
    nb, nx, ny = info["nb"], info["nx"], info["ny"]
    num_chal = nb + nx + 1 + ny
    vio = num_chal + info["vc_public"]
    vcons_rows, vrows_all = info["vc_cons"] // 32, info["vc_vars"] // 32
    vlx = (info["vc_cons"] - 1).bit_length()
    vly = (1 << (info["vc_vars"] - 1).bit_length()).bit_length() - 1 + 1
    tail = 1 + 32 + 1 + 32 + 2 * vly + 3 + 3 * vlx + vio + 1  # blind_vE, v_E, blind_vW, v_W, v_inner, v_claims, v_outer, rnd_X, rnd_u
    total = nwords // 4
    chal_hi = total - tail - 2 * (2 * vcons_rows + vrows_all)  # rnd_comm_E, rnd_comm_W, comm_T
    chal_lo = chal_hi - num_chal
    zvec_hi = chal_lo - info["vc_public"] - 2 * vrows_all - 2  # vpub, the rounds' rows, z_beta, z_delta
    zvec_lo = zvec_hi - CW
    return {2: (4 * chal_lo, 4 * chal_hi), 4: (4 * (total - tail), 4 * total), 6: (4 * zvec_lo, 4 * zvec_hi)}, 4 * (zvec_lo - 4)


@pytest.fixture(scope="module", params=sorted(KEYS))
def key(ctx, request):
    n, groups, core_groups = KEYS[request.param]
    steps = [frontend.synthetic_circuit(groups, 0xA5, num_public=1, witness_seed=50 + i) for i in range(n)]
    core = frontend.synthetic_circuit(core_groups, 0xA5 + (core_groups > groups), num_public=1, witness_seed=7)
    onn = ol.OracleNeutronNova(steps, core)
    gnn = host.NeutronNovaZkSNARK(ctx, steps, core)
    tape = ol.make_tape(300 + n, 65536)
    pos = gnn.prep_prove(tape)
    proofs = []
    for _ in range(NPROOFS):
        words, used, _ = gnn.prove(tape[pos:])
        pos += used
        proofs.append(words)
    assert all(not (proofs[0] == p).all() for p in proofs[1:])
    # one tampered proof per reachable code, found on the CPU
    sections, delta_x = scalar_sections(gnn.info, len(proofs[0]))
    bad = {}
    for code, (lo, hi) in sections.items():
        for p in range(lo, min(hi, lo + 64), 4):  # the low limb of the section's first scalars
            cand = proofs[0].copy()
            cand[p] ^= np.uint64(1)
            if onn.verify_words(cand) == code:
                bad[code] = cand
                break
        assert code in bad, f"no flip in words [{lo}, {hi}) makes the oracle answer {code}"
    truncated = proofs[0][:-4].copy()
    noncanonical = proofs[0].copy()
    noncanonical[-4:] = np.uint64(0xFFFFFFFFFFFFFFFF)  # blind_vE >= the modulus
    offcurve = proofs[0].copy()
    offcurve[delta_x] ^= np.uint64(1)
    k = {"onn": onn, "gnn": gnn, "proofs": proofs, "bad": bad, "malformed": [truncated, noncanonical, offcurve]}
    yield k
    gnn.close()


def expect(key, batch):
    """verify() of every proof; where that is not 1, the oracle agrees"""
    want = [key["gnn"].verify(p) for p in batch]
    for p, c in zip(batch, want):
        if c != 1:
            assert key["onn"].verify_words(p) == c
    return want


def mixed(key, size, bads):
    """`size` proofs with the tampered ones at the first, a middle and the last place, valid ones between them"""
    batch = [key["proofs"][1 + (i % (NPROOFS - 1))] for i in range(size)]
    for place, b in zip((0, size // 2, size - 1), bads):
        batch[place] = b
    return batch


@pytest.mark.parametrize("size", SIZES)
def test_all_valid(key, size):
    gnn = key["gnn"]
    batch = key["proofs"][:size]
    codes, info = gnn.verify_batch(batch, info=True, per_proof=False)
    assert codes == [0] * size
    assert info == {"matrix_chunks": 2 * ((size + KC - 1) // KC), "opening_batched_ok": 1, "fallback_proofs": 0, "opening_proofs": size}
    assert gnn.verify_batch(batch) == [0] * size  # the form the driver picks by itself


def test_tampered_among_valid(key):
    gnn, bad = key["gnn"], key["bad"]
    size = KC + 1
    for bads in ([bad[2], bad[4], bad[6]], key["malformed"], [bad[6], key["malformed"][2], bad[2]]):
        batch = mixed(key, size, bads)
        want = expect(key, batch)
        assert sum(1 for c in want if c == 0) == size - 3
        codes, info = gnn.verify_batch(batch, info=True, per_proof=False)
        assert codes == want
        assert info["opening_proofs"] == size - 3 + want.count(6)
    assert [gnn.verify(bad[c]) for c in (2, 4, 6)] == [2, 4, 6]
    assert [gnn.verify(p) for p in key["malformed"]] == [1, 1, 1]
    # a batch of 3 with two tampered proofs at its ends, and one that is all tampered
    for batch in ([bad[4], key["proofs"][2], bad[6]], [bad[2], bad[6], bad[4]]):
        assert gnn.verify_batch(batch, per_proof=False) == expect(key, batch)


def test_only_the_opening_fails(key):
    gnn, bad = key["gnn"], key["bad"]
    batch = [key["proofs"][0], bad[6], key["proofs"][1], key["proofs"][2]]
    codes, info = gnn.verify_batch(batch, info=True, per_proof=False)
    assert codes == [0, 6, 0, 0] == expect(key, batch)
    assert info["opening_batched_ok"] == 0 and info["opening_proofs"] == 4 and info["fallback_proofs"] == 4


def test_one_and_none(key):
    gnn, bad = key["gnn"], key["bad"]
    assert gnn.verify_batch([]) == [] and gnn.verify_bytes_batch([]) == []
    assert gnn.verify_batch([], info=True, per_proof=False) == ([], {"matrix_chunks": 0, "opening_batched_ok": 1, "fallback_proofs": 0, "opening_proofs": 0})
    for per_proof in (None, False, True):
        assert gnn.verify_batch([key["proofs"][0]], per_proof=per_proof) == [0]
        assert gnn.verify_batch([bad[6]], per_proof=per_proof) == [6]
        assert gnn.verify_batch([key["malformed"][0]], per_proof=per_proof) == [1]


def test_seed_and_forced_forms(key):
    gnn, bad = key["gnn"], key["bad"]
    batch = mixed(key, KC + 1, [bad[4], bad[6], key["malformed"][1]])
    want = expect(key, batch)
    assert gnn.verify_batch(batch, seed=SEED_A, per_proof=False) == want
    assert gnn.verify_batch(batch, seed=SEED_B, per_proof=False) == want
    codes, info = gnn.verify_batch(batch, info=True, per_proof=True)
    assert codes == want and info == {"matrix_chunks": 0, "opening_batched_ok": 1, "fallback_proofs": 0, "opening_proofs": 0}
    assert gnn.verify_batch(batch) == want


def test_bytes(key):
    gnn, bad = key["gnn"], key["bad"]
    good = [gnn.proof_to_bytes(p) for p in key["proofs"][:3]]
    b6 = gnn.proof_to_bytes(bad[6])
    b2 = gnn.proof_to_bytes(bad[2])
    nc = bytearray(good[0])
    nc[-32:] = bytes([0xFF]) * 32
    blobs = [good[0][:-1], good[1], b6, good[2] + b"\0", b2, b"", bytes(nc), good[0]]
    want = [gnn.verify_bytes(b) for b in blobs]
    assert want == [1, 0, 6, 1, 2, 1, 1, 0]
    for per_proof in (False, True, None):
        assert gnn.verify_bytes_batch(blobs, per_proof=per_proof) == want
    assert gnn.verify_bytes_batch(good, seed=SEED_A, info=True, per_proof=False) == ([0, 0, 0], {"matrix_chunks": 2, "opening_batched_ok": 1, "fallback_proofs": 0, "opening_proofs": 3})


def test_verify_is_undisturbed_by_a_batch(key):
    """the key holds the single form's tables and the batch's chunk tables side by side: each form answers as before after the other has run"""
    gnn, bad = key["gnn"], key["bad"]
    singles = [key["proofs"][0], bad[4], bad[6], key["proofs"][3]]
    before = [gnn.verify(p) for p in singles]
    assert before == [0, 4, 6, 0]
    batch = key["proofs"][: KC + 1]
    assert gnn.verify_batch(batch, per_proof=False) == [0] * (KC + 1)
    assert [gnn.verify(p) for p in singles] == before
    assert gnn.verify_batch(batch, per_proof=False) == [0] * (KC + 1)
