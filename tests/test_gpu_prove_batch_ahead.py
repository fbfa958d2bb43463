"""GPU parity: SpartanSNARK.prove_batch with the openings begun ahead (opening_ahead=True: sp_hyrax_prove_batch_begin once comm_W is complete,
sp_hyrax_prove_batch_rows from the inner sum-check's hook, sp_hyrax_prove_batch_finish in the batched call's place) and behind (opening_ahead=False).
Either way proof k is WORD FOR WORD OracleSpartan.prove's on tape k, uses as many tape blocks, and is accepted by the product's verifier and by
tests/pyverify.py; the states stay usable. Shapes: the two synthetic ones of test_gpu_prove_batch.py and one SHA-256 block (any message below 56 bytes:
the smallest circuit of the SHA-256 generator; on the 2048-wide key its witness has several rows, so the batched walk runs with a row stage - the
launch counts of test_per_proof_opening_wins_over_ahead pin that)."""
import numpy as np
import pytest

import oracle_lib as ol
import pyverify
from spartan2_amd import frontend, hip, host
from test_gpu_prove_batch import SYNTHETIC, oracles_prepped

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens():
    return host.from_label(b"ck", 2049), host.from_label(b"ck_s", 2)


def check_batch(gsp, osps, insts, tapes, gens, python_verifier=True, **kw):
    got, _ = gsp.prove_batch(tapes, **kw)
    (g, g_s) = gens
    for k, (words, used) in enumerate(got):
        want, want_used, _ = osps[k].prove(tapes[k])
        assert used == want_used, (kw, k)
        assert len(words) == len(want) and (words == want).all(), f"{kw}: proof {k} differs from the oracle's"
        assert gsp.verify(words) == 0
        if python_verifier:
            data = gsp.proof_to_bytes(words)
            assert pyverify.verify_bytes(insts[k], g[:2048], g[2048], g_s[0], g_s[1], data, vk_digest=gsp.vk_digest.tobytes()) == [int(v) for v in insts[k].publics]


@pytest.fixture(scope="module", params=sorted(SYNTHETIC))
def synthetic(request):
    insts = [frontend.synthetic_circuit(witness_seed=1000 * k, **SYNTHETIC[request.param]) for k in range(5)]
    return (insts,) + oracles_prepped(insts, 2900)


@pytest.mark.parametrize("K", [2, 3, 5])
def test_synthetic_ahead_and_behind_equal_the_oracle_and_states_stay_usable(ctx, gens, synthetic, K):
    insts, osps, prep_tapes, prep_used = (x[:K] for x in synthetic)
    gsp = host.SpartanSNARK(ctx, insts[0])
    assert gsp.prep_prove_batch(prep_tapes, witnesses=insts) == prep_used
    tapes = lambda s: [ol.make_tape(s + 7 * K + k, 4096) for k in range(K)]
    check_batch(gsp, osps, insts, tapes(3050), gens, opening_ahead=True)
    check_batch(gsp, osps, insts, tapes(3050), gens, python_verifier=False, opening_ahead=False)
    check_batch(gsp, osps, insts, tapes(3150), gens, python_verifier=False, opening_ahead=True)  # a second ahead batch
    j = K - 1
    gsp.ps, gsp.publics = gsp.batch[j]
    tape = ol.make_tape(3250 + K, 4096)
    words, used, _ = gsp.prove(tape)  # a lone prove on one state
    want, want_used, _ = osps[j].prove(tape)
    assert used == want_used and (words == want).all()
    check_batch(gsp, osps, insts, tapes(3350), gens, python_verifier=False, opening_ahead=True)  # and a batch after that
    gsp.close()


@pytest.fixture(scope="module")
def sha(ctx):
    K = 4
    msgs = [bytes((37 * i + 11 * k + 5) % 256 for i in range(3)) for k in range(K)]
    insts = [frontend.sha256_circuit(m) for m in msgs]
    osps, prep_tapes, prep_used = oracles_prepped(insts, 2700)
    gsp = host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(3)))
    assert gsp.prep_prove_batch(prep_tapes, msgs=msgs) == prep_used
    yield gsp, osps, insts
    gsp.close()


def test_sha256_batch_of_four_with_a_row_stage(ctx, gens, sha):
    gsp, osps, insts = sha
    tapes = [ol.make_tape(2800 + k, 8192) for k in range(4)]
    check_batch(gsp, osps, insts, tapes, gens, opening_ahead=True)
    check_batch(gsp, osps, insts, tapes, gens, python_verifier=False, opening_ahead=False)
    check_batch(gsp, osps, insts, [ol.make_tape(2850 + k, 8192) for k in range(4)], gens, python_verifier=False, opening_ahead=True)
    gsp.ps, gsp.publics = gsp.batch[1]
    tape = ol.make_tape(2870, 8192)
    words, used, _ = gsp.prove(tape)
    want, want_used, _ = osps[1].prove(tape)
    assert used == want_used and (words == want).all()
    check_batch(gsp, osps, insts, [ol.make_tape(2880 + k, 8192) for k in range(4)], gens, python_verifier=False, opening_ahead=True)


def test_per_proof_opening_wins_over_ahead(ctx, gens, sha):
    """with both flags the openings are K sp_hyrax_prove calls: no launch of the batched opening's kernels is recorded, and the proofs are the oracle's"""
    gsp, osps, insts = sha
    tapes = [ol.make_tape(2900 + k, 8192) for k in range(4)]
    ctx.reset_stats(True)
    try:
        check_batch(gsp, osps, insts, tapes, gens, python_verifier=False, opening_ahead=True, per_proof_opening=True)
        launches = lambda what: ctx.kernel_stats(what)[1]
        ahead_only, both = ("opening_batch_dvec", "opening_batch_ip"), ("opening_batch_rowmat", "opening_batch_walk", "opening_batch_z")
        assert [launches(w) for w in ahead_only + both + ("opening_batch_mask",)] == [0] * 6
        check_batch(gsp, osps, insts, tapes, gens, python_verifier=False, opening_ahead=True)
        assert [launches(w) for w in ahead_only] == [1, 1] and launches("opening_batch_mask") == 0
        assert [launches(w) for w in both] == [1, 2, 1]  # the walk: the delta vectors, then the comm_LZ vectors
    finally:
        ctx.reset_stats(False)


def test_a_failed_batch_leaks_no_job(ctx, gens):
    """the first state's witness does not satisfy the circuit: whatever the batch does with it (the reference proves without checking: the proof does
    not verify; an error exit is allowed too), no job stays open on the context - the next ahead batch on it proves right"""
    kw = SYNTHETIC["5x7"]
    insts = [frontend.synthetic_circuit(witness_seed=1000 * k, **kw) for k in range(2)]
    osps, prep_tapes, prep_used = oracles_prepped(insts, 2600)
    bad = frontend.synthetic_circuit(witness_seed=0, **kw)
    bad.witness = np.array(bad.witness, copy=True)
    bad.witness[0] ^= np.uint64(1)
    gsp = host.SpartanSNARK(ctx, insts[0])
    gsp.prep_prove_batch(prep_tapes, witnesses=[bad, insts[1]])
    tapes = [ol.make_tape(2610 + k, 4096) for k in range(2)]
    try:
        got, _ = gsp.prove_batch(tapes, opening_ahead=True)
        assert gsp.verify(got[0][0]) != 0
    except RuntimeError:
        pass
    gsp.close()
    gsp = host.SpartanSNARK(ctx, insts[0])
    assert gsp.prep_prove_batch(prep_tapes, witnesses=insts) == prep_used
    check_batch(gsp, osps, insts, tapes, gens, python_verifier=False, opening_ahead=True)
    # and a tape too short for the opening's blocks: the opening is not begun ahead, the error is the one prove reports, and nothing stays open
    short = [t[:8] for t in tapes]
    with pytest.raises(RuntimeError, match="tape"):
        gsp.prove_batch(short, opening_ahead=True)
    check_batch(gsp, osps, insts, tapes, gens, python_verifier=False, opening_ahead=True)
    gsp.close()
