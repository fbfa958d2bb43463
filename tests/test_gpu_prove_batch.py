"""GPU parity: SpartanSNARK.prove_batch - K proofs of one key, the outer and the inner sum-check of all of them in lockstep. Proof k must be WORD FOR WORD
the proof the CPU oracle (and prove) makes of witness k with tape k, consume the same tape blocks, and be accepted by the product's verifier and by the
independent Python-integer verifier (tests/pyverify.py). The states must stay usable: a second batch and a lone prove equal the oracle too."""
import numpy as np
import pytest

import oracle_lib as ol
import pyverify
from challenge_circuit import ChallengeCircuit
from spartan2_amd import frontend, hip, host

pytestmark = pytest.mark.gpu

SYNTHETIC = {"5x7": dict(n_groups=5, seed=7, num_public=2), "40xDEADBEEF": dict(n_groups=40, seed=0xDEADBEEF, num_public=5)}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens():
    return host.from_label(b"ck", 2049), host.from_label(b"ck_s", 2)


def same_shape(a, b):
    return (a.num_cons, a.num_shared, a.num_precommitted, a.num_rest, a.num_public) == (b.num_cons, b.num_shared, b.num_precommitted, b.num_rest, b.num_public) and all(
        (x == y).all() for ma, mb in zip(a.csr, b.csr) for x, y in zip(ma, mb))


def oracles_prepped(insts, seed):
    """one oracle per instance, prepared on its own tape -> (oracles, prep tapes, blocks used)"""
    osps, tapes, used = [], [], []
    for k, inst in enumerate(insts):
        osp = ol.OracleSpartan(inst)
        tape = ol.make_tape(seed + k, 1024)
        used.append(osp.prep_prove(tape))
        osps.append(osp)
        tapes.append(tape)
    return osps, tapes, used


def check_batch(gsp, osps, insts, tapes, gens, python_verifier=True):
    """prove_batch(tapes) == the oracle's proofs on the same tapes, equal `used`, accepted by both verifiers"""
    got, phases = gsp.prove_batch(tapes)
    assert len(got) == len(osps) and phases["total"] > 0
    (g, g_s) = gens
    for k, (words, used) in enumerate(got):
        want, want_used, _ = osps[k].prove(tapes[k])
        assert used == want_used, k
        assert len(words) == len(want) and (words == want).all(), f"proof {k} differs from the oracle's"
        assert gsp.verify(words) == 0
        if python_verifier:
            data = gsp.proof_to_bytes(words)
            assert pyverify.verify_bytes(insts[k], g[:2048], g[2048], g_s[0], g_s[1], data, vk_digest=gsp.vk_digest.tobytes()) == [int(v) for v in insts[k].publics]
    return got


@pytest.fixture(scope="module", params=sorted(SYNTHETIC))
def synthetic(request):
    """five witnesses of one synthetic shape, their oracles prepared once and shared by the K cases (an oracle state serves any number of proves)"""
    kw = SYNTHETIC[request.param]
    insts = [frontend.synthetic_circuit(witness_seed=1000 * k, **kw) for k in range(5)]
    for inst in insts[1:]:
        assert same_shape(insts[0], inst), "the witness seeds must give one shape"
        assert not (inst.witness == insts[0].witness).all()
    return (insts,) + oracles_prepped(insts, 900)


@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_synthetic_batch_equals_oracle_and_states_stay_usable(ctx, gens, synthetic, K):
    insts, osps, prep_tapes, prep_used = (x[:K] for x in synthetic)
    gsp = host.SpartanSNARK(ctx, insts[0])
    assert gsp.prep_prove_batch(prep_tapes, witnesses=insts) == prep_used
    assert gsp.ps is None and len(gsp.batch) == K
    check_batch(gsp, osps, insts, [ol.make_tape(50 + 7 * K + k, 4096) for k in range(K)], gens)
    # again, with fresh tapes
    check_batch(gsp, osps, insts, [ol.make_tape(150 + 7 * K + k, 4096) for k in range(K)], gens, python_verifier=False)
    # and a lone prove on one of the states
    j = K - 1
    gsp.ps, gsp.publics = gsp.batch[j]
    tape = ol.make_tape(250 + K, 4096)
    words, used, _ = gsp.prove(tape)
    want, want_used, _ = osps[j].prove(tape)
    assert used == want_used and (words == want).all()
    # ... after which the batch still proves
    if K > 1:
        check_batch(gsp, osps, insts, [ol.make_tape(350 + 7 * K + k, 4096) for k in range(K)], gens, python_verifier=False)
    gsp.close()
    assert gsp.batch == [] and gsp.ps is None


@pytest.mark.parametrize("n", [3, 150], ids=["3B", "150B"])
def test_sha256_batch_of_three_messages(ctx, gens, n):
    """one key, three messages through prep_prove_batch(msgs=...): the witnesses come from the device kernel, the publics (digest bits) differ per proof"""
    K = 3
    msgs = [bytes((37 * i + 11 * k + n) % 256 for i in range(n)) for k in range(K)]
    insts = [frontend.sha256_circuit(m) for m in msgs]
    osps, prep_tapes, prep_used = oracles_prepped(insts, 700 + n)
    gsp = host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(n)))
    assert gsp.prep_prove_batch(prep_tapes, msgs=msgs) == prep_used
    for k in range(K):
        assert (gsp.batch[k][1] == insts[k].publics).all()
    assert not (gsp.batch[0][1] == gsp.batch[1][1]).all()
    check_batch(gsp, osps, insts, [ol.make_tape(800 + n + k, 8192) for k in range(K)], gens, python_verifier=True)
    check_batch(gsp, osps, insts, [ol.make_tape(850 + n + k, 8192) for k in range(K)], gens, python_verifier=False)
    gsp.ps, gsp.publics = gsp.batch[1]
    tape = ol.make_tape(870 + n, 8192)
    words, used, _ = gsp.prove(tape)
    want, want_used, _ = osps[1].prove(tape)
    assert used == want_used and (words == want).all()
    gsp.close()


def test_refusals_leave_the_states_usable(ctx, gens):
    kw = SYNTHETIC["5x7"]
    insts = [frontend.synthetic_circuit(witness_seed=1000 * k, **kw) for k in range(2)]
    osps, prep_tapes, prep_used = oracles_prepped(insts, 600)
    gsp = host.SpartanSNARK(ctx, insts[0])
    assert gsp.prep_prove_batch(prep_tapes, witnesses=insts) == prep_used
    tapes = [ol.make_tape(610 + k, 4096) for k in range(3)]
    # a state listed twice
    with pytest.raises(RuntimeError, match="same state twice"):
        gsp.prove_batch(tapes, states=[gsp.batch[0], gsp.batch[1], gsp.batch[0]])
    # states of another key
    other = host.SpartanSNARK(ctx, frontend.synthetic_circuit(witness_seed=0, **SYNTHETIC["40xDEADBEEF"]))
    other.prep_prove_batch([ol.make_tape(620, 1024), ol.make_tape(621, 1024)])
    with pytest.raises(RuntimeError, match="another key"):
        gsp.prove_batch(tapes[:2], states=[gsp.batch[0], (other.batch[1][0], gsp.batch[1][1])])
    other.close()
    check_batch(gsp, osps, insts, tapes[:2], gens, python_verifier=False)
    gsp.close()
    # a circuit with verifier challenges is proved one at a time
    cinst = ChallengeCircuit(1)
    syn = cinst.synthesize(ol.to_mont, ol.from_mont)
    csp = host.SpartanSNARK(ctx, cinst)
    cprep = [ol.make_tape(630 + k, 1024) for k in range(2)]
    cused = csp.prep_prove_batch(cprep, is_small=False)
    with pytest.raises(RuntimeError, match="verifier challenges"):
        csp.prove_batch(tapes[:2])
    cosp = ol.OracleSpartan(cinst)
    assert cosp.prep_prove(cprep[1], is_small=False) == cused[1]
    csp.ps, csp.publics = csp.batch[1]
    got = csp.prove(tapes[2], synthesize=syn)[0]
    assert (got == cosp.prove(tapes[2], synthesize=syn)[0]).all()
    csp.close()
