"""GPU: NeutronNovaZkSNARK.prove_batch against the oracle and against prove(), proof for proof. The contract is that proof k of a batch over the states
of prep_prove_batch is the proof prove(tape_k, state=k) makes - the oracle's words for witnesses k and tape k, the same tape blocks used - whichever form
runs: the driver's default, a loop of prove (per_proof=True) or the outer and inner batched sum-checks of all proofs in lockstep (per_proof=False).
Keys: the small synthetic ones of test_gpu_nn_prep_prove_batch.py - (2 steps, 8 groups), (5, 30) padded to 8, (2, 30, core 2), the shared witness, the
rest-variables key. Every state has its own witnesses and its own tape; the oracle's proofs are computed once per key."""
import numpy as np
import pytest

import oracle_lib as ol
from spartan2_amd import hip, host
from test_gpu_nn_prep_prove_batch import KEYS, KMAX, TAPE_BLOCKS

pytestmark = pytest.mark.gpu
NAMES = ["8x2", "30x5", "30x2_core2", "shared_30x3", "rest_only_8x3"]
FORMS = {"default": None, "per_proof": True, "lockstep": False}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=NAMES)
def key(ctx, request):
    """per state k < KMAX: its witnesses, its tape, the oracle's (blocks of prep_prove, blocks of prove, proof words); the object under test"""
    wits = [KEYS[request.param](k) for k in range(KMAX)]
    tapes = [ol.make_tape(300 + 11 * k, TAPE_BLOCKS) for k in range(KMAX)]
    want = []
    for (steps, core), tape in zip(wits, tapes):
        words, used, _ = ol.OracleNeutronNova(steps, core).prove(tape)
        want.append((used[0], used[1], words))
    assert not (want[0][2] == want[1][2]).all()
    gnn = host.NeutronNovaZkSNARK(ctx, *wits[0])
    k = dict(name=request.param, ctx=ctx, wits=wits, tapes=tapes, want=want, gnn=gnn)
    yield k
    gnn.close()


@pytest.fixture(autouse=True)
def batch_freed(request):
    yield
    if "key" in request.fixturenames:
        request.getfixturevalue("key")["gnn"]._free_batch()


def prepared(key, K):
    """K states of prep_prove_batch -> the rest of each tape"""
    used = key["gnn"].prep_prove_batch(key["tapes"][:K], witnesses=key["wits"][:K])
    assert used == [key["want"][k][0] for k in range(K)]
    return [key["tapes"][k][used[k]:] for k in range(K)]


def check_proofs(key, got):
    for k, (words, used) in enumerate(got):
        assert used == key["want"][k][1], f"proof {k}: tape blocks"
        assert (words == key["want"][k][2]).all(), f"proof {k}: the words differ from the oracle's"


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("K", [1, 2, 3])
def test_proofs_are_the_oracle_s_and_prove_s(key, K, form):
    gnn = key["gnn"]
    rest = prepared(key, K)
    got = gnn.prove_batch(rest, per_proof=FORMS[form])
    assert len(got) == K
    check_proofs(key, got)
    ph = gnn.batch_prove_phases
    assert set(ph) == set(host.NN_BATCH_PROVE_PHASES) and ph["total"] > 0
    if form != "default":
        assert ph["lockstep"] == (0.0 if FORMS[form] else 1.0)
    for k in range(K):
        one, used, _ = gnn.prove(rest[k], state=k)
        assert used == got[k][1] and (one == got[k][0]).all(), f"proof {k}: prove(tape, state={k}) differs"
        assert gnn.verify(got[k][0]) == 0


def test_every_proof_is_accepted_by_the_python_verifier(key):
    import pynnverify

    gnn = key["gnn"]
    rest = prepared(key, KMAX)
    got = gnn.prove_batch(rest, per_proof=False)
    check_proofs(key, got)
    gens = host.from_label(b"ck", 2049)
    for k, (words, _) in enumerate(got):
        steps, core = key["wits"][k]
        assert gnn.verify(words) == 0
        pubs = pynnverify.verify_bytes(steps[0], core, len(steps), gens, gnn.proof_to_bytes(words))
        assert pubs == ([[int(v) for v in s.publics] for s in steps], [int(v) for v in core.publics]), f"proof {k}"


@pytest.mark.parametrize("form", ["per_proof", "lockstep"])
def test_a_second_batch_on_the_same_states_gives_the_same_words(key, form):
    gnn = key["gnn"]
    rest = prepared(key, KMAX)
    first = gnn.prove_batch(rest, per_proof=FORMS[form])
    second = gnn.prove_batch(rest, per_proof=FORMS[form])
    check_proofs(key, first)
    check_proofs(key, second)
    part = gnn.prove_batch([rest[2], rest[0]], states=[2, 0], per_proof=FORMS[form])  # a list of states, in the caller's order
    assert (part[0][0] == first[2][0]).all() and (part[1][0] == first[0][0]).all()


@pytest.mark.parametrize("form", ["per_proof", "lockstep"])
def test_a_short_tape_names_its_proof_and_leaves_the_states_usable(key, form):
    gnn = key["gnn"]
    rest = prepared(key, KMAX)
    need = key["want"][1][1]
    for cut in (need - 1, need // 2, 1):  # at the very end, inside the verifier-circuit rounds, at the first draw
        short = [rest[0], rest[1][:cut], rest[2]]
        with pytest.raises(hip.SpartanHipError, match=r"rc=-5: prove_batch: proof 1: .*random tape exhausted"):
            gnn.prove_batch(short, per_proof=FORMS[form])
    check_proofs(key, gnn.prove_batch(rest, per_proof=FORMS[form]))


def test_refusals(key):
    gnn = key["gnn"]
    rest = prepared(key, 2)
    with pytest.raises(hip.SpartanHipError, match="prove_batch: the same state twice, proofs 0 and 1"):
        gnn.prove_batch([rest[0], rest[0]], states=[0, 0])
    with pytest.raises(hip.SpartanHipError, match="prove_batch: count must be at least 1"):
        gnn.prove_batch([], states=[])
    with pytest.raises(hip.SpartanHipError, match="state 7 of a batch of 2"):
        gnn.prove_batch([rest[0]], states=[7])
    with pytest.raises(ValueError):
        gnn.prove_batch(rest[:1])
    check_proofs(key, gnn.prove_batch(rest))


def test_the_single_state_is_undisturbed(key):
    """self.ps made before a batch proves the oracle's words after prove_batch ran on the batch's states"""
    gnn = key["gnn"]
    want_used, _, want_words = key["want"][0]
    assert gnn.prep_prove(key["tapes"][0]) == want_used
    ps = gnn.ps
    used = gnn.prep_prove_batch(key["tapes"][1:], witnesses=key["wits"][1:])
    got = gnn.prove_batch([key["tapes"][k][used[k - 1]:] for k in range(1, KMAX)], per_proof=False)
    for j, k in enumerate(range(1, KMAX)):
        assert got[j][1] == key["want"][k][1] and (got[j][0] == key["want"][k][2]).all()
    assert gnn.ps is ps
    words, _, _ = gnn.prove(key["tapes"][0][want_used:])
    assert (words == want_words).all()
