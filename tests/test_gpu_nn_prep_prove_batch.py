"""GPU: NeutronNovaZkSNARK.prep_prove_batch against the oracle, state for state. The contract is that state k of a batch is the state prep_prove makes of
input k with tape k: the same tape blocks used and, proven with the rest of tape k, the proof words of OracleNeutronNova(steps_k, core_k).prove(tape_k)
(oracle/neutronnova_zk.hpp) - blinds, commitments and layers all enter those words. Keys: the three of test_gpu_nn_verify_batch.py ((2 steps, 8 groups),
(5, 30) with padding clones, (2, 30, core 2) whose step and core segments differ), a shared + precommitted key, a rest-only key and a 2-step
sha256_step_circuit key. Every state has its own witnesses and its own tape; the oracle's proofs are computed once per key. At most five prep states
are alive at once (a batch of three, one on a second object, self.ps)."""
import types

import numpy as np
import pytest

import oracle_lib as ol
from spartan2_amd import frontend, hip, host

pytestmark = pytest.mark.gpu
KMAX = 3
TAPE_BLOCKS = 4096


def _synthetic(n, groups, core_groups):
    def mk(k):
        steps = [frontend.synthetic_circuit(groups, 0xA5, num_public=1, witness_seed=50 + 10 * k + i) for i in range(n)]
        return steps, frontend.synthetic_circuit(core_groups, 0xA5 + (core_groups > groups), num_public=1, witness_seed=7 + k)
    return mk


def _shared(k):  # every circuit of a state shares step 0's shared witness (src/neutronnova_zk.rs:1485-1488): one witness seed per state
    mk = lambda: frontend.synthetic_circuit(30, 0x77, num_public=2, shared_permille=300, precommitted_permille=1000, witness_seed=5 + k)
    return [mk(), mk(), mk()], mk()


def _rest_only(k):
    mk = lambda ws: frontend.synthetic_circuit(8, 0xA5, num_public=1, precommitted_permille=0, witness_seed=ws)
    return [mk(11 + 10 * k + i) for i in range(3)], mk(99 + k)


def sha_blocks(k):
    return [bytes([16 * k + i + 1]) * 64 for i in range(2)]


def _sha(k):
    return [frontend.sha256_step_circuit(b) for b in sha_blocks(k)], frontend.sha256_step_circuit(bytes(64))


KEYS = {"8x2": _synthetic(2, 8, 8), "30x5": _synthetic(5, 30, 30), "30x2_core2": _synthetic(2, 30, 2), "shared_30x3": _shared, "rest_only_8x3": _rest_only,
        "sha256_step_x2": _sha}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=sorted(KEYS))
def key(ctx, request):
    """per state k < KMAX: its witnesses, its tape, the oracle's (tape blocks of prep_prove, proof words); the object under test"""
    wits = [KEYS[request.param](k) for k in range(KMAX)]
    tapes = [ol.make_tape(900 + 7 * k, TAPE_BLOCKS) for k in range(KMAX)]
    want = []
    for (steps, core), tape in zip(wits, tapes):
        words, used, _ = ol.OracleNeutronNova(steps, core).prove(tape)
        want.append((used[0], words))
    assert not (want[0][1] == want[1][1]).all()
    gnn = host.NeutronNovaZkSNARK(ctx, *wits[0])
    k = dict(name=request.param, ctx=ctx, wits=wits, tapes=tapes, want=want, gnn=gnn)
    yield k
    gnn.close()


@pytest.fixture(autouse=True)
def batch_freed(request):
    """every test leaves the object without a batch"""
    yield
    if "key" in request.fixturenames:
        request.getfixturevalue("key")["gnn"]._free_batch()


def check_states(key, used, states=None):
    """every state of the batch: the oracle's tape blocks and proof words, accepted, satisfied"""
    gnn = key["gnn"]
    states = range(len(used)) if states is None else states
    for k in states:
        want_used, want_words = key["want"][k]
        assert used[k] == want_used, f"state {k}"
        got, _, _ = gnn.prove(key["tapes"][k][used[k]:], state=k)
        assert (got == want_words).all(), f"state {k}: the proof differs from the oracle's"
        assert gnn.verify(got) == 0
        reps = gnn.is_sat(state=k)
        assert len(reps) == len(key["wits"][k][0]) + 1 and all(r.ok for r in reps), f"state {k}: {reps}"


@pytest.mark.parametrize("K", [1, 2, 3])
def test_states_are_the_oracle_s(key, K):
    gnn = key["gnn"]
    used = gnn.prep_prove_batch(key["tapes"][:K], witnesses=key["wits"][:K])
    assert len(gnn.batch) == K and set(gnn.batch_prep_phases) >= {"witness", "commit", "layers", "total"}
    check_states(key, used)


def test_a_fresh_prep_prove_on_a_second_object(key):
    """state 0 is made of the key's own instances: prep_prove + prove on a second object gives the words; so does the default source of a batch"""
    gnn = key["gnn"]
    want_used, want_words = key["want"][0]
    ref = host.NeutronNovaZkSNARK(key["ctx"], *key["wits"][0])
    assert ref.prep_prove(key["tapes"][0]) == want_used
    fresh, _, _ = ref.prove(key["tapes"][0][want_used:])
    ref.close()
    assert (fresh == want_words).all()
    used = gnn.prep_prove_batch([key["tapes"][0], key["tapes"][1]])  # neither witnesses nor blocks: the key's own instances, twice
    assert used == [want_used, want_used]
    got, _, _ = gnn.prove(key["tapes"][0][want_used:], state=0)
    assert (got == fresh).all()


@pytest.mark.parametrize("path", ["shared_stages", "per_state_commit", "per_state_layers", "both_flags", "loop_of_single_calls"])
def test_forced_paths_give_the_same_states(key, path):
    gnn = key["gnn"]
    kw = dict(shared_stages=dict(shared_commit=True, shared_layers=True), per_state_commit=dict(per_state_commit=True), per_state_layers=dict(per_state_layers=True), both_flags=dict(per_state_commit=True, per_state_layers=True),
              loop_of_single_calls=dict(one_pass=False))[path]
    used = gnn.prep_prove_batch(key["tapes"], witnesses=key["wits"], **kw)
    assert len(gnn.batch) == KMAX
    check_states(key, used)


@pytest.mark.parametrize("key", ["sha256_step_x2"], indirect=True)
def test_sha256_blocks_give_the_states_of_the_frontend_s_witnesses(key):
    gnn = key["gnn"]
    for kw in (dict(shared_commit=True, shared_layers=True), dict(per_state_commit=True, per_state_layers=True), dict(one_pass=False)):
        used = gnn.prep_prove_batch(key["tapes"], blocks=[sha_blocks(k) for k in range(KMAX)], **kw)
        check_states(key, used)


@pytest.mark.parametrize("key", ["8x2"], indirect=True)
def test_blocks_on_another_key_are_refused(key):
    gnn = key["gnn"]
    n = len(key["wits"][0][0])
    with pytest.raises(hip.SpartanHipError):
        gnn.prep_prove_batch(key["tapes"][:2], blocks=[[bytes(64)] * n] * 2)
    assert gnn.batch == []


def _failing_rows(inst, witness):
    """rows of the padded shape where A z o B z != C z for z = [witness | 1 | publics], from the oracle's products and Python integers"""
    oshape = ol.OracleShape(inst)
    P = ol.MODULI[0]
    W = np.zeros((oshape.num_vars, 4), dtype=np.uint64)
    w = ol.mont_array([int(x) for x in witness])
    s, p, r = oshape.num_shared_unpadded, oshape.num_precommitted_unpadded, oshape.num_rest_unpadded
    W[:s] = w[:s]
    W[oshape.num_shared : oshape.num_shared + p] = w[s : s + p]
    W[oshape.num_shared + oshape.num_precommitted : oshape.num_shared + oshape.num_precommitted + r] = w[s + p :]
    z = np.ascontiguousarray(np.concatenate([W, ol.mont_array([1] + [int(x) for x in inst.publics])]))
    out = [np.zeros((oshape.num_cons, 4), dtype=np.uint64) for _ in range(3)]
    assert ol.lib().orc_shape_multiply_vec(oshape.h, ol.p64(z), *(ol.p64(o) for o in out)) == 0
    a, b, c = (ol.ints_of(o) for o in out)
    return [i for i in range(oshape.num_cons) if (a[i] * b[i] - c[i]) % P]


def test_a_bad_state_is_named_alone(key):
    """a wrong witness word in step 1 of state 1: is_sat(state=1) names that instance and its rows, the other states are clean and still prove"""
    gnn = key["gnn"]
    steps, core = key["wits"][1]
    w = np.array(steps[1].witness, dtype=np.uint64).copy()
    at = len(w) - 3  # (not in a shared segment, which state 1 takes from its step 0)
    w[at] = np.uint64(1) - w[at] if int(w[at]) in (0, 1) else w[at] + np.uint64(1)
    want_rows = _failing_rows(steps[1], w)
    assert want_rows, "the altered word is not constrained: pick another"
    bad_step = types.SimpleNamespace(witness=w, publics=steps[1].publics)
    wits = [key["wits"][0], ([steps[0], bad_step] + list(steps[2:]), core), key["wits"][2]]
    used = gnn.prep_prove_batch(key["tapes"], witnesses=wits)
    reps = gnn.is_sat(state=1)
    for i, r in enumerate(reps):
        if i == 1:
            assert not r.ok and r.num_failing == len(want_rows) and r.first_failing == want_rows[:16] and r.bad_commitment_rows == []
        else:
            assert r.ok, f"instance {i}: {r}"
    check_states(key, used, states=(0, 2))


def test_refusals_leave_no_state_behind(key):
    gnn = key["gnn"]
    with pytest.raises(hip.SpartanHipError, match="prep_prove_batch: count must be at least 1"):
        gnn.prep_prove_batch([])
    assert gnn.batch == []
    steps, core = key["wits"][1]
    with pytest.raises(hip.SpartanHipError, match="prep_prove_batch: state 1: InvalidWitnessLength"):
        gnn.prep_prove_batch(key["tapes"], witnesses=[key["wits"][0], (steps[:-1], core), key["wits"][2]])
    assert gnn.batch == []
    need = key["want"][2][0]  # blinds state 2 draws: none on the rest-only key, whose prep_prove commits nothing
    short = [key["tapes"][0], key["tapes"][1], key["tapes"][2][: max(need - 1, 1)]]  # one block too few (every other key draws more than two)
    if need:
        with pytest.raises(hip.SpartanHipError, match="prep_prove_batch: state 2: random tape exhausted"):
            gnn.prep_prove_batch(short, witnesses=key["wits"])
    else:
        assert gnn.prep_prove_batch(short, witnesses=key["wits"])[2] == 0
        gnn._free_batch()
    assert gnn.batch == []
    used = gnn.prep_prove_batch(key["tapes"][:2], witnesses=key["wits"][:2])  # and a following batch works
    check_states(key, used)


def test_the_single_state_is_undisturbed(key):
    """self.ps made before a batch proves the oracle's words after it, and a single prep_prove after a batch is the one it always was"""
    gnn = key["gnn"]
    want_used, want_words = key["want"][0]
    assert gnn.prep_prove(key["tapes"][0]) == want_used
    ps = gnn.ps
    used = gnn.prep_prove_batch(key["tapes"][1:], witnesses=key["wits"][1:])
    assert gnn.ps is ps and len(gnn.batch) == KMAX - 1
    got, _, _ = gnn.prove(key["tapes"][0][want_used:])
    assert (got == want_words).all()
    assert all(r.ok for r in gnn.is_sat())
    for j, k in enumerate(range(1, KMAX)):
        words, _, _ = gnn.prove(key["tapes"][k][used[j]:], state=j)
        assert used[j] == key["want"][k][0] and (words == key["want"][k][1]).all()
    assert gnn.prep_prove(key["tapes"][0]) == want_used and len(gnn.batch) == KMAX - 1
    again, _, _ = gnn.prove(key["tapes"][0][want_used:])
    assert (again == want_words).all()
    with pytest.raises(hip.SpartanHipError, match="state 5 of a batch of 2"):
        gnn.prove(key["tapes"][0], state=5)
