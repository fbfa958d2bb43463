"""GPU parity: SpartanSNARK.prep_prove_batch in one pass (ss_prep_prove_batch_opts / ss_prep_prove_sha256_batch_opts) - K prep states of one key with the
commitments through sp_hyrax_commit_batch and, on request, the cached products through sp_multiply_vec_chunked. State k must be WORD FOR WORD the state the CPU
oracle's prep_prove makes of witness k with tape k - commitment rows, cached Az / Bz / Cz, tape blocks used - and must prove, alone and in a batch,
to the oracle's proof. The per-state flags and the loop of single calls give the same states."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
from spartan2_amd import frontend, hip, host

pytestmark = pytest.mark.gpu

SYNTHETIC = {
    "5x7": dict(n_groups=5, seed=7, num_public=2),
    # shared, precommitted and rest segments, all non-empty
    "40xDEADBEEF_split": dict(n_groups=40, seed=0xDEADBEEF, num_public=5, shared_permille=200, precommitted_permille=500),
}
PATHS = {"one_pass": {}, "loop": dict(one_pass=False), "per_state_commit": dict(per_state_commit=True), "per_state_matvec": dict(per_state_matvec=True),
         "chunked_matvec": dict(chunked_matvec=True), "per_state_both": dict(per_state_commit=True, per_state_matvec=True)}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def oracles_prepped(insts, seed):
    """one oracle per instance, prepared on its own tape -> (oracles, prep tapes, blocks used, exports)"""
    osps, tapes, used, exports = [], [], [], []
    for k, inst in enumerate(insts):
        osp = ol.OracleSpartan(inst)
        tape = ol.make_tape(seed + k, 1024)
        used.append(osp.prep_prove(tape))
        osps.append(osp)
        tapes.append(tape)
        exports.append(osp.prep_export())
    return osps, tapes, used, exports


def state_export(gsp, k):
    gsp.ps, gsp.publics = gsp.batch[k]
    return gsp.prep_export()


def check_exports(gsp, exports):
    assert len(gsp.batch) == len(exports)
    for k, want in enumerate(exports):
        got = state_export(gsp, k)
        for name, g, w in zip(("comm_W", "caz", "cbz", "ccz"), got, want):
            assert g.shape == w.shape and (g == w).all(), f"state {k}: {name} differs from the oracle's"
    gsp.ps = None


@pytest.fixture(scope="module", params=sorted(SYNTHETIC))
def synthetic(request):
    kw = SYNTHETIC[request.param]
    insts = [frontend.synthetic_circuit(witness_seed=1000 * k, **kw) for k in range(5)]
    if "split" in request.param:
        i = insts[0]
        assert i.num_shared and i.num_precommitted and i.num_rest
    return (insts,) + oracles_prepped(insts, 4100)


@pytest.mark.parametrize("K", [1, 2, 5])
def test_synthetic_states_equal_the_oracle_s_and_prove(ctx, synthetic, K):
    insts, osps, prep_tapes, prep_used, exports = (x[:K] for x in synthetic)
    gsp = host.SpartanSNARK(ctx, insts[0])
    assert gsp.prep_prove_batch(prep_tapes, witnesses=insts) == prep_used
    assert gsp.ps is None and len(gsp.batch) == K
    ph = gsp.batch_prep_phases
    assert ph["total"] > 0 and ph["commit"] > 0
    check_exports(gsp, exports)
    # prep_ms of a state: the batch's phases divided by the count
    gsp.ps = gsp.batch[K - 1][0]
    assert abs(gsp.prep_phases()["total"] * K - ph["total"]) < 1e-6 * ph["total"]
    gsp.ps = None
    # the batch proves to the oracle's proofs, and so does one state alone
    tapes = [ol.make_tape(4200 + 7 * K + k, 4096) for k in range(K)]
    got, _ = gsp.prove_batch(tapes)
    for k, (words, used) in enumerate(got):
        want, want_used, _ = osps[k].prove(tapes[k])
        assert used == want_used and (words == want).all(), f"proof {k} differs from the oracle's"
        assert gsp.verify(words) == 0
    j = K - 1
    gsp.ps, gsp.publics = gsp.batch[j]
    tape = ol.make_tape(4300 + K, 4096)
    words, used, _ = gsp.prove(tape)
    want, want_used, _ = osps[j].prove(tape)
    assert used == want_used and (words == want).all()
    assert gsp.verify(words) == 0
    gsp.close()
    assert gsp.batch == [] and gsp.ps is None


@pytest.mark.parametrize("path", [p for p in sorted(PATHS) if p != "one_pass"])
def test_the_other_paths_give_the_same_states(ctx, synthetic, path):
    insts, osps, prep_tapes, prep_used, exports = synthetic  # five states: the chunked product crosses a chunk boundary
    gsp = host.SpartanSNARK(ctx, insts[0])
    assert gsp.prep_prove_batch(prep_tapes, witnesses=insts, **PATHS[path]) == prep_used
    check_exports(gsp, exports)
    gsp.close()


def test_states_of_the_key_s_own_instance(ctx, synthetic):
    """no witnesses, no messages: K states of the instance the key was set up from, each with its own blinds"""
    insts, osps, prep_tapes, prep_used, exports = synthetic
    gsp = host.SpartanSNARK(ctx, insts[0])
    tapes = [prep_tapes[0], ol.make_tape(4400, 1024)]
    assert gsp.prep_prove_batch(tapes) == [prep_used[0]] * 2
    got0, got1 = state_export(gsp, 0), state_export(gsp, 1)
    for g, w in zip(got0, exports[0]):
        assert (g == w).all()
    assert not (got1[0] == got0[0]).all()  # other blinds
    for a, b in zip(got1[1:], got0[1:]):
        assert (a == b).all()  # the same cached products
    gsp.close()


@pytest.mark.parametrize("n", [3, 150], ids=["3B", "150B"])
def test_sha256_batch_of_three_messages(ctx, n):
    K = 3
    msgs = [bytes((37 * i + 11 * k + n) % 256 for i in range(n)) for k in range(K)]
    insts = [frontend.sha256_circuit(m) for m in msgs]
    osps, prep_tapes, prep_used, exports = oracles_prepped(insts, 4500 + n)
    gsp = host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(n)))
    assert gsp.prep_prove_batch(prep_tapes, msgs=msgs) == prep_used
    for k in range(K):
        assert (gsp.batch[k][1] == insts[k].publics).all()
    assert not (gsp.batch[0][1] == gsp.batch[1][1]).all()
    check_exports(gsp, exports)
    tapes = [ol.make_tape(4600 + n + k, 8192) for k in range(K)]
    got, _ = gsp.prove_batch(tapes)
    for k, (words, used) in enumerate(got):
        want, want_used, _ = osps[k].prove(tapes[k])
        assert used == want_used and (words == want).all()
    # the loop of single calls gives the same states and publics
    assert gsp.prep_prove_batch(prep_tapes, msgs=msgs, one_pass=False) == prep_used
    check_exports(gsp, exports)
    gsp.close()


def test_is_sat_on_a_state_of_a_batch(ctx):
    kw = SYNTHETIC["5x7"]
    insts = [frontend.synthetic_circuit(witness_seed=1000 * k, **kw) for k in range(3)]
    tapes = [ol.make_tape(4700 + k, 1024) for k in range(3)]
    gsp = host.SpartanSNARK(ctx, insts[0])
    gsp.prep_prove_batch(tapes, witnesses=insts)
    single = host.SpartanSNARK(ctx, insts[1])
    single.prep_prove(tapes[1])
    gsp.ps, gsp.publics = gsp.batch[1]
    wrong = np.ascontiguousarray(insts[1].publics, dtype=np.uint64) + np.uint64(1)
    for pubs in (None, wrong):
        a, b = gsp.is_sat(publics=pubs), single.is_sat(publics=pubs)
        assert (a.ok, a.reason, a.num_failing, a.first_failing, a.bad_commitment_rows) == (b.ok, b.reason, b.num_failing, b.first_failing, b.bad_commitment_rows)
    assert gsp.is_sat().ok and not gsp.is_sat(publics=wrong).ok
    # the commitment of ANOTHER state of the batch is not this state's
    other = state_export(gsp, 2)[0]
    gsp.ps, gsp.publics = gsp.batch[1]
    rep = gsp.is_sat(commitment=other)
    assert not rep.ok and len(rep.bad_commitment_rows) > 0
    single.close()
    gsp.close()


def test_a_wrong_witness_names_its_state_and_the_key_stays_usable(ctx):
    kw = SYNTHETIC["5x7"]
    insts = [frontend.synthetic_circuit(witness_seed=1000 * k, **kw) for k in range(3)]
    osps, prep_tapes, prep_used, exports = oracles_prepped(insts, 4800)
    gsp = host.SpartanSNARK(ctx, insts[0])

    class Short:
        witness = insts[1].witness[:-1]
        publics = insts[1].publics

    with pytest.raises(hip.SpartanHipError, match=r"prep_prove_batch: state 1: InvalidWitnessLength"):
        gsp.prep_prove_batch(prep_tapes, witnesses=[insts[0], Short, insts[2]])
    assert gsp.batch == []
    # the entry point itself: one length for all states, checked before any device work; nothing is written to out_ps
    import ctypes

    L = host.lib()
    K = 3
    ws = [np.ascontiguousarray(i.witness, dtype=np.uint64) for i in insts]
    wptr = (hip.c_u64p * K)(*[hip.p64(w) for w in ws])
    tptr = (hip.c_u8p * K)(*[hip.p8(t) for t in prep_tapes])
    tblk = (ctypes.c_size_t * K)(*[t.shape[0] for t in prep_tapes])
    pss = (ctypes.c_void_p * K)()
    rc = L.ss_prep_prove_batch_opts(gsp.pk, wptr, ctypes.c_size_t(len(ws[0]) - 1), ctypes.c_size_t(K), 1, tptr, tblk, None, pss, None, ctypes.c_uint(0))
    assert rc == -2 and b"prep_prove_batch: state 0: InvalidWitnessLength" in L.ss_last_error()
    assert not any(pss[k] for k in range(K))
    # a tape too short for state 2's blinds: the states made so far are freed, the error names the state
    short_tapes = [prep_tapes[0], prep_tapes[1], prep_tapes[2][:0]]
    if prep_used[2] > 0:
        with pytest.raises(hip.SpartanHipError, match=r"prep_prove_batch: state 2: random tape exhausted"):
            gsp.prep_prove_batch(short_tapes, witnesses=insts)
        assert gsp.batch == []
    assert gsp.prep_prove_batch(prep_tapes, witnesses=insts) == prep_used
    check_exports(gsp, exports)
    gsp.close()


def test_prep_prove_on_a_short_tape_fails_as_it_always_did_and_the_key_stays_usable(ctx):
    """prep_prove is the count-1 case of the batch driver: its errors still carry no batch prefix (code and message recorded before the two drivers
    became one), and the same entry point through ss_prep_prove_batch with count 1 still names the state"""
    inst = frontend.synthetic_circuit(witness_seed=0, **SYNTHETIC["5x7"])
    tape = ol.make_tape(4900, 1024)
    osp = ol.OracleSpartan(inst)
    used = osp.prep_prove(tape)
    assert used > 0
    gsp = host.SpartanSNARK(ctx, inst)
    with pytest.raises(hip.SpartanHipError) as e:
        gsp.prep_prove(tape[:0])
    assert str(e.value) == "rc=-5: random tape exhausted"
    assert gsp.ps is None
    with pytest.raises(hip.SpartanHipError) as e:
        gsp.prep_prove_batch([tape[:0]], witnesses=[inst])
    assert str(e.value) == "rc=-5: prep_prove_batch: state 0: random tape exhausted"
    assert gsp.prep_prove(tape) == used
    for g, w in zip(gsp.prep_export(), osp.prep_export()):
        assert (g == w).all()
    ptape = ol.make_tape(4901, 4096)
    words, pused, _ = gsp.prove(ptape)
    want, want_used, _ = osp.prove(ptape)
    assert pused == want_used and (words == want).all()
    gsp.close()


_TRACE_CHILD = """
import ctypes, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import oracle_lib as ol
from spartan2_amd import frontend, hip, host
ctx = hip.Context(0)
inst = frontend.synthetic_circuit(n_groups=5, seed=7, num_public=2)
gsp = host.SpartanSNARK(ctx, inst)
tape = ol.make_tape(4910, 1024)
sys.stderr.write("single\\n"); sys.stderr.flush()
gsp.prep_prove(tape)
sys.stderr.write("batch of one\\n"); sys.stderr.flush()
w = np.ascontiguousarray(inst.witness, dtype=np.uint64)
wptr = (hip.c_u64p * 1)(hip.p64(w))
tptr = (hip.c_u8p * 1)(hip.p8(tape))
tblk = (ctypes.c_size_t * 1)(tape.shape[0])
pss = (ctypes.c_void_p * 1)()
rc = host.lib().ss_prep_prove_batch(gsp.pk, wptr, ctypes.c_size_t(len(w)), ctypes.c_size_t(1), 1, tptr, tblk, None, pss, None)
assert rc == 0, host.lib().ss_last_error()
host.lib().ss_prep_free(ctypes.c_void_p(pss[0]))
gsp.close(); ctx.close()
"""


def test_the_prep_trace_lines_of_the_single_and_the_count_one_batch_entry_points():
    """SPARTAN_PREP_TRACE=1 in a child process (the lines go to the C library's stderr): ss_prep_prove prints the `prep_prove:` line, ss_prep_prove_batch with count 1 the
    `prep_prove_batch(1):` line - the forms recorded before the two drivers became one"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _TRACE_CHILD.format(root=root, tests=os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPARTAN_PREP_TRACE="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    num = r"\d+\.\d{3}"
    phases = rf"witness {num} commit {num} tables {num} matvec {num} scratch {num} total {num} ms"
    lines = [l for l in r.stderr.splitlines() if l.startswith(("single", "batch of one", "prep_prove"))]
    assert len(lines) == 4 and lines[0] == "single" and lines[2] == "batch of one", lines
    assert re.fullmatch(rf"prep_prove: {phases}", lines[1]), lines[1]
    assert re.fullmatch(rf"prep_prove_batch\(1\): {phases}", lines[3]), lines[3]
