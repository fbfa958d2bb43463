"""GPU: the SPARTAN_* switch values that no default run takes (tests/switch_registry.py), each routed through existing oracle-parity tests in a child
process of its own - the switches are read once per process. Every target compares bit-exact with the oracle or the Python-integer verifiers.

A child run that passes on the default path proves nothing, so where the library prints evidence of the path (SPARTAN_ROUND_TRACE=1: one line per
sum-check round with its `tail` state; SPARTAN_HOST_LAPS=2: one line per batched round) the child runs with -s and its stderr is checked. Where it
prints none, the parameter's comment gives the shape by which the target reaches the branch.

Child runs go one at a time, each under a time limit; after one that crashed or timed out no further child starts in this process."""
import os
import re
import shlex
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 180
_abnormal = []  # the first child that crashed or timed out


def _run_child(env, targets, show_stderr=False):
    if os.environ.get("SPARTAN_TEST_CHILD"):
        pytest.skip("already inside a child process of a switched-path run")
    if _abnormal:
        pytest.fail(f"not started: an earlier child run ended abnormally ({_abnormal[0]})")
    args = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + (["-s"] if show_stderr else []) + shlex.split(targets)
    child_env = dict(os.environ, SPARTAN_TEST_CHILD="1", **dict(kv.split("=", 1) for kv in env.split()))
    t0 = time.monotonic()
    try:
        r = subprocess.run(args, cwd=ROOT, env=child_env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _abnormal.append(f"{env}: timed out after {CHILD_TIMEOUT_S} s")
        pytest.fail(_abnormal[-1])
    print(f"child [{env}] {targets}: {time.monotonic() - t0:.1f} s")
    if r.returncode < 0 or r.returncode >= 128:
        _abnormal.append(f"{env}: exit status {r.returncode}")
    tail = (r.stdout or "")[-1500:]
    assert r.returncode == 0, tail + "\n" + (r.stderr or "")[-1500:]
    assert " passed" in tail and "no tests ran" not in tail, tail
    return r.stderr or ""


# ---- evidence parsers -------------------------------------------------------------------------------------------------------------------------------
# SPARTAN_ROUND_TRACE=1 (csrc/capi_core.hip): "quad round  3 len    4096 tail 1 ...", "cubic rounds 12+13 len     64 tail 2 ..." (two rounds of the
# resident tail in one step). A round reports tail != 0 when the resident kernel produced its sums; the tail is launched by the round BEFORE it,
# over that round's table of length L <= 2^TAIL_LOG2, so the first round reporting it has length L / 2.
_ROUND = re.compile(r"^(quad|cubic) rounds? +\d+(?:\+ *\d+)? len +(\d+) tail (\d+)", re.M)
# SPARTAN_HOST_LAPS=2: "inner batched round 3 (len 4096, fused, next queued ahead): hook ..." - `fused` = this round's sums came from the previous
# round's fused bind + evaluate launch (k_bind_eval_quad_pair_small), `separate launches` = evaluated on its own
_INNER = re.compile(r"^inner batched round (\d+) \(len (\d+), (fused|separate launches)", re.M)
_BATCHED = re.compile(r"^(?:inner|outer) batched round .*$", re.M)
TAIL_WIDE_Q, TAIL_WIDE_Q_CUBIC = 256, 128  # kernels_poly.hpp: pairs of one resident block


def _rounds(err):
    rounds = [(kind, int(n), int(t)) for kind, n, t in _ROUND.findall(err)]
    assert rounds, "no sum-check round lines on stderr (SPARTAN_ROUND_TRACE=1)"
    return rounds


def _summary(rounds):
    return sorted(set(rounds))


def _tail_takes_over_at(log2):
    def check(err):
        rounds = _rounds(err)
        late = [x for x in rounds if x[2] and x[1] > 1 << (log2 - 1)]
        assert not late, f"resident tail above 2^{log2 - 1}: {_summary(late)}"
        assert any(t and n == 1 << (log2 - 1) for _, n, t in rounds), f"no tail over 2^{log2 - 1}-entry tables: {_summary(rounds)}"
        # ... and tables the default (2^16) would have given to the tail ran as ordinary rounds
        assert any(not t and 1 << (log2 - 1) < n <= 1 << 15 for _, n, t in rounds), _summary(rounds)
    return check


def _tail_budget_zero(err):
    # A multi-block tail leases its blocks from the budget; a single-block tail (q <= TAIL_WIDE_Q pairs) is not counted (capi_core.hip TailLease), so
    # with no budget only single-block tails remain: quad tables of <= 4 * 256, cubic of <= 4 * 128 entries, first reported a round later.
    rounds = _rounds(err)
    limit = {"quad": 2 * TAIL_WIDE_Q, "cubic": 2 * TAIL_WIDE_Q_CUBIC}
    multi = [x for x in rounds if x[2] and x[1] > limit[x[0]]]
    assert not multi, f"a multi-block tail with SPARTAN_TAIL_BUDGET=0: {_summary(multi)}"
    assert any(not t and 2 * TAIL_WIDE_Q < n <= 1 << 15 for _, n, t in rounds), _summary(rounds)
    assert any(t for _, _, t in rounds), f"not even a single-block tail: {_summary(rounds)}"


def _small_pairs(max_fused, must_fuse=None):
    """Inner batched rounds with SMALL_PAIR_WIDE=0: the fused launch over a table of 2L entries (q = L / 2 pairs) fits the 64 ordinary result slots
    with the fewest groups of 64 pairs a block up to SMALL_PAIR_CHUNKS: q <= 2048 * chunks. The default (wide slots) fuses every round up to 2^14."""
    def check(err):
        rounds = [(int(j), int(n), kind == "fused") for j, n, kind in _INNER.findall(err)]
        assert rounds, "no inner batched round lines on stderr (SPARTAN_HOST_LAPS=2)"
        over = sorted({n for _, n, f in rounds if f and n > max_fused})
        assert not over, f"fused rounds beyond the reach of the switch: len {over}"
        if must_fuse:
            assert any(f and n == must_fuse for _, n, f in rounds), f"no fused round of len {must_fuse}: {sorted(set(rounds))[:40]}"
        else:
            assert any(j > 0 and not f and max_fused < n <= 1 << 14 for j, n, f in rounds), f"no separate round the default fuses: {sorted(set(rounds))[:40]}"
    return check


def _never_queued_ahead(err):
    lines = _BATCHED.findall(err)
    assert lines, "no batched round lines on stderr (SPARTAN_HOST_LAPS=2)"
    ahead = [ln for ln in lines if "queued ahead" in ln]
    assert not ahead, ahead[:5]


# ---- targets ----------------------------------------------------------------------------------------------------------------------------------------
COMB = "tests/test_gpu_configs.py::test_c4_full_scalar_commit_2048_rows_matches_oracle"
C1 = "tests/test_gpu_configs.py::test_c1_c2_sha256_spartan_prove_bit_exact"
POLY_ABC = f"tests/test_gpu_r1cs.py {C1} -k 'spmv or 1024'"
SPARTAN = f"{C1} tests/test_gpu_spartan.py -k '1024 or prove_matches_oracle'"
TAILS = "tests/test_gpu_sumcheck.py tests/test_gpu_abi_gaps.py -k '(cubic_matches or quad_matches or two_round or 2_pow_21 or streaming or zero_check) and not switched'"
STREAMING = "tests/test_gpu_sumcheck.py -k '2_pow_21 or streaming'"
BATCHED = "tests/test_gpu_batched_sumcheck.py"
NN = "tests/test_gpu_neutronnova_zk.py -k prove_matches_oracle"
C2_C3 = "tests/test_gpu_configs.py::test_c1_c2_sha256_spartan_prove_bit_exact tests/test_gpu_neutronnova_zk.py -k '2048 or oracle'"

PATHS = [
    # comb tables: 2048 full-scalar rows >= comb_min_rows (256) build the key's table at window C and take k_comb_*<C> (capi_group.hip:876);
    # 0 = the batched bucket MSMs over the same rows
    pytest.param("SPARTAN_COMB_BITS=0", COMB, None, id="COMB_BITS=0"),
    pytest.param("SPARTAN_COMB_BITS=8", COMB, None, id="COMB_BITS=8"),
    pytest.param("SPARTAN_COMB_BITS=10", COMB, None, id="COMB_BITS=10"),
    pytest.param("SPARTAN_COMB_BITS=12", COMB, None, id="COMB_BITS=12"),
    pytest.param("SPARTAN_COMB_BITS=14", COMB, None, id="COMB_BITS=14"),
    # poly_ABC's column structure (capi_sparse.hip:447-475), built for every shape: the SHA-256 instances' 2^15 / 2^19 columns are nearly all short
    # (< LONG_COLUMN entries), so a window of 777 (= 3 * 7 * 37, no divisor of the power-of-two column count less the few long columns) leaves its
    # last window partly full, and a window of 1 sorts nothing
    pytest.param("SPARTAN_POLYABC_LAYOUT=natural", POLY_ABC, None, id="POLYABC_LAYOUT=natural"),
    pytest.param("SPARTAN_POLYABC_ORDER=natural", POLY_ABC, None, id="POLYABC_ORDER=natural"),
    pytest.param("SPARTAN_POLYABC_ORDER=window", POLY_ABC, None, id="POLYABC_ORDER=window"),
    pytest.param("SPARTAN_POLYABC_ORDER=window SPARTAN_POLYABC_WINDOW=1", POLY_ABC, None, id="POLYABC_WINDOW=1"),
    pytest.param("SPARTAN_POLYABC_ORDER=window SPARTAN_POLYABC_WINDOW=777", POLY_ABC, None, id="POLYABC_WINDOW=777"),
    pytest.param("SPARTAN_POLYABC_LAYOUT=natural SPARTAN_POLYABC_ORDER=window SPARTAN_POLYABC_WINDOW=777", POLY_ABC, None, id="POLYABC_natural_window"),
    # every SpartanSNARK prove with N >= 2 allocates the round-0 products unless switched off (spartan_snark.cpp:233)
    pytest.param("SPARTAN_ROUND0_PRODUCTS=0", SPARTAN, None, id="ROUND0_PRODUCTS=0"),
    # resident tail: evidence from the round trace
    pytest.param("SPARTAN_TAIL_LOG2=10 SPARTAN_ROUND_TRACE=1", TAILS, _tail_takes_over_at(10), id="TAIL_LOG2=10"),
    pytest.param("SPARTAN_TAIL_LOG2=15 SPARTAN_ROUND_TRACE=1", TAILS, _tail_takes_over_at(15), id="TAIL_LOG2=15"),
    pytest.param("SPARTAN_TAIL_BUDGET=0 SPARTAN_ROUND_TRACE=1", TAILS, _tail_budget_zero, id="TAIL_BUDGET=0"),
    # the folded second stage's slots (read only with FOLD_STAGE2=1): the streaming kernels run over tables of >= 2^19 pairs (STREAM_MIN_Q) in the
    # 2^21-row and streaming tests; 1 slot = every group behind one ticket, 7 is halved (capi_core.hip:632) to a count that divides the groups
    pytest.param("SPARTAN_FOLD_STAGE2=1 SPARTAN_FOLD_SLOTS=1", STREAMING, None, id="FOLD_SLOTS=1"),
    pytest.param("SPARTAN_FOLD_STAGE2=1 SPARTAN_FOLD_SLOTS=7", STREAMING, None, id="FOLD_SLOTS=7"),
    # fused batched rounds (capi_core.hip:2034-2047): evidence from the batched-round lines of test_quad_batched[15] (tables of 2^15 .. 2^1)
    pytest.param("SPARTAN_SMALL_PAIR_WIDE=0 SPARTAN_HOST_LAPS=2", BATCHED, _small_pairs(4096), id="SMALL_PAIR_WIDE=0"),
    pytest.param("SPARTAN_SMALL_PAIR_CHUNKS=2 SPARTAN_SMALL_PAIR_WIDE=0 SPARTAN_HOST_LAPS=2", BATCHED, _small_pairs(8192, 8192), id="SMALL_PAIR_CHUNKS=2"),
    pytest.param("SPARTAN_SMALL_PAIR_CHUNKS=16 SPARTAN_SMALL_PAIR_WIDE=0 SPARTAN_HOST_LAPS=2", BATCHED, _small_pairs(16384, 16384), id="SMALL_PAIR_CHUNKS=16"),
    # launches ahead of their challenge over tables > 2^19 entries (launch_ahead_ok) are gated: the 2^21-row and streaming sum-checks
    pytest.param("SPARTAN_GATE=0", "tests/test_gpu_sumcheck.py tests/test_gpu_spartan.py -k '2_pow_21 or streaming or prove_matches_oracle'", None, id="GATE=0"),
    # the NeutronNova ZK prove's batched sum-checks run with a host-only round hook: by default their next round is queued ahead of it
    pytest.param("SPARTAN_BATCHED_AHEAD=0 SPARTAN_HOST_LAPS=2", NN, _never_queued_ahead, id="BATCHED_AHEAD=0"),
    # the verifier-circuit instance's relaxed-Spartan sum-checks go to the host when walkers exist (the default) (neutronnova_zk.cpp:950)
    pytest.param("SPARTAN_HOST_SC=0", "tests/test_gpu_neutronnova_zk.py -k oracle", None, id="HOST_SC=0"),
    # FLAG_PREFIX_CACHE: C1 proves five times on one prep (the cached prefix reused), the driver-path test on fresh preps
    pytest.param("SPARTAN_PREFIX_CACHE=1", f"{C1} tests/test_gpu_spartan.py -k '1024 or prove_matches_oracle or every_driver_path'", None, id="PREFIX_CACHE=1"),
    # the opening's delta MSM is issued when that many inner rounds are left (spartan_snark.cpp:691); 1 = in the last round, 64 > the 15-20 rounds
    # of these instances = never inside the sum-check (the publish at :714)
    pytest.param("SPARTAN_DELTA_ROUNDS_LEFT=1", SPARTAN, None, id="DELTA_ROUNDS_LEFT=1"),
    pytest.param("SPARTAN_DELTA_ROUNDS_LEFT=64", SPARTAN, None, id="DELTA_ROUNDS_LEFT=64"),
    # z_vec armed behind the scale: the PCS prove of every Spartan prove and the eq job of the row-matrix product, one live context (capi_group.hip:1532)
    pytest.param("SPARTAN_ZVEC_ARMED=0", "tests/test_gpu_spartan.py tests/test_gpu_group.py -k 'prove_matches_oracle or rowmat_vec_eq_job or hyrax_prove_is_the'",
                 None, id="ZVEC_ARMED=0"),
    # multi-mul walks of 128 .. 1023 scalars (>= 32 blocks of 4, below the wide kernel) join in 8 groups: the openings' L^T key walks
    pytest.param("SPARTAN_WALK_GROUPS=0", "tests/test_gpu_spartan.py tests/test_gpu_group.py -k 'prove_matches_oracle or hyrax_prove_is_the'", None,
                 id="WALK_GROUPS=0"),
    # host copies of the 16-bit-window tables: every key of <= 2 bases (the single multiplications of a Spartan prove) and the narrow keys of the
    # verifier circuit's split commitments, which without them fall back to the device walk (capi_group.hip:534, sp_hyrax_commit_split_available)
    pytest.param("SPARTAN_HOST_T16=0", "tests/test_gpu_neutronnova_zk.py tests/test_gpu_spartan.py tests/test_gpu_group.py "
                 "-k 'prove_matches_oracle or commit_split or commit_rows_host'", None, id="HOST_T16=0"),
]


@pytest.mark.parametrize("env,targets,evidence", PATHS)
def test_switched_path_in_a_child_process(env, targets, evidence):
    """One non-default value of a path switch: the targets stay bit-exact against the oracle, and where the library reports the path, it was taken."""
    err = _run_child(env, targets, show_stderr=evidence is not None)
    if evidence is not None:
        evidence(err)


def test_scheduling_switches_leave_proofs_unchanged():
    """Waits and thread placement only: the runtime's blocking wait, polling before it, walkers unpinned and in the idle class, host tables on ordinary
    pages - C2 and C3 proofs stay the oracle's."""
    _run_child("SPARTAN_SYNC_SHORT=0 SPARTAN_SYNC_SPIN_US=50 SPARTAN_WALKERS_PIN=0 SPARTAN_WALKERS_IDLE=1 SPARTAN_HOST_T16_THP=0", C2_C3)


def test_trace_switches_leave_proofs_unchanged():
    """Tracing, including the stream synchronisations HOST_LAPS and PREP_TRACE add in the middle of the MSM and prove paths: C2 and C3 proofs stay
    the oracle's."""
    _run_child("SPARTAN_HOST_LAPS=1 SPARTAN_PREP_TRACE=1 SPARTAN_ROUND_TRACE=1 SPARTAN_SLOWPATH_LOG=1 SPARTAN_SLOW_PROVE_MS=0.001", C2_C3)
