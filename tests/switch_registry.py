"""Every SPARTAN_* environment switch the product reads, with its default, the values worth testing and the tests that run them.

A switch is read once per process (almost always into a `static const`), so a default `-m gpu` run never takes the path behind a non-default value.
Each entry says what the other values change:

  path        how a result is computed (another kernel, geometry or host/device split): every value needs a parity test that sets it
  scheduling  waits and thread placement only: the values run together in one parity run, and a proof must not change
  trace       diagnostics on stderr (some add synchronisations): they run together in one parity run

`values` holds only values the parser KEEPS: a value it rejects or clamps away silently tests the default (SPARTAN_COMB_BITS=11 is 13,
SPARTAN_TAIL_LOG2=17 is 16), so clamped ranges are tested at their edges. `Cover.test` names the test that runs a value, `Cover.sets` the code text in
that test's file which sets it (by default the `SPARTAN_<NAME>=<value>` of a child-run parameter). tests/test_switch_registry_cpu.py checks this
module against the sources and the test files; tests/test_gpu_switched_paths.py holds the child runs of the values nothing else covers.
"""
from dataclasses import dataclass, field

PATH, SCHEDULING, TRACE = "path", "scheduling", "trace"

ABI_GAPS = "tests/test_gpu_abi_gaps.py::test_switched_code_paths_in_a_process_of_their_own"
SWITCHED = "tests/test_gpu_switched_paths.py::test_switched_path_in_a_child_process"
SCHEDULING_RUN = "tests/test_gpu_switched_paths.py::test_scheduling_switches_leave_proofs_unchanged"
TRACE_RUN = "tests/test_gpu_switched_paths.py::test_trace_switches_leave_proofs_unchanged"
DRIVER_PATHS = "tests/test_gpu_spartan.py::test_prove_is_identical_on_every_driver_path"


@dataclass(frozen=True)
class Cover:
    test: str  # "<file>::<test function>"
    sets: str = ""  # code text of that file (comments and docstrings left out) that sets the value; "" = "SPARTAN_<NAME>=<value>"


@dataclass(frozen=True)
class Switch:
    name: str  # without the SPARTAN_ prefix
    default: str  # what the product does without the variable ("unset" where only presence matters)
    cls: str
    values: dict = field(default_factory=dict)  # non-default value -> tuple of Cover
    source: str = ""  # where the parser is
    note: str = ""


def _child(*tests):
    return tuple(Cover(t) for t in tests)


_ENTRIES = [
    # ---- path ------------------------------------------------------------------------------------------------------------------------------------------
    Switch("COMB_BITS", "13", PATH, {v: _child(SWITCHED) for v in ("0", "8", "10", "12", "14")}, "spartan2_amd/csrc/capi_comb.hip:19",
           "signed comb window width C of the key's fixed-base tables (k_comb_*<C>, ceil(257 / C) windows); 0 = no comb path (bucket MSMs). "
           "Other values fall back to 13."),
    Switch("COMB_MINW", "3", PATH, {"2": _child(ABI_GAPS)}, "spartan2_amd/csrc/capi_comb.hip:95", "waves per SIMD of the comb kernels"),
    Switch("PIP_MINW", "3", PATH, {"2": _child(ABI_GAPS)}, "spartan2_amd/csrc/capi_pippenger.hip:31", "waves per SIMD of the Pippenger bucket kernels"),
    Switch("FBTABLES_OLD", "0", PATH, {"1": _child(ABI_GAPS)}, "spartan2_amd/csrc/capi_group.hip:547", "round-5 fixed-base table build"),
    Switch("FOLD_STAGE2", "0", PATH, {"1": _child(ABI_GAPS)}, "spartan2_amd/csrc/capi_core.hip:608", "second stage folded into the streaming producers"),
    Switch("FOLD_SLOTS", "64", PATH, {"1": _child(SWITCHED), "7": _child(SWITCHED)}, "spartan2_amd/csrc/capi_core.hip:627",
           "slots of the folded second stage, clamped to 1..64; read only with FOLD_STAGE2=1. 7 is halved to a count that divides the groups (7 -> 3 -> 1)."),
    Switch("HAND_N_CUBIC", "16", PATH, {"256": _child(ABI_GAPS), "64": _child(ABI_GAPS)}, "spartan2_amd/csrc/capi_core.hip:760",
           "table length of the resident tail's hand-over to the host (cubic); clamped above at 256"),
    Switch("HAND_N_QUAD", "32", PATH, {"512": _child(ABI_GAPS), "128": _child(ABI_GAPS)}, "spartan2_amd/csrc/capi_core.hip:755",
           "table length of the resident tail's hand-over to the host (quad); clamped above at 512"),
    Switch("VC_SPLIT", "1", PATH, {"0": _child(ABI_GAPS)}, "spartan2_amd/host/verifier_circuit.hpp:400", "verifier-circuit round commitments through the device walk"),
    Switch("WALKERS", "8", PATH, {"0": _child(ABI_GAPS)}, "spartan2_amd/csrc/walk_pool.hpp:186", "polling host threads; 0 = none (device forms of the split work)"),
    Switch("POLYABC_LAYOUT", "permuted", PATH, {"natural": _child(SWITCHED)}, "spartan2_amd/csrc/capi_sparse.hip:469",
           "poly_ABC's column-major structure stored in column order (col_permuted = false)"),
    Switch("POLYABC_ORDER", "sorted", PATH, {"natural": _child(SWITCHED), "window": _child(SWITCHED)}, "spartan2_amd/csrc/capi_sparse.hip:448",
           "walk order of the short columns: unsorted, or sorted inside windows of POLYABC_WINDOW columns"),
    Switch("POLYABC_WINDOW", "4096", PATH, {"1": _child(SWITCHED), "777": _child(SWITCHED)}, "spartan2_amd/csrc/capi_sparse.hip:454",
           "window of POLYABC_ORDER=window (read only with it); any value > 0. 777 leaves the last window partly full."),
    Switch("ROUND0_PRODUCTS", "1", PATH, {"0": _child(SWITCHED)}, "spartan2_amd/host/spartan_snark.cpp:227",
           "outer round 1 evaluated straight from Az, Bz, Cz instead of the products of the matrix-vector pass"),
    Switch("TAIL_LOG2", "16", PATH, {"10": _child(SWITCHED), "15": _child(SWITCHED)}, "spartan2_amd/csrc/capi_core.hip:1013",
           "table length from which the resident sum-check tail takes over, clamped to 2^10..2^16"),
    Switch("TAIL_BUDGET", "64", PATH, {"0": _child(SWITCHED)}, "spartan2_amd/csrc/capi_core.hip:1118",
           "process-wide budget of resident tail blocks; 0 = only single-block tails (they are not counted), ordinary rounds before them"),
    Switch("SMALL_PAIR_CHUNKS", "1", PATH, {"2": _child(SWITCHED), "16": _child(SWITCHED)}, "spartan2_amd/csrc/capi_core.hip:2036",
           "groups of 64 pairs a block of the fused batched rounds may take, clamped to 1..16; more than one group is only needed above the "
           "result slots, so the child runs pair it with SMALL_PAIR_WIDE=0"),
    Switch("SMALL_PAIR_WIDE", "1", PATH, {"0": _child(SWITCHED)}, "spartan2_amd/csrc/capi_core.hip:2041",
           "fused batched rounds limited to the 64 ordinary result slots (q <= 2048 pairs)"),
    Switch("GATE", "1", PATH, {"0": _child(SWITCHED)}, "spartan2_amd/csrc/capi_core.hip:1088", "launches over tables > 2^19 wait for their challenge on the host"),
    Switch("BATCHED_AHEAD", "1", PATH, {"0": _child(SWITCHED)}, "spartan2_amd/csrc/capi_core.hip:2168", "batched rounds never queued ahead of the round hook"),
    Switch("HOST_SC", "1", PATH, {"0": _child(SWITCHED)}, "spartan2_amd/host/neutronnova_zk.cpp:947",
           "relaxed-Spartan sum-checks of the verifier-circuit instance on the device"),
    Switch("PREFIX_CACHE", "0", PATH, {"1": _child(SWITCHED)}, "spartan2_amd/host/spartan_snark.cpp:220", "FLAG_PREFIX_CACHE: the transcript prefix kept per prep"),
    Switch("DELTA_ROUNDS_LEFT", "17", PATH, {"1": _child(SWITCHED), "64": _child(SWITCHED)}, "spartan2_amd/host/spartan_snark.cpp:71",
           "inner-sum-check rounds left when the opening's delta MSM is issued (>= 1); above the round count it falls through to the publish"),
    Switch("ZVEC_ARMED", "1", PATH, {"0": _child(SWITCHED)}, "spartan2_amd/csrc/capi_group.hip:1780", "z_vec launched behind the scale, not armed ahead"),
    Switch("WALK_GROUPS", "1", PATH, {"0": _child(SWITCHED)}, "spartan2_amd/csrc/capi_group.hip:2106", "multi-mul walks joined once on the device"),
    Switch("HOST_T16", "1", PATH, {"0": _child(SWITCHED)}, "spartan2_amd/csrc/capi_group.hip:568", "no host copies of the 16-bit-window tables: the split commitments are refused and the verifier circuit's round commitments take the device walk"),
    Switch("LZ_DIRECT", "0", PATH, {"1": (Cover(DRIVER_PATHS, 'monkeypatch.setenv("SPARTAN_LZ_DIRECT", "1")'),)}, "spartan2_amd/host/spartan_snark.cpp:220",
           "comm_LZ in the reference's order"),
    Switch("MAIL_DEV", "1", PATH, {"0": (Cover(DRIVER_PATHS, 'monkeypatch.setenv("SPARTAN_MAIL_DEV", "0")'),)}, "spartan2_amd/csrc/capi_core.hip:217",
           "mailbox in host memory (read when a context is created)"),
    Switch("PREP_TABLES", "lazy", PATH, {v: (Cover(DRIVER_PATHS, 'for mode in ("off", "sync", "prep"):'),) for v in ("off", "sync", "prep")},
           "spartan2_amd/host/spartan_snark.cpp:225", "when the row tables of the prepared witness are built (read at every prep)"),
    Switch("KEY_TABLES", "1", PATH,
           {"0": (Cover(DRIVER_PATHS, 'monkeypatch.setenv("SPARTAN_KEY_TABLES", "0")'),
                  Cover("tests/test_gpu_group.py::test_hyrax_prove_is_the_oracles_pcs_prove", '(16, "0")'))},
           "spartan2_amd/csrc/capi_group.hip:2250", "bucket MSMs instead of the key's window tables (read at every call)"),
    Switch("SHARD_GATHER_LOG2", "16", PATH,
           {"0": (Cover("tests/test_gpu_sharded_snark.py::test_sharded_prove_is_the_unsharded_proof", '(2, "synthetic", 0)'),),
            "8": (Cover("tests/test_gpu_sharded_snark.py::test_sharded_prove_is_the_unsharded_proof", '(2, "segments", 8)'),)},
           "spartan2_amd/host/sharded_snark.cpp:246", "where the sharded sum-checks hand over from slices to gathered tables, clamped to 0..24"),
    Switch("SHA_PORTABLE", "unset", PATH, {"1": (Cover("tests/test_wire_cpu.py::test_sha256_both_block_functions", 'SPARTAN_SHA_PORTABLE="1"'),)},
           "spartan2_amd/csrc/sha256.hpp:91", "portable SHA-256 instead of the SHA-NI one (set = portable)"),
    # ---- scheduling ------------------------------------------------------------------------------------------------------------------------------------
    Switch("SYNC_SHORT", "1", SCHEDULING, {"0": _child(SCHEDULING_RUN)}, "spartan2_amd/csrc/capi_core.hip:66", "the runtime's blocking stream wait"),
    Switch("SYNC_SPIN_US", "0", SCHEDULING, {"50": _child(SCHEDULING_RUN)}, "spartan2_amd/csrc/capi_core.hip:36", "poll for n us before the runtime's wait"),
    Switch("WALKERS_PIN", "1", SCHEDULING, {"0": _child(SCHEDULING_RUN)}, "spartan2_amd/csrc/walk_pool.hpp:70", "walkers not pinned near the caller"),
    Switch("WALKERS_IDLE", "0", SCHEDULING, {"1": _child(SCHEDULING_RUN)}, "spartan2_amd/csrc/walk_pool.hpp:153", "walkers in SCHED_IDLE"),
    Switch("HOST_T16_THP", "1", SCHEDULING, {"0": _child(SCHEDULING_RUN)}, "spartan2_amd/csrc/capi_group.hip:592", "no huge pages for the host tables"),
    # ---- trace -----------------------------------------------------------------------------------------------------------------------------------------
    Switch("HOST_LAPS", "unset", TRACE, {"1": _child(TRACE_RUN), "2": _child(SWITCHED)}, "spartan2_amd/host/spartan_snark.cpp:1168 and ten more",
           "laps on stderr; some sites take any value, others only 1 or 2 (batched rounds); adds stream_sync calls mid-path"),
    Switch("PREP_TRACE", "unset", TRACE, {"1": _child(TRACE_RUN)}, "spartan2_amd/host/spartan_snark.cpp:226", "prep phases on stderr, one synchronise"),
    Switch("ROUND_TRACE", "0", TRACE, {"1": _child(TRACE_RUN, SWITCHED)}, "spartan2_amd/csrc/capi_core.hip:1002", "one line per sum-check round"),
    Switch("SLOWPATH_LOG", "unset", TRACE, {"1": _child(TRACE_RUN)}, "spartan2_amd/csrc/capi_core.hip:27", "waits that fell back to the slow path"),
    Switch("SLOW_PROVE_MS", "0", TRACE, {"0.001": _child(TRACE_RUN)}, "spartan2_amd/host/spartan_snark.cpp:2350", "phases of proves slower than t ms"),
]

SWITCHES = {s.name: s for s in _ENTRIES}
assert len(SWITCHES) == len(_ENTRIES), "a switch is registered twice"
