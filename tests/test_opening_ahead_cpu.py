"""CPU: the batch opened ahead exists where a caller looks for it - sp_hyrax_prove_batch_begin / _rows / _finish / _drop and the two _observed lockstep
sum-checks declared in include/spartan_hip.h, exported by libspartan_hip.so and bound in hip.py; the driver's two flags in host.py - its calls refuse
cleanly without a device, and the compiler's resource report (tools/spill_report.py on spartan2_amd/lib/*.o) shows its two kernels
(k_ob_dvec and k_ob_ip, in kernels_opening_batch.hpp beside the others) and the ones it shares with sp_hyrax_prove_batch without a spilled VGPR, the
cooperative-addition walk within the two any kernel is allowed. No GPU."""
import ctypes
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spill_report  # noqa: E402

from spartan2_amd import hip, host  # noqa: E402

NEW = ("sp_hyrax_prove_batch_begin", "sp_hyrax_prove_batch_rows", "sp_hyrax_prove_batch_finish", "sp_hyrax_prove_batch_drop",
       "sp_sumcheck_cubic3_lockstep_observed", "sp_sumcheck_quad_lockstep_observed")
KERNELS_HEADER = os.path.join(ROOT, "spartan2_amd", "csrc", "kernels_opening_batch.hpp")
NO_SPILL = ("k_ob_dvec", "k_ob_ip", "k_ob_mask", "k_ob_rowmat", "k_ob_z")
WALK = "k_ob_walk"


def test_symbols_declared_exported_and_bound():
    declared = hip.declared_symbols()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/spartan_hip.h"
        assert hasattr(hip.lib(), name), f"libspartan_hip.so does not export {name}"
    L, S = hip._opening_batch_lib(), hip._lockstep_lib()
    for fn in (L.sp_hyrax_prove_batch_begin, L.sp_hyrax_prove_batch_rows, L.sp_hyrax_prove_batch_finish, L.sp_hyrax_prove_batch_drop,
               S.sp_sumcheck_cubic3_lockstep_observed, S.sp_sumcheck_quad_lockstep_observed):
        assert fn.argtypes, "not bound in hip.py"
    assert len(L.sp_hyrax_prove_batch_finish.argtypes) == len(L.sp_hyrax_prove_batch.argtypes) + 1
    assert hasattr(hip, "OpeningJob") and hasattr(hip, "LOCKSTEP_HOOK")
    assert (host.SS_BATCH_OPENING_AHEAD, host.SS_BATCH_OPENING_BEHIND) == (32, 64)
    assert "opening_ahead" in inspect.signature(host.SpartanSNARK.prove_batch).parameters


def test_the_calls_refuse_cleanly_without_a_device():
    L, S = hip._opening_batch_lib(), hip._lockstep_lib()
    job = ctypes.c_void_p()
    for count in (0, hip.LOCKSTEP_MAX + 1):
        assert L.sp_hyrax_prove_batch_begin(None, None, None, count, None, 1, None, 2, None, None, None, ctypes.byref(job)) == -1
        assert b"sp_hyrax_prove_batch_begin: count must be" in L.sp_last_error()
    assert L.sp_hyrax_prove_batch_begin(None, None, None, 2, None, 1, None, 2, None, None, None, ctypes.byref(job)) == -1
    assert b"sp_hyrax_prove_batch_begin: null argument" in L.sp_last_error()
    assert L.sp_hyrax_prove_batch_begin(None, None, None, 2, None, 1, None, 2, None, None, None, None) == -1
    assert job.value is None
    assert L.sp_hyrax_prove_batch_rows(None, None, None) == -1
    assert b"sp_hyrax_prove_batch_rows" in L.sp_last_error()
    nothing = (None, None, 2, None, None, 1, None, 2, None, None, 1, None, None, None, None, None)
    assert L.sp_hyrax_prove_batch_finish(None, None, *nothing) == -1
    assert b"sp_hyrax_prove_batch_finish: null argument" in L.sp_last_error()
    L.sp_hyrax_prove_batch_drop(None, None)  # nothing to drop: returns
    hook = hip.LOCKSTEP_HOOK()
    assert S.sp_sumcheck_quad_lockstep_observed(None, 2, None, 3, None, None, None, None, None, None, hook, None) == -1
    assert b"null argument" in L.sp_last_error()
    assert S.sp_sumcheck_cubic3_lockstep_observed(None, 2, None, None, 3, None, None, None, None, None, None, None, hook, None) == -1
    assert b"null argument" in L.sp_last_error()


def test_new_and_changed_kernels_do_not_spill():
    names = re.findall(r"__global__\s+void\s+__launch_bounds__\([^)]*\)\s+(k_ob_[a-z0-9_]+)\s*\(", open(KERNELS_HEADER).read())
    assert sorted(names) == sorted(NO_SPILL + (WALK,)), names
    lib = os.path.join(ROOT, "spartan2_amd", "lib")
    assert os.path.isdir(lib) and [f for f in os.listdir(lib) if f.endswith(".o")], "spartan2_amd/lib/*.o not built (run __graft_entry__.build())"
    by_base = {}
    for r in spill_report.kernels(lib):
        by_base.setdefault(re.sub(r"[<(].*$", "", re.sub(r"^void ", "", r["name"])), []).append(r)
    for name in NO_SPILL + (WALK,):
        got = by_base.get("spk::" + name)
        assert got and len(got) == 1, f"{name} is not (once) in the code objects of spartan2_amd/lib/*.o"
        assert got[0]["object"] == "capi_opening_batch.o"
        spills = got[0].get("vgpr_spill_count", 0)
        assert spills <= (2 if name == WALK else 0), f"{got[0]['name']} spills {spills} VGPRs"
