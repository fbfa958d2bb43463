"""CPU: the batched opening exists where a caller looks for it - sp_hyrax_prove_batch declared in include/spartan_hip.h and exported by
libspartan_hip.so, ss_prove_batch_opts exported by libspartan_host.so - refuses count and null arguments without a device, and every kernel of
kernels_opening_batch.hpp is in capi_opening_batch.o: the streaming ones without a spilled VGPR, the cooperative-addition walk with at most the two
that tests/test_spills_cpu.py allows any kernel (tools/spill_report.py on spartan2_amd/lib/*.o). Runs without a GPU."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spill_report  # noqa: E402

from spartan2_amd import hip, host  # noqa: E402

KERNELS_HEADER = os.path.join(ROOT, "spartan2_amd", "csrc", "kernels_opening_batch.hpp")
STREAMING = ("k_ob_mask", "k_ob_dvec", "k_ob_ip", "k_ob_rowmat", "k_ob_z")
WALK = "k_ob_walk"


def test_symbols_declared_and_exported():
    assert "sp_hyrax_prove_batch" in hip.declared_symbols(), "sp_hyrax_prove_batch is not declared in include/spartan_hip.h"
    assert hasattr(hip.lib(), "sp_hyrax_prove_batch"), "libspartan_hip.so does not export sp_hyrax_prove_batch"
    assert hasattr(host.lib(), "ss_prove_batch_opts") and hasattr(host.lib(), "ss_prove_batch")
    assert host.SS_BATCH_PER_PROOF_OPENING == 1


def test_refusals_that_need_no_device():
    """count 0 and 65 and null arguments are refused before the context is touched"""
    L = hip._opening_batch_lib()
    nothing = (None, None, 1, None, 2, None, None, 1, None, None, None, None, None)
    for count in (0, hip.LOCKSTEP_MAX + 1):
        assert L.sp_hyrax_prove_batch(None, None, None, count, *nothing) == -1
        assert b"sp_hyrax_prove_batch: count must be" in L.sp_last_error()
    assert L.sp_hyrax_prove_batch(None, None, None, 2, *nothing) == -1
    assert b"sp_hyrax_prove_batch: null argument" in L.sp_last_error()


def header_kernels():
    """names of the __global__ functions of kernels_opening_batch.hpp"""
    txt = open(KERNELS_HEADER).read()
    names = re.findall(r"__global__\s+void\s+__launch_bounds__\([^)]*\)\s+(k_ob_[a-z0-9_]+)\s*\(", txt)
    assert sorted(names) == sorted(STREAMING + (WALK,)), names
    return names


def test_every_kernel_is_built_and_within_its_spill_bound():
    lib = os.path.join(ROOT, "spartan2_amd", "lib")
    assert os.path.isdir(lib) and [f for f in os.listdir(lib) if f.endswith(".o")], "spartan2_amd/lib/*.o not built (run __graft_entry__.build())"
    by_base = {}
    for r in spill_report.kernels(lib):
        base = re.sub(r"[<(].*$", "", re.sub(r"^void ", "", r["name"]))
        by_base.setdefault(base, []).append(r)
    for name in header_kernels():
        got = by_base.get("spk::" + name)
        assert got and len(got) == 1, f"{name} is not (once) in the code objects of spartan2_amd/lib/*.o"
        r = got[0]
        assert r["object"] == "capi_opening_batch.o"
        spills = r.get("vgpr_spill_count", 0)
        assert spills <= (2 if name == WALK else 0), f"{r['name']} spills {spills} VGPRs"
