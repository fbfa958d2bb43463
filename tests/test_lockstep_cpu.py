"""CPU: the lockstep sum-checks exist where a caller looks for them - declared in include/spartan_hip.h and exported by libspartan_hip.so, prove_batch
exported by libspartan_host.so - and every kernel of kernels_lockstep.hpp is in the built code objects without a spilled VGPR (tools/spill_report.py:
llvm-objcopy -> clang-offload-bundler -> llvm-readelf --notes on spartan2_amd/lib/*.o). Runs without a GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spill_report  # noqa: E402

from spartan2_amd import hip, host  # noqa: E402

SYMBOLS = ("sp_sumcheck_cubic3_lockstep", "sp_sumcheck_quad_lockstep")
KERNELS_HEADER = os.path.join(ROOT, "spartan2_amd", "csrc", "kernels_lockstep.hpp")


def test_symbols_declared_and_exported():
    declared = hip.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/spartan_hip.h"
        assert hasattr(hip.lib(), name), f"libspartan_hip.so does not export {name}"
    assert re.search(r"#define\s+SP_LOCKSTEP_MAX\s+64\b", open(hip.HEADER).read())
    assert hip.LOCKSTEP_MAX == 64
    assert hasattr(host.lib(), "ss_prove_batch")


def test_refusals_that_need_no_device():
    """count and null arguments are refused before the context is touched"""
    import ctypes

    L = hip._lockstep_lib()
    for count in (0, hip.LOCKSTEP_MAX + 1):
        assert L.sp_sumcheck_cubic3_lockstep(None, count, None, None, 3, None, None, None, None, None, None, None) == -1
        assert L.sp_sumcheck_quad_lockstep(None, count, None, 3, None, None, None, None, None, None) == -1
    assert b"lockstep" in L.sp_last_error()
    del ctypes


def header_kernels():
    """names of the __global__ functions of kernels_lockstep.hpp"""
    txt = open(KERNELS_HEADER).read()
    names = re.findall(r"__global__\s+void\s+__launch_bounds__\(\d+\)\s+(k_ls_[a-z0-9_]+)\s*\(", txt)
    assert len(names) >= 6 and len(set(names)) == len(names), names
    return names


def test_every_lockstep_kernel_is_built_without_vgpr_spills():
    lib = os.path.join(ROOT, "spartan2_amd", "lib")
    assert os.path.isdir(lib) and [f for f in os.listdir(lib) if f.endswith(".o")], "spartan2_amd/lib/*.o not built (run __graft_entry__.build())"
    rows = spill_report.kernels(lib)
    by_base = {}
    for r in rows:
        base = re.sub(r"[<(].*$", "", re.sub(r"^void ", "", r["name"]))
        by_base.setdefault(base, []).append(r)
    for name in header_kernels():
        got = by_base.get("spk::" + name)
        assert got, f"{name} is not in the code objects of spartan2_amd/lib/*.o"
        for r in got:
            assert r["object"] == "capi_lockstep.o"
            assert r.get("vgpr_spill_count", 0) == 0, f"{r['name']} spills {r['vgpr_spill_count']} VGPRs"
            assert r.get("max_flat_workgroup_size") in (64, 256), r  # 256-thread blocks; the one-wave second stage and last bind
    # both instantiations of the templated kernels are there
    assert len(by_base["spk::k_ls_sum_partials"]) == 2 and len(by_base["spk::k_ls_bind_last"]) == 2
