"""CPU: sp_poly_abc_batch exists where a caller looks for it - declared in include/spartan_hip.h and exported by libspartan_hip.so, the prove_batch
options of host.py equal the driver's enum - it refuses null arguments before it touches a device, and every kernel of kernels_polyabc_batch.hpp is in
the built code objects without a spilled VGPR (tools/spill_report.py on spartan2_amd/lib/*.o). Runs without a GPU."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spill_report  # noqa: E402

from spartan2_amd import hip, host  # noqa: E402

SYMBOLS = ("sp_poly_abc_batch", "sp_poly_abc_batch_chunk")
KERNELS_HEADER = os.path.join(ROOT, "spartan2_amd", "csrc", "kernels_polyabc_batch.hpp")
DRIVER = os.path.join(ROOT, "spartan2_amd", "host", "spartan_snark.cpp")
FLAGS = ("SS_BATCH_PER_PROOF_OPENING", "SS_BATCH_PER_PROOF_POLYABC", "SS_BATCH_BATCHED_POLYABC", "SS_BATCH_PER_PROOF_REST_COMMIT", "SS_BATCH_BATCHED_REST_COMMIT")


def test_symbols_declared_and_exported():
    declared = hip.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/spartan_hip.h"
        assert hasattr(hip.lib(), name), f"libspartan_hip.so does not export {name}"
    assert hip.poly_abc_batch_chunk() in (2, 4)
    assert hasattr(host.lib(), "ss_prove_batch_opts")


def test_flags_equal_the_drivers_enum():
    src = open(DRIVER).read()
    values = {}
    for name in FLAGS:
        m = re.search(r"\b" + name + r"\s*=\s*(\d+)\s*[,}\n]", src)
        assert m, f"{name} is not in the enum of spartan_snark.cpp"
        values[name] = int(m.group(1))
        assert getattr(host, name) == values[name], name
    assert [values[n] for n in FLAGS] == [1, 2, 4, 8, 16]


def test_refusals_that_need_no_device():
    L = hip.lib()
    sz = ctypes.c_size_t
    dummy = ctypes.c_void_p(8)  # never dereferenced: the null checks come first
    r = (ctypes.c_uint64 * 8)()
    outs = (ctypes.c_void_p * 2)()
    for c, s, r_x, rr, o in ((None, dummy, r, r, outs), (dummy, None, r, r, outs), (dummy, dummy, None, r, outs), (dummy, dummy, r, None, outs), (dummy, dummy, r, r, None)):
        assert L.sp_poly_abc_batch(c, s, sz(2), r_x, sz(1), rr, sz(4), o) == -1
        assert b"poly_abc_batch" in L.sp_last_error()


def header_kernels():
    names = re.findall(r"__global__\s+void\s+__launch_bounds__\(\d+\)\s+(k_pab_[a-z0-9_]+)\s*\(", open(KERNELS_HEADER).read())
    assert len(names) == 3 and len(set(names)) == 3, names
    return names


def test_every_kernel_is_built_without_vgpr_spills():
    lib = os.path.join(ROOT, "spartan2_amd", "lib")
    assert os.path.isdir(lib) and [f for f in os.listdir(lib) if f.endswith(".o")], "spartan2_amd/lib/*.o not built (run __graft_entry__.build())"
    by_base = {}
    for r in spill_report.kernels(lib):
        base = re.sub(r"[<(].*$", "", re.sub(r"^void ", "", r["name"]))
        by_base.setdefault(base, []).append(r)
    for name in header_kernels():
        got = by_base.get("spk::" + name)
        assert got, f"{name} is not in the code objects of spartan2_amd/lib/*.o"
        for r in got:
            assert r["object"] == "capi_sparse.o"
            assert r.get("vgpr_spill_count", 0) == 0, f"{r['name']} spills {r['vgpr_spill_count']} VGPRs"
    assert len(by_base["spk::k_pab_walk"]) == 2  # the full chunk and the ragged one
    # the per-proof kernel is still there, as it was
    assert len(by_base["spk::k_polyabc_short_and_long"]) == 1
