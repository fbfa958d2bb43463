"""CPU: the one-pass prep_prove exists where a caller looks for it - sp_hyrax_commit_batch and sp_multiply_vec_chunked declared in include/spartan_hip.h
and exported by libspartan_hip.so, the four ss_prep_prove*_batch* entry points exported by libspartan_host.so - refuses count 0 and null arguments
without a device, and its two kernels are in the code objects once each without a spilled VGPR (tools/spill_report.py on spartan2_amd/lib/*.o).
Runs without a GPU."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spill_report  # noqa: E402

from spartan2_amd import hip, host  # noqa: E402

SP_SYMBOLS = ("sp_hyrax_commit_batch", "sp_multiply_vec_chunked")
SS_SYMBOLS = ("ss_prep_prove_batch", "ss_prep_prove_batch_opts", "ss_prep_prove_sha256_batch", "ss_prep_prove_sha256_batch_opts")
KERNELS = {"k_commit_canon_classify": ("capi_group.o", "kernels_msm.hpp"), "k_spmv3_multi": ("capi_sparse.o", "kernels_spmv_multi.hpp")}


def test_symbols_declared_and_exported():
    for name in SP_SYMBOLS + ("sp_multiply_vec_chunk", "sp_hyrax_commit_batch_workspace"):
        assert name in hip.declared_symbols(), f"{name} is not declared in include/spartan_hip.h"
        assert hasattr(hip.lib(), name), f"libspartan_hip.so does not export {name}"
    for name in SS_SYMBOLS:
        assert hasattr(host.lib(), name), f"libspartan_host.so does not export {name}"
    assert (host.SS_PREP_PER_STATE_COMMIT, host.SS_PREP_PER_STATE_MATVEC, host.SS_PREP_CHUNKED_MATVEC) == (1, 2, 4)
    assert hip.SPMV_KC == hip.multiply_vec_chunk() >= 2
    assert hip.hyrax_commit_batch_workspace() == 1 << 23


def test_refusals_that_need_no_device():
    """count 0 and null arguments are refused before a context or a key is touched"""
    L, H = hip.lib(), host.lib()
    sz = ctypes.c_size_t
    one = (ctypes.c_void_p * 1)()
    assert L.sp_hyrax_commit_batch(None, None, sz(0), one, sz(0), sz(1), one, one) == -1
    assert b"sp_hyrax_commit_batch: count must be at least 1" in L.sp_last_error()
    for args in ((None, None, sz(1), one, sz(0), sz(1), one, one), (one, one, sz(1), None, sz(0), sz(1), one, one), (one, one, sz(1), one, sz(0), sz(1), one, None)):
        assert L.sp_hyrax_commit_batch(*args) == -1
        assert b"sp_hyrax_commit_batch: null argument" in L.sp_last_error()
    assert L.sp_hyrax_commit_batch(one, one, sz(1), one, sz(0), sz(1), None, one) == -1
    assert b"sp_hyrax_commit_batch: null blinds" in L.sp_last_error()
    assert L.sp_hyrax_commit_batch(one, one, sz(1), one, sz(0), sz(1), one, one) == -1
    assert b"sp_hyrax_commit_batch: null table, polynomial 0" in L.sp_last_error()
    assert L.sp_multiply_vec_chunked(None, None, None, sz(2), None, None, None) == -1
    assert b"multiply_vec_chunked: null argument" in L.sp_last_error()
    assert L.sp_multiply_vec_chunked(one, one, None, sz(2), one, one, one) == -1
    assert b"multiply_vec_chunked: null argument" in L.sp_last_error()
    for fn, args in ((H.ss_prep_prove_batch_opts, (one, one, sz(5), sz(0), 1, one, one, None, one, None, ctypes.c_uint(0))),
                     (H.ss_prep_prove_batch, (one, one, sz(5), sz(0), 1, one, one, None, one, None)),
                     (H.ss_prep_prove_sha256_batch_opts, (one, one, one, sz(3), sz(0), 1, one, one, None, one, one, None, ctypes.c_uint(0))),
                     (H.ss_prep_prove_sha256_batch, (one, one, one, sz(3), sz(0), 1, one, one, None, one, one, None))):
        assert fn(*args) == -1
        assert b"prep_prove_batch: count must be at least 1" in H.ss_last_error()
    assert H.ss_prep_prove_batch_opts(None, one, sz(5), sz(2), 1, one, one, None, one, None, ctypes.c_uint(0)) == -1
    assert b"prep_prove_batch: null argument" in H.ss_last_error()
    assert H.ss_prep_prove_batch_opts(one, one, sz(5), sz(2), 1, one, one, None, None, None, ctypes.c_uint(0)) == -1
    assert b"prep_prove_batch: null argument" in H.ss_last_error()
    assert H.ss_prep_prove_sha256_batch_opts(one, None, one, sz(3), sz(2), 1, one, one, None, one, one, None, ctypes.c_uint(0)) == -1
    assert b"prep_prove_batch: null argument" in H.ss_last_error()
    assert H.ss_prep_prove_sha256_batch_opts(one, one, one, sz(3), sz(2), 1, one, one, None, one, None, None, ctypes.c_uint(0)) == -1
    assert b"prep_prove_batch: null argument" in H.ss_last_error()


def test_each_kernel_is_built_once_without_spills():
    lib = os.path.join(ROOT, "spartan2_amd", "lib")
    assert os.path.isdir(lib) and [f for f in os.listdir(lib) if f.endswith(".o")], "spartan2_amd/lib/*.o not built (run __graft_entry__.build())"
    by_base = {}
    for r in spill_report.kernels(lib):
        base = re.sub(r"[<(].*$", "", re.sub(r"^void ", "", r["name"]))
        by_base.setdefault(base, []).append(r)
    for name, (obj, header) in KERNELS.items():
        txt = open(os.path.join(ROOT, "spartan2_amd", "csrc", header)).read()
        assert re.search(r"__global__\s+void\s+__launch_bounds__\([^)]*\)\s+" + name + r"\s*\(", txt), f"{name} is not in {header}"
        got = by_base.get("spk::" + name)
        assert got and len(got) == 1, f"{name} is not (once) in the code objects of spartan2_amd/lib/*.o"
        r = got[0]
        assert r["object"] == obj
        assert r.get("vgpr_spill_count", 0) == 0, f"{r['name']} spills {r['vgpr_spill_count']} VGPRs"
        assert r.get("private_segment_fixed_size", 0) == 0, f"{r['name']} uses scratch"
