"""CPU: the pieces of NeutronNovaZkSNARK.verify_batch exist where a caller looks for them - sp_msm_shared_weights_grouped and its twins declared in
include/spartan_hip.h and exported by libspartan_hip.so, nnz_verify_batch / nnz_verify_bytes_batch (and their _opts forms) exported by
libspartan_host.so, the Python methods with the driver's flag values - the grouped call refuses null arguments before it touches a device, its bucket
kernel is in capi_group.o without a spilled VGPR (tools/spill_report.py on spartan2_amd/lib/*.o) beside the kernels it reuses, which are still there once each.
Runs without a GPU."""
import ctypes
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spill_report  # noqa: E402

from spartan2_amd import hip, host  # noqa: E402

SYMBOLS = ("sp_msm_shared_weights_grouped", "sp_msm_shared_weights_grouped_aux", "sp_msm_shared_weights_grouped_opts", "sp_msm_shared_weights_group_rows")
HOST_SYMBOLS = ("nnz_verify_batch", "nnz_verify_batch_opts", "nnz_verify_bytes_batch", "nnz_verify_bytes_batch_opts")
DRIVER = os.path.join(ROOT, "spartan2_amd", "host", "neutronnova_zk.cpp")
REUSED = ("k_msm_sort", "k_fold_sign", "k_to_canonical", "k_msm_window_reduce_seg", "k_msm_horner_rows", "k_msm_bucket_sum_shared")


def test_symbols_declared_and_exported():
    declared = hip.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/spartan_hip.h"
        assert hasattr(hip.lib(), name), f"libspartan_hip.so does not export {name}"
    assert hip.msm_shared_weights_group_rows() == 512  # config 5's own sp_msm_shared_weights call: the bucket workspace of a launch
    for name in HOST_SYMBOLS:
        assert hasattr(host.lib(), name), f"libspartan_host.so does not export {name}"
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    for name in SYMBOLS:
        assert re.search(r"\bpub fn " + name + r"\(", ffi), f"{name} is not in integration/hip_ffi.rs"


def test_python_surface():
    assert callable(hip.msm_shared_weights_grouped)
    for name in ("verify_batch", "verify_bytes_batch"):
        params = inspect.signature(getattr(host.NeutronNovaZkSNARK, name)).parameters
        assert list(params)[:4] == ["self", "proofs" if name == "verify_batch" else "blobs", "seed", "info"]
        assert params["seed"].default is None and params["info"].default is False
    src = open(DRIVER).read()
    for name, value in (("NNZ_VERIFY_BATCH_PER_PROOF", 1), ("NNZ_VERIFY_BATCH_SHARED", 2)):
        m = re.search(r"\b" + name + r"\s*=\s*(\d+)\s*[,}\n ]", src)
        assert m and int(m.group(1)) == value == getattr(host, name), name


def test_refusals_that_need_no_device():
    L = hip.lib()
    sz = ctypes.c_size_t
    dummy = ctypes.c_void_p(8)  # never dereferenced: the null checks come first
    for f in (L.sp_msm_shared_weights_grouped, L.sp_msm_shared_weights_grouped_aux):
        for c, w, b, o in ((None, dummy, dummy, dummy), (dummy, None, dummy, dummy), (dummy, dummy, None, dummy), (dummy, dummy, dummy, None)):
            assert f(c, w, sz(4), b, sz(8), sz(8), o) == -1
            assert b"msm_shared_weights_grouped" in L.sp_last_error()
    for c, w, b, o, flags in ((None, dummy, dummy, dummy, 0), (dummy, dummy, dummy, None, 1), (dummy, dummy, dummy, dummy, 3)):  # flags: 0, 1 and 2 only
        assert L.sp_msm_shared_weights_grouped_opts(c, w, sz(4), b, sz(8), sz(8), o, ctypes.c_uint(flags)) == -1
        assert b"msm_shared_weights_grouped" in L.sp_last_error()
    assert (hip.MSM_GROUPED_HORNER_HOST, hip.MSM_GROUPED_HORNER_DEVICE) == (1, 2)
    H = host.lib()
    H.ss_last_error.restype = ctypes.c_char_p
    codes = (ctypes.c_int * 2)()
    lens = (sz * 2)(0, 0)
    ptrs = (ctypes.c_void_p * 2)()
    for f in (H.nnz_verify_batch, H.nnz_verify_bytes_batch):
        for pk, items, ln, cd in ((None, ptrs, lens, codes), (dummy, None, lens, codes), (dummy, ptrs, None, codes), (dummy, ptrs, lens, None)):
            assert f(pk, items, ln, sz(2), None, cd, None) == -1
            assert b"null argument" in H.ss_last_error()


def kernels_by_base():
    lib = os.path.join(ROOT, "spartan2_amd", "lib")
    assert os.path.isdir(lib) and [f for f in os.listdir(lib) if f.endswith(".o")], "spartan2_amd/lib/*.o not built (run __graft_entry__.build())"
    by_base = {}
    for r in spill_report.kernels(lib):
        base = re.sub(r"[<(].*$", "", re.sub(r"^void ", "", r["name"]))
        by_base.setdefault(base, []).append(r)
    return by_base


def test_grouped_bucket_kernel_is_built_without_vgpr_spills():
    by_base = kernels_by_base()
    got = by_base.get("spk::k_msm_bucket_sum_grouped")
    assert got and len(got) == 1, "k_msm_bucket_sum_grouped is not in the code objects of spartan2_amd/lib/*.o"
    assert got[0]["object"] == "capi_group.o"
    assert got[0].get("vgpr_spill_count", 0) == 0, f"{got[0]['name']} spills {got[0]['vgpr_spill_count']} VGPRs"
    for name in REUSED:  # still there, once each
        same = [r for r in by_base.get("spk::" + name, []) if r["object"] == "capi_group.o"]
        assert len(same) == 1, (name, [r["name"] for r in same])
