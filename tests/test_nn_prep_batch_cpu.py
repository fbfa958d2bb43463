"""CPU: the one-pass NeutronNova prep_prove exists where a caller looks for it - sp_nifs_layers_batch / sp_nifs_layers_chunk declared in
include/spartan_hip.h, exported by libspartan_hip.so and bound in spartan2_amd/hip.py beside sp_hyrax_commit_batch, the four nnz_prep_prove*_batch* entry
points exported by libspartan_host.so and bound in spartan2_amd/host.py - refuses count 0 and null arguments without a device, and its kernel is in the
code objects once without a spilled VGPR or scratch (tools/spill_report.py on spartan2_amd/lib/*.o). Runs without a GPU."""
import ctypes
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spill_report  # noqa: E402

from spartan2_amd import hip, host  # noqa: E402

SP_SYMBOLS = ("sp_nifs_layers_batch", "sp_nifs_layers_chunk", "sp_hyrax_commit_batch")
NNZ_SYMBOLS = ("nnz_prep_prove_batch", "nnz_prep_prove_batch_opts", "nnz_prep_prove_sha256_batch", "nnz_prep_prove_sha256_batch_opts")


def test_symbols_declared_exported_and_bound():
    for name in SP_SYMBOLS:
        assert name in hip.declared_symbols(), f"{name} is not declared in include/spartan_hip.h"
        assert hasattr(hip.lib(), name), f"libspartan_hip.so does not export {name}"
        assert name in open(hip.__file__).read(), f"{name} is not bound in spartan2_amd/hip.py"
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    assert "fn sp_nifs_layers_batch(" in ffi and "fn sp_nifs_layers_chunk(" in ffi
    for name in NNZ_SYMBOLS:
        assert hasattr(host.lib(), name), f"libspartan_host.so does not export {name}"
    src = inspect.getsource(host.NeutronNovaZkSNARK.prep_prove_batch)
    assert "nnz_prep_prove_batch_opts" in src and "nnz_prep_prove_sha256_batch_opts" in src
    assert (host.NNZ_PREP_PER_STATE_COMMIT, host.NNZ_PREP_PER_STATE_LAYERS) == (1, 2)
    assert (host.NNZ_PREP_SHARED_COMMIT, host.NNZ_PREP_SHARED_LAYERS) == (4, 8)
    cpp = open(os.path.join(ROOT, "spartan2_amd", "host", "neutronnova_zk.cpp")).read()
    assert "NNZ_PREP_PER_STATE_COMMIT = 1, NNZ_PREP_PER_STATE_LAYERS = 2, NNZ_PREP_SHARED_COMMIT = 4, NNZ_PREP_SHARED_LAYERS = 8" in cpp
    assert hip.nifs_layers_chunk() >= 2
    for fn, arg in ((host.NeutronNovaZkSNARK.prove, "state"), (host.NeutronNovaZkSNARK.is_sat, "state")):
        assert inspect.signature(fn).parameters[arg].default is None


def test_refusals_that_need_no_device():
    """count 0 and null arguments are refused before a context, a shape or a key is touched"""
    L, H = hip.lib(), host.lib()
    sz = ctypes.c_size_t
    one = (ctypes.c_void_p * 1)()
    assert L.sp_nifs_layers_batch(one, one, sz(0), one, sz(2), one, one) == -1
    assert b"sp_nifs_layers_batch: count must be at least 1" in L.sp_last_error()
    for args in ((None, one, sz(1), one, sz(2), one, one), (one, None, sz(1), one, sz(2), one, one), (one, one, sz(1), None, sz(2), one, one),
                 (one, one, sz(1), one, sz(2), None, one)):
        assert L.sp_nifs_layers_batch(*args) == -1
        assert b"sp_nifs_layers_batch: null argument" in L.sp_last_error()
    assert L.sp_nifs_layers_batch(one, one, sz(1), one, sz(0), one, one) == -1
    assert b"sp_nifs_layers_batch: no instances" in L.sp_last_error()
    u = ctypes.c_uint(0)
    words = (one, sz(0), one, one, one, one, sz(1), one, one, 1, one, one, None, one, None)  # pk, count, n, step_wit, wit_len, step_pub, npub, core_wit, core_pub, ...
    sha = (one, one, sz(0), one, one, 1, one, one, None, one, None)  # pk, plan, count, blocks, n, ...
    for fn, args in ((H.nnz_prep_prove_batch_opts, words + (u,)), (H.nnz_prep_prove_batch, words), (H.nnz_prep_prove_sha256_batch_opts, sha + (u,)),
                     (H.nnz_prep_prove_sha256_batch, sha)):
        assert fn(*args) == -1
        assert b"prep_prove_batch: count must be at least 1" in H.ss_last_error()
    two = sz(2)
    for i in (0, 2, 3, 4, 5, 7, 8, 10, 11, 13):  # each pointer argument in turn
        args = list(words)
        args[1], args[i] = two, None
        assert H.nnz_prep_prove_batch_opts(*args, u) == -1, i
        assert b"prep_prove_batch: null argument" in H.ss_last_error()
    for i in (0, 1, 3, 4, 6, 7, 9):
        args = list(sha)
        args[2], args[i] = two, None
        assert H.nnz_prep_prove_sha256_batch_opts(*args, u) == -1, i
        assert b"prep_prove_batch: null argument" in H.ss_last_error()
    null_tapes = (ctypes.c_void_p * 2)()
    args = list(words)
    args[1], args[10] = two, null_tapes
    assert H.nnz_prep_prove_batch_opts(*args, u) == -1
    assert b"prep_prove_batch: state 0: null tape" in H.ss_last_error()


def test_the_kernel_is_built_once_without_spills():
    lib = os.path.join(ROOT, "spartan2_amd", "lib")
    assert os.path.isdir(lib) and [f for f in os.listdir(lib) if f.endswith(".o")], "spartan2_amd/lib/*.o not built (run __graft_entry__.build())"
    got = [r for r in spill_report.kernels(lib) if re.sub(r"[<(].*$", "", re.sub(r"^void ", "", r["name"])) == "spk::k_nifs_layers"]
    txt = open(os.path.join(ROOT, "spartan2_amd", "csrc", "kernels_nifs_layers.hpp")).read()
    assert re.search(r"__global__\s+void\s+__launch_bounds__\([^)]*\)\s+k_nifs_layers\s*\(", txt), "k_nifs_layers is not in kernels_nifs_layers.hpp"
    assert len(got) == 1, "k_nifs_layers is not (once) in the code objects of spartan2_amd/lib/*.o"
    r = got[0]
    assert r["object"] == "capi_sparse.o"  # beside the shape and the walks it shares SplitDev / acc_small with
    assert r.get("vgpr_spill_count", 0) == 0, f"{r['name']} spills {r['vgpr_spill_count']} VGPRs"
    assert r.get("private_segment_fixed_size", 0) == 0, f"{r['name']} uses scratch"
