"""CPU: NeutronNovaZkSNARK.prove_batch exists where a caller looks for it - sp_sumcheck_cubic_outer_pow_batched_lockstep / sp_sumcheck_quad_batched_lockstep
declared in include/spartan_hip.h, exported by libspartan_hip.so and bound in spartan2_amd/hip.py and integration/hip_ffi.rs, nnz_prove_batch /
nnz_prove_batch_opts exported by libspartan_host.so and bound in spartan2_amd/host.py with the driver's flag values - refuses count 0 and null arguments
without a device, and its new kernels are in the code objects once each without a spilled VGPR or scratch (tools/spill_report.py on
spartan2_amd/lib/*.o). Runs without a GPU."""
import ctypes
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spill_report  # noqa: E402

from spartan2_amd import hip, host  # noqa: E402

SP_SYMBOLS = ("sp_sumcheck_cubic_outer_pow_batched_lockstep", "sp_sumcheck_quad_batched_lockstep")
NNZ_SYMBOLS = ("nnz_prove_batch", "nnz_prove_batch_opts")
KERNELS = ("k_ls_eval_cubic_pow<false>", "k_ls_eval_cubic_pow<true>", "k_ls_bind_eval_cubic_pow<false>", "k_ls_bind_eval_cubic_pow<true>")


def test_symbols_declared_exported_and_bound():
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    for name in SP_SYMBOLS:
        assert name in hip.declared_symbols(), f"{name} is not declared in include/spartan_hip.h"
        assert hasattr(hip.lib(), name), f"libspartan_hip.so does not export {name}"
        assert f"def {name[3:]}(" in open(hip.__file__).read(), f"{name} is not bound in spartan2_amd/hip.py"
        assert f"fn {name}(" in ffi
    header = open(hip.HEADER).read()
    assert "#define SP_LOCKSTEP_PAIRS_MAX (SP_LOCKSTEP_MAX / 2)" in header
    assert hip.LOCKSTEP_PAIRS_MAX == hip.LOCKSTEP_MAX // 2 == 32
    for name in NNZ_SYMBOLS:
        assert hasattr(host.lib(), name), f"libspartan_host.so does not export {name}"
    src = inspect.getsource(host.NeutronNovaZkSNARK.prove_batch)
    assert "nnz_prove_batch_opts" in src
    sig = inspect.signature(host.NeutronNovaZkSNARK.prove_batch).parameters
    assert sig["states"].default is None and sig["per_proof"].default is None
    assert (host.NNZ_BATCH_PER_PROOF, host.NNZ_BATCH_LOCKSTEP) == (1, 2)
    cpp = open(os.path.join(ROOT, "spartan2_amd", "host", "neutronnova_zk.cpp")).read()
    assert "NNZ_BATCH_PER_PROOF = 1, NNZ_BATCH_LOCKSTEP = 2" in cpp
    assert len(host.NN_BATCH_PROVE_PHASES) == 10  # the doubles nnz_prove_batch_opts writes


def test_refusals_that_need_no_device():
    """count 0 and null arguments are refused before a context, a table or a key is touched"""
    L, H = hip._batched_lockstep_lib(), host.lib()
    sz = ctypes.c_size_t
    one = (ctypes.c_void_p * 1)()  # a one-entry array holding NULL: never dereferenced further than that
    words = (ctypes.c_uint64 * 16)()
    w = ctypes.cast(words, hip.c_u64p)
    cb, users = hip._pair_hooks([lambda rnd, cs, cc: 0])
    ctx = ctypes.c_void_p(8)  # never dereferenced by a refusal
    # ctx, count, num_rounds, pow_left, pow_right, A_step .. C_core, t_out_step, start_round, hook, users, out_r
    cubic = [ctx, sz(1), sz(2), one, one, one, one, one, one, one, one, w, sz(0), cb, users, w]
    # ctx, count, claims, num_rounds, A0, A1, B0, B1, start_round, hook, users, out_r, out_final
    quad = [ctx, sz(1), w, sz(2), one, one, one, one, sz(0), cb, users, w, w]
    for fn, args, count_at, ptrs, hook_at in ((L.sp_sumcheck_cubic_outer_pow_batched_lockstep, cubic, 1, (0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14, 15), 13),
                                              (L.sp_sumcheck_quad_batched_lockstep, quad, 1, (0, 2, 4, 5, 6, 7, 10, 11, 12), 9)):
        for count in (0, hip.LOCKSTEP_PAIRS_MAX + 1):
            a = list(args)
            a[count_at] = sz(count)
            assert fn(*a) == -1
            assert b"(lockstep): count must be 1 .. SP_LOCKSTEP_PAIRS_MAX" in L.sp_last_error()
        for i in ptrs:  # each pointer argument in turn
            a = list(args)
            a[i] = None
            assert fn(*a) == -1, i
            assert b"(lockstep): null argument" in L.sp_last_error(), i
        a = list(args)
        a[hook_at] = hip.ROUND_HOOK()
        assert fn(*a) == -1
        assert b"(lockstep): null hook" in L.sp_last_error()
        assert fn(*args) == -1  # every array entry is NULL
        assert b"(lockstep): null table, pair 0" in L.sp_last_error()
    u = ctypes.c_uint(0)
    ms = (ctypes.c_double * 10)()
    used = (sz * 1)()
    # pk, ps, count, tapes, tape_blocks, tape_used, out_words, out_cap, phase_ms
    batch = [one, one, sz(0), one, used, used, one, sz(0), ms]
    for fn, args in ((H.nnz_prove_batch_opts, batch + [u]), (H.nnz_prove_batch, batch)):
        assert fn(*args) == -1
        assert b"prove_batch: count must be at least 1" in H.ss_last_error()
        for i in (0, 1, 3, 4, 6):  # each pointer argument that must be there (tape_used and phase_ms are optional)
            a = list(args)
            a[2], a[i] = sz(1), None
            assert fn(*a) == -1, i
            assert b"prove_batch: null argument" in H.ss_last_error(), i
        a = list(args)
        a[2] = sz(1)
        assert fn(*a) == -1  # tapes[0] is NULL
        assert b"prove_batch: proof 0: null tape or output" in H.ss_last_error()


def test_the_kernels_are_built_once_without_spills():
    lib = os.path.join(ROOT, "spartan2_amd", "lib")
    assert os.path.isdir(lib) and [f for f in os.listdir(lib) if f.endswith(".o")], "spartan2_amd/lib/*.o not built (run __graft_entry__.build())"
    txt = open(os.path.join(ROOT, "spartan2_amd", "csrc", "kernels_lockstep.hpp")).read()
    for base in ("k_ls_eval_cubic_pow", "k_ls_bind_eval_cubic_pow"):
        assert re.search(r"template <bool FALLBACK>\s*__global__\s+void\s+__launch_bounds__\([^)]*\)\s+" + base + r"\s*\(", txt), f"{base} is not in kernels_lockstep.hpp"
    rows = spill_report.kernels(lib)
    for want in KERNELS:
        got = [r for r in rows if re.sub(r"\(.*$", "", re.sub(r"^void ", "", r["name"])) == "spk::" + want]
        assert len(got) == 1, f"{want} is not (once) in the code objects of spartan2_amd/lib/*.o"
        r = got[0]
        assert r["object"] == "capi_lockstep.o"
        assert r.get("vgpr_spill_count", 0) == 0, f"{r['name']} spills {r['vgpr_spill_count']} VGPRs"
        assert r.get("sgpr_spill_count", 0) == 0, f"{r['name']} spills {r['sgpr_spill_count']} SGPRs"
        assert r.get("private_segment_fixed_size", 0) == 0, f"{r['name']} uses scratch"
