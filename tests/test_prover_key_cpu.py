"""CPU: what of the prover key's load runs without a device. The new entry points are declared, exported and bound; the flag values; the device-free
refusals; the sort kernels' constants as the kernel header, the library and the GPU test state them; the compiler's resource report of the new kernels;
no new SPARTAN_* variable, and the three SPARTAN_POLYABC_* reads still in capi_sparse.hip."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

from spartan2_amd import hip, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_SYMBOLS = ["sp_shape_from_wire_full_stages", "sp_shape_wire_sort_tile", "sp_shape_wire_sort_digit_bits", "sp_shape_compare"]
HOST_SYMBOLS = ["ss_pk_to_bytes", "ss_prover_from_bytes", "ss_prover_stages", "ss_prover_full_device_default"]
KERNELS = ["spk::k_full_filt_counts", "spk::k_full_filt_scatter", "spk::k_full_col_counts", "spk::k_full_col_place", "spk::k_full_sort_hist", "spk::k_full_sort_scatter",
           "spk::k_full_col_scatter"]


def read(path):
    with open(os.path.join(ROOT, path)) as f:
        return f.read()


def test_symbols_are_declared_exported_and_bound():
    declared = hip.declared_symbols()
    ffi = read("integration/hip_ffi.rs")
    for n in HIP_SYMBOLS:
        assert n in declared and hasattr(hip.lib(), n), n
        assert f"pub fn {n}(" in ffi, n
    for n in HOST_SYMBOLS:
        assert hasattr(host.lib(), n), n
    for name in ("from_wire", "compare", "info"):
        assert callable(getattr(hip.Shape, name))
    assert "sp_shape_from_wire_stages" in declared  # the eight fields of the row decode keep their entry point


def test_flag_values_are_pinned():
    header = read("include/spartan_hip.h")
    want = {"SP_SHAPE_WIRE_DEVICE": 1, "SP_SHAPE_WIRE_HOST": 2, "SP_SHAPE_WIRE_FULL": 4, "SP_SHAPE_WIRE_TIMED": 8, "SP_SHAPE_WIRE_FULL_DEVICE": 16}
    for name, v in want.items():
        assert re.search(rf"^#define {name} {v}$", header, flags=re.M), name
        assert f"pub const {name}: c_int = {v};" in read("integration/hip_ffi.rs"), name
    assert (hip.SHAPE_WIRE_DEVICE, hip.SHAPE_WIRE_HOST, hip.SHAPE_WIRE_FULL, hip.SHAPE_WIRE_TIMED, hip.SHAPE_WIRE_FULL_DEVICE) == (1, 2, 4, 8, 16)
    assert host.SS_PK_TRUST_DIGEST == 1 << 16 and host.SS_PK_TRUST_DIGEST > 2 * hip.SHAPE_WIRE_FULL_DEVICE  # outside the SP_SHAPE_WIRE_* range
    assert re.search(r"SS_PK_TRUST_DIGEST = 1u << 16", read("spartan2_amd/host/spartan_snark.cpp"))
    default = re.search(r"constexpr bool PK_FULL_DEVICE_DEFAULT = (true|false);", read("spartan2_amd/host/spartan_snark.cpp")).group(1)
    assert bool(host.lib().ss_prover_full_device_default()) == (default == "true")


def test_python_signatures():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(host.SpartanProver.from_bytes) == [("ctx", E), ("data", E), ("trust_digest", False), ("full_device", None), ("timed", False)]
    assert params(hip.Shape.from_wire) == [("ctx", E), ("data", E), ("device_decode", None), ("full", False), ("timed", False), ("full_device", False)]
    assert params(hip.Shape.compare) == [("self", E), ("other", E)]
    assert params(host.SpartanSNARK.pk_to_bytes) == [("self", E)]
    assert params(host.SpartanProver.prep_prove)[:5] == [("self", E), ("tape", E), ("witness", E), ("publics", E), ("is_small", True)]
    assert [n for n, _ in params(host.SpartanProver.prep_prove_batch)[:5]] == ["self", "tapes", "witnesses", "msgs", "publics"]
    for name in ("prep_prove_sha256", "prove", "prove_batch", "is_sat", "verify", "verify_bytes", "verify_batch", "verify_bytes_batch", "proof_to_bytes", "proof_layout"):
        assert getattr(host.SpartanProver, name) is getattr(host.SpartanSNARK, name), name  # shared, not restated
    with pytest.raises(TypeError):
        host.SpartanProver()


def test_device_free_refusals():
    L = host.lib()
    out = ctypes.c_void_p(1)
    buf = np.zeros(200, dtype=np.uint8)
    fake_ctx = ctypes.c_void_p(buf.ctypes.data)  # never reached: the arguments are refused first
    for ctx, b, n in ((None, hip.p8(buf), len(buf)), (fake_ctx, None, len(buf)), (fake_ctx, hip.p8(buf), 0)):
        assert L.ss_prover_from_bytes(ctx, b, ctypes.c_size_t(n), ctypes.c_uint(0), ctypes.byref(out)) == -1
        assert b"prover_from_bytes: null context, null bytes or no bytes" in L.ss_last_error() and not out.value
    assert L.ss_prover_from_bytes(fake_ctx, hip.p8(buf), ctypes.c_size_t(len(buf)), ctypes.c_uint(0), None) == -1 and b"null out" in L.ss_last_error()
    for flags in (hip.SHAPE_WIRE_DEVICE, hip.SHAPE_WIRE_HOST, hip.SHAPE_WIRE_DEVICE | host.SS_PK_TRUST_DIGEST):
        assert L.ss_prover_from_bytes(fake_ctx, hip.p8(buf), ctypes.c_size_t(len(buf)), ctypes.c_uint(flags), ctypes.byref(out)) == -1
        assert b"a prover's key holds the full shape" in L.ss_last_error() and not out.value
    for n in (1, 31, 32):  # no room for a key in front of the digest
        assert L.ss_prover_from_bytes(fake_ctx, hip.p8(buf), ctypes.c_size_t(n), ctypes.c_uint(0), ctypes.byref(out)) == -1
        assert b"unexpected end of input" in L.ss_last_error()
    with pytest.raises(hip.SpartanHipError, match="null context"):
        host.SpartanProver.from_bytes(None, bytes(100))
    L.ss_pk_to_bytes.restype = ctypes.c_long
    assert L.ss_pk_to_bytes(None, *([ctypes.c_size_t(0)] * 6), *([None] * 9), None, ctypes.c_size_t(0)) < 0 and b"null key" in L.ss_last_error()
    where = ctypes.create_string_buffer(64)
    H = hip.lib()
    for args in ((None, fake_ctx, fake_ctx, where, 64), (fake_ctx, None, fake_ctx, where, 64), (fake_ctx, fake_ctx, None, where, 64), (fake_ctx, fake_ctx, fake_ctx, None, 64),
                 (fake_ctx, fake_ctx, fake_ctx, where, 0)):
        assert H.sp_shape_compare(*args[:4], ctypes.c_size_t(args[4])) == -1 and b"sp_shape_compare: null argument" in H.sp_last_error()
    out8 = (ctypes.c_double * 8)(*([7.0] * 8))
    H.sp_shape_from_wire_full_stages(out8)  # no call on this thread yet: zeros
    assert list(out8) == [0.0] * 8
    L.ss_prover_stages(out8)
    assert out8[5] >= 0.0


def test_sort_constants_are_the_headers():
    src = read("spartan2_amd/csrc/kernels_wire_full.hpp")
    val = {n: int(v) for n, v in re.findall(r"constexpr unsigned (FULL_[A-Z_]+) = (\d+);", src)}
    c = hip.wire_full_constants()
    assert c["sort_tile"] == val["FULL_SORT_TILE"] == hip.wire_decode_constants()["block"] * val["FULL_SORT_ITEMS"]
    assert c["digit_bits"] == val["FULL_SORT_BITS"] and val["FULL_SORT_BINS"] == 1 << val["FULL_SORT_BITS"]
    gpu = read("tests/test_gpu_prover_key.py")  # (read as text: no GPU test module is imported here)
    assert f"FULL_SORT_TILE = {c['sort_tile']}\n" in gpu and f"FULL_SORT_BITS = {c['digit_bits']}\n" in gpu
    assert f"WIRE_SCAN_TILE = {hip.wire_decode_constants()['scan_tile']}\n" in gpu
    m = re.search(r"constexpr unsigned LONG_COLUMN = (\d+);", read("spartan2_amd/csrc/capi_sparse.hip"))
    assert f"LONG_COLUMN = {m.group(1)} " in gpu


def test_new_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report

    rows = spill_report.kernels(os.path.join(ROOT, "spartan2_amd", "lib"))
    seen = {}
    for r in rows:
        name = re.sub(r"[<(].*$", "", re.sub(r"^void ", "", r["name"]))
        if name in KERNELS:
            seen.setdefault(name, []).append(r)
    assert sorted(seen) == sorted(KERNELS), f"not in the resource report: {sorted(set(KERNELS) - set(seen))}"
    assert len(seen["spk::k_full_sort_hist"]) == 2 and len(seen["spk::k_full_sort_scatter"]) == 2  # the first pass and the later ones
    for name, rs in seen.items():
        for r in rs:
            assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (name, r)
    profile = read("profiles/prover_key.md")
    for name in KERNELS:
        assert name.split("::")[1] in profile, f"{name} is not listed in profiles/prover_key.md"


def test_no_new_environment_variable():
    import switch_registry as reg
    from test_switch_registry_cpu import switches_read

    found = switches_read()
    assert set(found) <= set(reg.SWITCHES)
    for name in ("POLYABC_ORDER", "POLYABC_LAYOUT", "POLYABC_WINDOW"):  # read where the registry says, and nowhere else
        assert found[name] == ["spartan2_amd/csrc/capi_sparse.hip"], name
        assert reg.SWITCHES[name].source.startswith("spartan2_amd/csrc/capi_sparse.hip")
        assert read("spartan2_amd/csrc/capi_sparse.hip").count(f'getenv("SPARTAN_{name}")') == 1
    assert "getenv" not in read("spartan2_amd/csrc/kernels_wire_full.hpp")
    for path, names in (("spartan2_amd/csrc/capi_sparse.hip", ("sp_shape_from_wire", "wire_decode_device", "wire_full_device", "sort_columns_by_key", "sp_shape_compare")),
                        ("spartan2_amd/host/spartan_snark.cpp", ("key_from_bytes", "prover_from_bytes", "pk_to_bytes", "ss_prover_from_bytes", "ss_pk_to_bytes"))):
        src = read(path)
        for fn in names:  # the body of each function, up to the next closing brace at column 0
            m = re.search(rf"^[\w:\*<> ]+\b{fn}\([^;]*?\) \{{\n(.*?)^\}}", src, flags=re.S | re.M)
            assert m, (path, fn)
            assert "getenv" not in m.group(1) and "SPARTAN_" not in m.group(1), (path, fn)
