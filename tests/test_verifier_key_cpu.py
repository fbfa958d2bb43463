"""CPU: what of the verifier key's load runs without a device. The new entry points are declared, exported and bound; sp_unwire_hyrax_key inverts
pywire.Writer.hyrax_key on the oracle's generators and refuses what concerns it; the digest hashed from slices of a key's bytes is the oracle's; the
device-free refusals; the decode kernels' block constants as the header, the library and the GPU test state them; the compiler's resource report of the
new kernels; no new SPARTAN_* variable."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

import oracle_lib as ol
import pywire
from spartan2_amd import frontend, hip, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_SYMBOLS = ["sp_unwire_hyrax_key", "sp_shape_from_wire", "sp_shape_from_wire_stages", "sp_shape_wire_block", "sp_shape_wire_scan_tile",
               "sp_shape_wire_device_default", "sp_vk_digest_from_wire"]
HOST_SYMBOLS = ["ss_vk_to_bytes", "ss_verifier_from_bytes", "ss_verifier_free"]
KERNELS = ["spk::k_wire_entries", "spk::k_wire_row_counts", "spk::k_wire_scan_reduce", "spk::k_wire_scan_blocks", "spk::k_wire_scan_add", "spk::k_wire_scatter"]


def test_symbols_are_declared_exported_and_bound():
    declared = hip.declared_symbols()
    for n in HIP_SYMBOLS:
        assert n in declared and hasattr(hip.lib(), n), n
    for n in HOST_SYMBOLS:
        assert hasattr(host.lib(), n), n
    with open(os.path.join(ROOT, "integration", "hip_ffi.rs")) as f:
        ffi = f.read()
    for n in HIP_SYMBOLS:
        assert f"pub fn {n}(" in ffi, n
    for flag in ("SP_SHAPE_WIRE_DEVICE", "SP_SHAPE_WIRE_HOST", "SP_SHAPE_WIRE_FULL"):
        assert f"pub const {flag}: c_int" in ffi
    assert (hip.SHAPE_WIRE_DEVICE, hip.SHAPE_WIRE_HOST, hip.SHAPE_WIRE_FULL) == (1, 2, 4)


def test_python_signatures():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    assert params(hip.Shape.from_wire)[:4] == [("ctx", inspect.Parameter.empty), ("data", inspect.Parameter.empty), ("device_decode", None), ("full", False)]
    assert params(host.SpartanVerifier.from_bytes)[:3] == [("ctx", inspect.Parameter.empty), ("data", inspect.Parameter.empty), ("device_decode", None)]
    assert params(host.SpartanSNARK.vk_to_bytes) == [("self", inspect.Parameter.empty)]
    for name in ("verify", "verify_bytes", "verify_batch", "verify_bytes_batch"):
        assert inspect.signature(getattr(host.SpartanVerifier, name)) == inspect.signature(getattr(host.SpartanSNARK, name)), name
    assert callable(host.SpartanVerifier.close)
    with pytest.raises(TypeError):
        host.SpartanVerifier()


@pytest.fixture(scope="module")
def key():
    osp = ol.OracleSpartan(frontend.cubic_circuit())
    return osp, osp.vk_bytes(), osp.export_keys()


def test_unwire_hyrax_key_round_trip_and_refusals(key):
    osp, vk, (ck, h, ck_s, h_s, dig) = key
    for gens, hh in ((ck, h), (ck_s.reshape(1, 8), h_s), (ck[:5], h_s)):
        w = pywire.Writer()
        w.hyrax_key(gens, hh)
        got_ck, got_h = hip.unwire_hyrax_key(w.bytes())
        assert (got_ck == gens).all() and (got_h == hh).all()
    w = pywire.Writer()
    w.hyrax_key(ck[:4], h)
    good = w.bytes()
    assert good == (4).to_bytes(8, "little") * 2 + vk[16:16 + 64 * 4] + vk[16 + 64 * 2048:16 + 64 * 2048 + 96]  # (the oracle's bytes of the same points)

    def refused(blob, match):
        with pytest.raises(hip.SpartanHipError, match=match):
            hip.unwire_hyrax_key(blob)

    refused((3).to_bytes(8, "little") + good[8:], "generators for num_cols")  # num_cols != the generator count, both ways
    refused(good[:8] + (3).to_bytes(8, "little") + good[16:], "generators for num_cols")
    for at in (16 + 32, 16 + 64 * 3, 16 + 64 * 4 + 32):  # y of the first generator, x of the last, y of h
        bad = bytearray(good)
        bad[at] ^= 1
        refused(bytes(bad), "not on the curve")
    bad = bytearray(good)
    bad[16:48] = pywire.P_BASE.to_bytes(32, "little")  # x = p
    refused(bytes(bad), "non-canonical coordinate")
    for cut in (0, 7, 8, 15, 16, 16 + 64 * 4 - 1, 16 + 64 * 4, len(good) - 1):
        refused(good[:cut], "unexpected end of input|length prefix exceeds the input")
    refused(good[:8] + (1 << 62).to_bytes(8, "little") + good[16:], "generators for num_cols|length prefix exceeds the input")
    refused(good + b"\0", "trailing bytes")
    # the generator buffer's capacity is checked, and the sizing call consumes nothing
    buf = np.frombuffer(good, dtype=np.uint8)
    r = ctypes.c_void_p()
    L = hip.lib()
    L.sp_unwire_left.restype = ctypes.c_size_t
    assert L.sp_unwire_new(hip.p8(buf), ctypes.c_size_t(len(buf)), ctypes.byref(r)) == 0
    n = ctypes.c_size_t(0)
    assert L.sp_unwire_hyrax_key(r, None, ctypes.c_size_t(0), ctypes.byref(n), None) == 0 and n.value == 4 and L.sp_unwire_left(r) == len(good)
    out, hh = np.zeros((4, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    assert L.sp_unwire_hyrax_key(r, hip.p64(out), ctypes.c_size_t(3), ctypes.byref(n), hip.p64(hh)) == -1 and b"buffer too small" in L.sp_last_error()
    assert L.sp_unwire_left(r) == len(good)
    assert L.sp_unwire_hyrax_key(r, hip.p64(out), ctypes.c_size_t(4), ctypes.byref(n), hip.p64(hh)) == 0 and L.sp_unwire_left(r) == 0
    L.sp_unwire_free(r)


@pytest.mark.parametrize("which", ["cubic", "synthetic_segments"])
def test_digest_from_slices_is_the_oracles(which, key):
    if which == "cubic":
        osp, vk, keys = key
    else:
        osp = ol.OracleSpartan(frontend.synthetic_circuit(60, 9, num_public=3, shared_permille=200, precommitted_permille=500))
        vk, keys = osp.vk_bytes(), osp.export_keys()
    assert hip.vk_digest_from_wire(vk) == keys[4].tobytes()
    flipped = bytearray(vk)
    flipped[-9] ^= 1  # the last row pointer of C: every byte of the key is under the hash
    assert hip.vk_digest_from_wire(bytes(flipped)) != keys[4].tobytes()
    for blob, match in ((vk + b"\0", "trailing bytes"), (vk[:-1], "unexpected end of input|length prefix exceeds"), (vk[:100], "unexpected end of input|length prefix exceeds"),
                        (b"", "null argument")):
        with pytest.raises(hip.SpartanHipError, match=match):
            hip.vk_digest_from_wire(blob)


def test_device_free_refusals(key):
    osp, vk, _ = key
    L = host.lib()
    out = ctypes.c_void_p(1)
    buf = np.frombuffer(vk, dtype=np.uint8)
    fake_ctx = ctypes.c_void_p(buf.ctypes.data)  # never reached: the bytes are refused first
    for ctx, b, n in ((None, hip.p8(buf), len(buf)), (fake_ctx, None, len(buf)), (fake_ctx, hip.p8(buf), 0)):
        assert L.ss_verifier_from_bytes(ctx, b, ctypes.c_size_t(n), ctypes.c_uint(0), ctypes.byref(out)) == -1
        assert b"null context, null bytes or no bytes" in L.ss_last_error() and not out.value
    with pytest.raises(hip.SpartanHipError, match="null context"):
        host.SpartanVerifier.from_bytes(None, vk)
    with pytest.raises(hip.SpartanHipError, match="null argument"):
        hip.Shape.from_wire(None, vk)
    L.ss_verifier_free(None)  # like free(NULL)


def test_block_constants_are_the_headers():
    with open(os.path.join(ROOT, "spartan2_amd", "csrc", "kernels_wire_decode.hpp")) as f:
        src = f.read()
    val = {n: int(v) for n, v in re.findall(r"constexpr unsigned (WIRE_[A-Z_]+) = (\d+);", src)}
    c = hip.wire_decode_constants()
    assert c["block"] == val["WIRE_BLOCK"] and c["scan_tile"] == val["WIRE_SCAN_TILE"] == val["WIRE_BLOCK"] * val["WIRE_SCAN_ITEMS"]
    assert val["WIRE_BLOCK"] % 64 == 0
    with open(os.path.join(ROOT, "tests", "test_gpu_verifier_key.py")) as f:  # (read as text: no GPU test module is imported here)
        gpu = f.read()
    assert f"WIRE_BLOCK = {c['block']}\n" in gpu and f"WIRE_SCAN_TILE = {c['scan_tile']}\n" in gpu
    m = re.search(r"constexpr unsigned SPMV_LONG_ROW = (\d+);", open(os.path.join(ROOT, "spartan2_amd", "csrc", "capi_sparse.hip")).read())
    assert f"SPMV_LONG_ROW = {m.group(1)} " in gpu
    default = re.search(r"constexpr bool WIRE_DEVICE_DEFAULT = (true|false);", open(os.path.join(ROOT, "spartan2_amd", "csrc", "capi_sparse.hip")).read()).group(1)
    assert c["device_default"] == (default == "true")


def test_new_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report

    rows = spill_report.kernels(os.path.join(ROOT, "spartan2_amd", "lib"))
    seen = {}
    for r in rows:
        name = re.sub(r"[<(].*$", "", re.sub(r"^void ", "", r["name"]))
        if name in KERNELS:
            seen[name] = r
    assert sorted(seen) == sorted(KERNELS), f"not in the resource report: {sorted(set(KERNELS) - set(seen))}"
    for name, r in seen.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (name, r)


def test_no_new_environment_variable():
    import switch_registry as reg
    from test_switch_registry_cpu import switches_read

    assert set(switches_read()) <= set(reg.SWITCHES)
    for path in ("spartan2_amd/csrc/kernels_wire_decode.hpp",):
        assert "getenv" not in open(os.path.join(ROOT, path)).read()
    for path, names in (("spartan2_amd/csrc/capi_sparse.hip", ("sp_shape_from_wire", "wire_decode_device", "wire_decode_host", "wire_parse_shape")),
                        ("spartan2_amd/host/spartan_snark.cpp", ("verifier_from_bytes", "vk_to_bytes")), ("spartan2_amd/csrc/capi_wire.hip", ("sp_unwire_hyrax_key", "sp_vk_digest_from_wire"))):
        src = open(os.path.join(ROOT, path)).read()
        for fn in names:  # the body of each new function, up to the next one at column 0
            m = re.search(rf"^[\w:\*<> ]+\b{fn}\([^;]*?\) \{{\n(.*?)^\}}", src, flags=re.S | re.M)
            assert m, (path, fn)
            assert "getenv" not in m.group(1) and "SPARTAN_" not in m.group(1), (path, fn)
