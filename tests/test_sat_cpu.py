"""CPU-side checks of the is_sat surface (R1CSShape::is_sat / is_sat_relaxed, src/r1cs/mod.rs:358-394, :430-471): the header declares the three entry points
and SP_ERR_UNSAT, both libraries export what the Python classes call, and the residual kernel is in the gfx950 code objects - every instantiation -
without a spilled VGPR or a byte of scratch. Runs without a GPU, after __graft_entry__.build(). (That the product reads no SPARTAN_* switch outside
tests/switch_registry.py is tests/test_switch_registry_cpu.py's check; is_sat adds none.)"""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from spartan2_amd import hip, host  # noqa: E402

ENTRY_POINTS = ("sp_r1cs_residual", "sp_r1cs_residual_batched", "sp_shape_is_sat")


def _header():
    return open(hip.HEADER).read()


def test_header_declares_the_entry_points_and_the_error_class():
    txt = _header()
    assert set(ENTRY_POINTS) <= set(hip.declared_symbols())
    assert re.search(r"#define\s+SP_ERR_UNSAT\s+\(-6\)", txt)
    m = re.search(r"typedef struct sp_sat_report \{(.*?)\} sp_sat_report;", txt, flags=re.S)
    assert m and [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == ["uint64_t num_failing", "uint64_t num_listed", "uint64_t first[16]"]
    # the ctypes mirror has the header's layout
    assert ctypes.sizeof(hip._SatReport) == 8 * 18 and hip._SatReport.first.offset == 16
    assert host.SP_ERR_UNSAT == -6


def test_libspartan_hip_exports_them():
    L = hip.lib()
    for n in ENTRY_POINTS:
        assert hasattr(L, n), n


def test_libspartan_host_exports_the_drivers():
    L = host.lib()
    for n in ("ss_prep_is_sat", "nnz_prep_is_sat"):
        assert hasattr(L, n), n


def test_python_surface():
    assert callable(hip.r1cs_residual) and callable(hip.Shape.is_sat) and callable(host.SpartanSNARK.is_sat) and callable(host.NeutronNovaZkSNARK.is_sat)
    ok = hip.SatReport(hip._SatReport())
    assert ok.ok and ok.reason is None and ok.num_failing == 0 and ok.first_failing == [] and ok.bad_commitment_rows == []
    raw = hip._SatReport()
    raw.num_failing, raw.num_listed = 40, 16
    for i in range(16):
        raw.first[i] = 3 * i
    r = hip.SatReport(raw, [2])
    assert not r.ok and r.reason == "R1CS is unsatisfiable" and r.first_failing == [3 * i for i in range(16)] and r.bad_commitment_rows == [2]  # takes precedence
    assert hip.SatReport(hip._SatReport(), [5]).reason == "Invalid commitment"


def test_residual_kernel_has_no_spill_and_no_scratch():
    import spill_report

    lib = os.path.join(ROOT, "spartan2_amd", "lib")
    rows = [r for r in spill_report.kernels(lib) if "k_r1cs_residual" in r["name"]]
    # <HAS_U, HAS_E>: the plain check, the two mixed forms and the relaxed check
    assert sorted(re.search(r"k_r1cs_residual<(\w+), (\w+)>", r["name"]).groups() for r in rows) == [("false", "false"), ("false", "true"), ("true", "false"), ("true", "true")]
    for r in rows:
        assert r["object"] == "capi_sparse.o"
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r
        assert r.get("group_segment_fixed_size", 0) == 0 and r["vgpr_count"] <= 128, r  # a streaming kernel: four waves a SIMD or more
