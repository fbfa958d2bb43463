"""verify_batch without a GPU: the new entry points are declared, exported and bound at every layer (header, both libraries, Python, the Rust FFI file)."""
import ctypes
import inspect
import os
import re

from spartan2_amd import hip, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_declares_and_exports_the_entry_point():
    assert "sp_shape_matrix_evals_batched" in hip.declared_symbols()
    assert hasattr(hip.lib(), "sp_shape_matrix_evals_batched")
    for name in ("ss_verify_batch", "ss_verify_bytes_batch"):
        assert hasattr(host.lib(), name), name


def test_python_methods_have_the_stated_signatures():
    assert list(inspect.signature(hip.Shape.matrix_evals_batched).parameters) == ["self", "txs", "tys"]
    for name, first in (("verify_batch", "proofs"), ("verify_bytes_batch", "blobs")):
        sig = inspect.signature(getattr(host.SpartanSNARK, name))
        assert list(sig.parameters) == ["self", first, "seed", "info"], name
        assert sig.parameters["seed"].default is None and sig.parameters["info"].default is False
    assert [n for n, _ in host.VerifyBatchInfo._fields_][:3] == ["matrix_chunks", "opening_batched_ok", "fallback_proofs"]
    assert ctypes.sizeof(host.VerifyBatchInfo) == 32


def test_chunk_getter_is_the_kernels_constant():
    assert "sp_shape_matrix_evals_chunk" in hip.declared_symbols()
    src = open(os.path.join(ROOT, "spartan2_amd", "csrc", "kernels_mateval.hpp")).read()
    assert int(re.search(r"constexpr int MATEVAL_KC = (\d+);", src).group(1)) == hip.matrix_evals_chunk()


def test_rust_ffi_names_the_entry_point():
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    assert re.search(r"pub fn sp_shape_matrix_evals_batched\(", ffi)
    assert re.search(r"pub fn sp_shape_matrix_evals_chunk\(", ffi)
