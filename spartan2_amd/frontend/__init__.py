"""ctypes view of the integer R1CS generators (spartan2_amd/frontend/r1cs_builder.hpp)."""
import ctypes
import os
import subprocess

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_DIR, "libsp_frontend.so")


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB, os.path.join(_DIR, "frontend_capi.cpp")])


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            build()
        L = ctypes.CDLL(_LIB)
        L.spf_sha256_circuit.restype = ctypes.c_void_p
        L.spf_synthetic_circuit.restype = ctypes.c_void_p
        L.spf_cubic_circuit.restype = ctypes.c_void_p
        L.spf_sha256_step_circuit.restype = ctypes.c_void_p
        L.spf_sha256_rest_circuit.restype = ctypes.c_void_p
        L.spf_witness.restype = ctypes.POINTER(ctypes.c_uint64)
        L.spf_publics.restype = ctypes.POINTER(ctypes.c_uint64)
        L.spf_last_error.restype = ctypes.c_char_p
        L.spf_sha256_witness_plan.restype = ctypes.c_void_p
        L.spf_sha256_step_witness_plan.restype = ctypes.c_void_p
        L.spf_sha256_plan_descriptors.restype = ctypes.POINTER(ctypes.c_uint32)
        L.spf_sha256_plan_block_starts.restype = ctypes.POINTER(ctypes.c_uint32)
        _lib = L
    return _lib


class R1CSInstanceInt:
    """Integer R1CS + satisfying assignment; the arguments of SplitR1CSShape::new (src/r1cs/mod.rs:810-820)."""

    def __init__(self, handle):
        if not handle:
            raise RuntimeError(lib().spf_last_error().decode())
        self._h = ctypes.c_void_p(handle)
        d = (ctypes.c_uint64 * 9)()
        lib().spf_dims(self._h, d)
        (self.num_cons, self.num_shared, self.num_precommitted, self.num_rest, self.num_public, self.num_challenges, nnzA, nnzB, nnzC) = [int(x) for x in d]
        self.num_aux = self.num_shared + self.num_precommitted + self.num_rest
        st = (ctypes.c_uint64 * 2)()
        lib().spf_multieq_stats(self._h, st)
        # SHA-256 circuits: the constraint count of the reference's synthesizer, whose MultiEq packs the additions' equality rows (r1cs_builder.hpp
        # MultiEqSim); this generator emits them one per addition (int64 coefficients)
        self.addmany_rows, self.multieq_rows = int(st[0]), int(st[1])
        self.num_cons_bellpepper = self.num_cons - (self.addmany_rows - self.multieq_rows)
        self.csr = []
        for which, nnz in enumerate((nnzA, nnzB, nnzC)):
            data = ctypes.POINTER(ctypes.c_int64)()
            idx = ctypes.POINTER(ctypes.c_uint32)()
            ptr = ctypes.POINTER(ctypes.c_uint64)()
            lib().spf_csr(self._h, which, ctypes.byref(data), ctypes.byref(idx), ctypes.byref(ptr))
            d = np.ctypeslib.as_array(data, (nnz,)).copy() if nnz else np.zeros(0, dtype=np.int64)
            i = np.ctypeslib.as_array(idx, (nnz,)).copy() if nnz else np.zeros(0, dtype=np.uint32)
            self.csr.append((d, i, np.ctypeslib.as_array(ptr, (self.num_cons + 1,)).copy()))
        self.witness = np.ctypeslib.as_array(lib().spf_witness(self._h), (self.num_aux,)).copy() if self.num_aux else np.zeros(0, dtype=np.uint64)
        self.publics = np.ctypeslib.as_array(lib().spf_publics(self._h), (self.num_public,)).copy() if self.num_public else np.zeros(0, dtype=np.uint64)
        lib().spf_free(self._h)
        self._h = None


def sha256_circuit(preimage: bytes) -> R1CSInstanceInt:
    """Sha256Circuit of benches/sha256_spartan.rs:36-152 for the given preimage."""
    return R1CSInstanceInt(lib().spf_sha256_circuit(preimage, ctypes.c_size_t(len(preimage))))


def synthetic_circuit(n_groups: int, seed: int, num_public: int = 4, shared_permille: int = 0, precommitted_permille: int = 1000,
                      witness_seed: int = 0) -> R1CSInstanceInt:
    """Seeded SHA-like circuit; the permille arguments cut the aux list into shared | precommitted | rest segments.
    witness_seed != 0: same matrices, a different satisfying assignment."""
    return R1CSInstanceInt(lib().spf_synthetic_circuit(ctypes.c_size_t(n_groups), ctypes.c_uint64(seed), ctypes.c_size_t(num_public),
                                                       ctypes.c_uint(shared_permille), ctypes.c_uint(precommitted_permille), ctypes.c_uint64(witness_seed)))


def cubic_circuit() -> R1CSInstanceInt:
    """CubicCircuit of the reference's own end-to-end test (src/spartan.rs:587-651): rest-only, public output 15."""
    return R1CSInstanceInt(lib().spf_cubic_circuit())


def sha256_step_circuit(block: bytes) -> R1CSInstanceInt:
    """Sha256StepCircuit (benches/sha256_neutronnova.rs:49-133) on a 64-byte block: one compression with the constant IV, x = 0 inputized.
    The bench's CoreCircuit (:139-183) is the same shape on bytes(64)."""
    assert len(block) == 64
    return R1CSInstanceInt(lib().spf_sha256_step_circuit(bytes(block)))


def sha256_rest_circuit(preimage: bytes) -> R1CSInstanceInt:
    """Sha256Circuit of the reference's NeutronNova test (src/neutronnova_zk.rs:2357-2418): the whole circuit in synthesize, i.e. REST variables only;
    preimage bits LSB first per byte, x = 0 inputized."""
    return R1CSInstanceInt(lib().spf_sha256_rest_circuit(bytes(preimage), ctypes.c_size_t(len(preimage))))


class Sha256WitnessPlan:
    """For every aux variable of a SHA-256 circuit structure, the bit of its block's native compression trace that it equals
    (sha256_witness_plan.hpp): `descriptors` (n_aux,) uint32 = slot | bit << 11 | invert << 17, `block_starts` (n_blocks + 1,), the first `n_pre`
    variables being the preimage bits (512 per block). One plan serves every message of `msg_len` bytes."""

    def __init__(self, handle):
        if not handle:
            raise RuntimeError(lib().spf_last_error().decode())
        self._h = ctypes.c_void_p(handle)
        d = (ctypes.c_uint64 * 6)()
        lib().spf_sha256_plan_dims(self._h, d)
        self.msg_len, padded, self.n_aux, self.n_pre, self.n_blocks, self.trace_slots = [int(x) for x in d]
        self.padded = bool(padded)
        self.descriptors = np.ctypeslib.as_array(lib().spf_sha256_plan_descriptors(self._h), (self.n_aux,)).copy()
        self.block_starts = np.ctypeslib.as_array(lib().spf_sha256_plan_block_starts(self._h), (self.n_blocks + 1,)).copy()

    def eval(self, msg: bytes, with_digest=False):
        """The witness (n_aux,) uint64 of the plan's circuit for `msg`: native compressions -> trace -> bits, no circuit synthesis."""
        if len(msg) != self.msg_len:
            raise ValueError(f"this plan serves messages of {self.msg_len} bytes, got {len(msg)}")
        out = np.zeros(self.n_aux, dtype=np.uint64)
        dig = np.zeros(32, dtype=np.uint8)
        if lib().spf_sha256_plan_eval(self._h, bytes(msg), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), dig.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) != 0:
            raise RuntimeError(lib().spf_last_error().decode())
        return (out, dig.tobytes()) if with_digest else out

    def close(self):
        if self._h:
            lib().spf_sha256_plan_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sha256_witness_plan(msg_len: int) -> Sha256WitnessPlan:
    """Plan for sha256_circuit(msg) with len(msg) == msg_len >= 1 (the circuit's structure depends only on the length)."""
    return Sha256WitnessPlan(lib().spf_sha256_witness_plan(ctypes.c_size_t(msg_len)))


def sha256_step_witness_plan() -> Sha256WitnessPlan:
    """Plan for sha256_step_circuit(block) (and the core circuit: the same shape on bytes(64))."""
    return Sha256WitnessPlan(lib().spf_sha256_step_witness_plan())
