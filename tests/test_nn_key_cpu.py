"""CPU: the bincode bytes of NeutronNovaVerifierKey / NeutronNovaProverKey written in Python (tests/pynnkey.py) and the digest walk over those serde bytes
that the loaders run (pynnkey.digest_from_bytes, restated from src/neutronnova_zk.rs:1305-1333): the digest of the bytes is the one pyvcircuit.nn_vk_digest
builds field by field in digest form and the one the oracle's setup computes; the prover key is its fields in order; keys of step counts with the same
ceil(log2) are the same bytes."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import pynnkey
import pyvcircuit
from spartan2_amd import frontend

# (steps, groups, core_groups): the shapes of tests/test_gpu_nn_keys.py - equal circuits, and the two whose equalized precommitted | rest splits differ
CASES = [(2, 8, 8), (5, 30, 30), (3, 2, 30), (3, 8, 2)]


@pytest.fixture(scope="module")
def gens():
    g = np.zeros((2049, 8), dtype=np.uint64)
    ol.lib().orc_from_label(b"ck", ctypes.c_size_t(2049), ol.p64(g))
    return g


def circuits(n, groups, core_groups):
    steps = [frontend.synthetic_circuit(groups, 0xA5, num_public=1, witness_seed=50 + i) for i in range(n)]
    return steps, frontend.synthetic_circuit(core_groups, 0xA5 + (core_groups > groups), num_public=1, witness_seed=7)


@pytest.mark.parametrize("n,groups,core_groups", CASES)
def test_digest_of_the_serde_bytes_is_the_keys_digest(gens, n, groups, core_groups):
    steps, core = circuits(n, groups, core_groups)
    vk = pynnkey.vk_bytes(steps[0], core, n, gens)
    dig = pynnkey.digest_from_bytes(vk)
    assert dig == pyvcircuit.nn_vk_digest(steps[0], core, n, gens)[0]
    assert dig == ol.OracleNeutronNova(steps, core).digest().tobytes()
    # the prover key: its fields in order, that digest at its place, the verifier's duplicates left out
    f = dict(pynnkey.vk_fields(steps[0], core, n, gens))
    assert f["vk_ee"] == f["ck"] and f["vc_vk"] == f["vc_ck"]
    pk = pynnkey.pk_bytes(steps[0], core, n, gens)
    assert pk == f["ck"] + f["S_step"] + f["S_core"] + dig + f["vc_shape"] + f["vc_shape_regular"] + f["vc_ck"]
    assert len(vk) == len(pk) - 32 + len(f["ck"]) + len(f["vc_ck"])
    off = pynnkey.offsets(pynnkey.pk_fields(steps[0], core, n, gens))
    assert pk[off["vk_digest"]:off["vk_digest"] + 32] == dig and off["end"] == len(pk)
    # a changed byte anywhere changes the digest (one byte in every field)
    voff = pynnkey.offsets(pynnkey.vk_fields(steps[0], core, n, gens))
    for name in pynnkey.VK_FIELDS:
        bad = bytearray(vk)
        bad[voff[name] + 40] ^= 1
        assert pynnkey.digest_from_bytes(bytes(bad)) != dig, name


def test_one_key_serves_every_step_count_of_one_log(gens):
    steps, core = circuits(4, 8, 2)
    k2, k3, k4, k5 = (pynnkey.vk_bytes(steps[0], core, n, gens) for n in (2, 3, 4, 5))
    assert k3 == k4 and k3 != k2 and k5 != k4
    assert pynnkey.pk_bytes(steps[0], core, 3, gens) == pynnkey.pk_bytes(steps[0], core, 4, gens)
    # 2 and 3 steps: one NIFS round more in the verifier circuit, everything else the same bytes
    f2, f3 = dict(pynnkey.vk_fields(steps[0], core, 2, gens)), dict(pynnkey.vk_fields(steps[0], core, 3, gens))
    assert {k for k in pynnkey.VK_FIELDS if f2[k] != f3[k]} == {"vc_shape", "vc_shape_regular"}
    assert ol.OracleNeutronNova(steps[:3], core).digest().tobytes() == ol.OracleNeutronNova(steps[:4], core).digest().tobytes() == pynnkey.digest_from_bytes(k3)


def test_the_walk_refuses_short_bytes(gens):
    steps, core = circuits(2, 2, 2)
    vk = pynnkey.vk_bytes(steps[0], core, 2, gens)
    off = pynnkey.offsets(pynnkey.vk_fields(steps[0], core, 2, gens))
    for cut in (0, 7, off["vk_ee"] - 1, off["S_step"] + 79, off["S_core"] - 1, off["S_core"] + 100):
        with pytest.raises(AssertionError, match="unexpected end of input"):
            pynnkey.digest_from_bytes(vk[:cut])


# ---- the library's side, as far as it runs without a device ---------------------------------------------------------------------------------------------
def test_the_librarys_digest_walk_is_the_python_one(gens):
    """nnz_vk_digest_from_bytes (the walk the loaders run on their helper thread) over the verifier key's bytes and over the prover key's, where ck stands
    for vk_ee, vc_ck for vc_vk and the stored digest is stepped over: pynnkey's digest both times, whatever the stored digest says"""
    from spartan2_amd import hip, host

    for n, groups, core_groups in CASES[2:]:
        steps, core = circuits(n, groups, core_groups)
        vk = pynnkey.vk_bytes(steps[0], core, n, gens)
        dig = pynnkey.digest_from_bytes(vk)
        assert host.nn_vk_digest_from_bytes(vk) == dig
        assert host.nn_vk_digest_from_bytes(pynnkey.pk_bytes(steps[0], core, n, gens), prover=True) == dig
        assert host.nn_vk_digest_from_bytes(pynnkey.pk_bytes(steps[0], core, n, gens, digest=bytes(32)), prover=True) == dig
        off = pynnkey.offsets(pynnkey.pk_fields(steps[0], core, n, gens))
        pk = pynnkey.pk_bytes(steps[0], core, n, gens)
        for cut in [off[k] for k in pynnkey.PK_FIELDS] + [off["S_core"] + 100, off["vc_shape"] + 50, off["end"] - 1]:
            with pytest.raises(hip.SpartanHipError, match="unexpected end of input|length prefix exceeds the input|null argument"):
                host.nn_vk_digest_from_bytes(pk[:cut], prover=True)
        for cut in (8, len(vk) // 2):
            with pytest.raises(hip.SpartanHipError, match="unexpected end of input|length prefix exceeds the input"):
                host.nn_vk_digest_from_bytes(vk[:cut])


def test_python_signatures():
    import inspect

    from spartan2_amd import host

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(host.NeutronNovaVerifier.from_bytes) == [("ctx", E), ("data", E), ("num_steps", E), ("device_decode", None), ("timed", False)]
    assert params(host.NeutronNovaProver.from_bytes) == [("ctx", E), ("data", E), ("num_steps", E), ("trust_digest", False), ("full_device", None), ("timed", False)]
    assert [n for n, _ in params(host.NeutronNovaProver.prep_prove)[:6]] == ["self", "tape", "step_witnesses", "step_publics", "core_witness", "core_publics"]
    assert params(host.NeutronNovaZkSNARK.vk_to_bytes) == params(host.NeutronNovaZkSNARK.pk_to_bytes) == [("self", E)]
    shared = ("verify", "verify_bytes", "verify_batch", "verify_bytes_batch", "proof_to_bytes", "proof_from_bytes")
    for name in shared + ("prep_prove_sha256", "prove", "prove_batch", "is_sat"):
        assert getattr(host.NeutronNovaProver, name) is getattr(host.NeutronNovaZkSNARK, name), name  # shared, not restated
    for name in shared:
        assert getattr(host.NeutronNovaVerifier, name) is getattr(host.NeutronNovaZkSNARK, name), name
    for cls in (host.NeutronNovaVerifier, host.NeutronNovaProver):
        with pytest.raises(TypeError):
            cls()


def test_device_free_refusals():
    from spartan2_amd import hip, host

    L = host.lib()
    out = ctypes.c_void_p(1)
    buf = np.zeros(200, dtype=np.uint8)
    fake_ctx = ctypes.c_void_p(buf.ctypes.data)  # never reached: the arguments are refused first
    sz, u = ctypes.c_size_t, ctypes.c_uint
    for fn, who in ((L.nnz_verifier_from_bytes, b"nnz_verifier_from_bytes"), (L.nnz_prover_from_bytes, b"nnz_prover_from_bytes")):
        for ctx, b, n in ((None, hip.p8(buf), len(buf)), (fake_ctx, None, len(buf)), (fake_ctx, hip.p8(buf), 0)):
            assert fn(ctx, b, sz(n), sz(2), u(0), ctypes.byref(out)) == -1
            assert who + b": null context, null bytes or no bytes" in L.ss_last_error() and not out.value
        assert fn(fake_ctx, hip.p8(buf), sz(len(buf)), sz(2), u(0), None) == -1 and b"null out" in L.ss_last_error()
        for steps in (0, 1):
            assert fn(fake_ctx, hip.p8(buf), sz(len(buf)), sz(steps), u(0), ctypes.byref(out)) == -1
            assert who + b": num_steps: at least two step circuits" in L.ss_last_error() and not out.value
    for flags in (hip.SHAPE_WIRE_FULL, hip.SHAPE_WIRE_FULL_DEVICE):  # the exclusions of the Spartan loaders
        assert L.nnz_verifier_from_bytes(fake_ctx, hip.p8(buf), sz(len(buf)), sz(2), u(flags), ctypes.byref(out)) == -1
        assert b"a verifier's key holds the row-only shapes" in L.ss_last_error()
    for flags in (hip.SHAPE_WIRE_DEVICE, hip.SHAPE_WIRE_HOST, hip.SHAPE_WIRE_DEVICE | host.SS_PK_TRUST_DIGEST):
        assert L.nnz_prover_from_bytes(fake_ctx, hip.p8(buf), sz(len(buf)), sz(2), u(flags), ctypes.byref(out)) == -1
        assert b"a prover's key holds the full shapes" in L.ss_last_error() and not out.value
    with pytest.raises(hip.SpartanHipError, match="null context"):
        host.NeutronNovaVerifier.from_bytes(None, bytes(100), 2)
    for fn in (L.nnz_vk_to_bytes, L.nnz_pk_to_bytes):
        fn.restype = ctypes.c_long
        assert fn(None, *([sz(0)] * 6), *([None] * 9), *([sz(0)] * 6), *([None] * 9), None, sz(0)) < 0 and b"null key" in L.ss_last_error()
    st = (ctypes.c_double * 8)(*([7.0] * 8))
    L.nnz_key_stages(st)  # every load of this thread was refused before its first stage: zeros
    assert list(st) == [0.0] * 8
    assert L.nnz_verifier_device_default() in (0, 1) and L.nnz_prover_full_device_default() in (0, 1)
