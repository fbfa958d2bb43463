"""Witness plans of the SHA-256 circuits (spartan2_amd/frontend/sha256_witness_plan.hpp) against the circuit generator they were recorded from:
plan.eval(msg) - native compressions -> trace -> bits - must give the generator's witness for every message of the length, element for element."""
import hashlib

import numpy as np
import pytest

from spartan2_amd import frontend

LENGTHS = (1, 3, 55, 56, 63, 64, 65, 119, 120, 150, 1024, 2048)


def _messages(n):
    rng = np.random.default_rng(1000 + n)
    return [bytes(n), b"\xff" * n, rng.bytes(n), rng.bytes(n)]


def _digest_bits(msg):
    return np.array([(b >> (7 - k)) & 1 for b in hashlib.sha256(msg).digest() for k in range(8)], dtype=np.uint64)


@pytest.mark.parametrize("n", LENGTHS)
def test_plan_eval_equals_the_generators_witness(n):
    plan = frontend.sha256_witness_plan(n)
    assert plan.msg_len == n and plan.padded and plan.n_pre == 8 * n and plan.n_blocks == (n + 9 + 63) // 64
    assert plan.descriptors.shape == (plan.n_aux,) and plan.block_starts.shape == (plan.n_blocks + 1,)
    assert int(plan.block_starts[0]) == plan.n_pre and int(plan.block_starts[-1]) == plan.n_aux
    assert ((plan.descriptors & 0x7FF) < plan.trace_slots).all()
    for msg in _messages(n):
        inst = frontend.sha256_circuit(msg)
        assert inst.num_aux == plan.n_aux
        w, dig = plan.eval(msg, with_digest=True)
        assert w.dtype == np.uint64 and w.shape == inst.witness.shape
        assert (w == inst.witness).all(), np.nonzero(w != inst.witness)[0][:8]
        assert int(w.max()) <= 1
        assert dig == hashlib.sha256(msg).digest()
        assert (inst.publics == _digest_bits(msg)).all()


@pytest.mark.parametrize("n", (1, 55, 56, 64, 65, 120, 200))
def test_circuit_structure_depends_only_on_the_length(n):
    """What makes one plan (and one key) serve every message of a length: the matrices of two different messages are equal entry for entry."""
    a, b, c = (frontend.sha256_circuit(m) for m in _messages(n)[:3])
    for other in (b, c):
        assert (a.num_cons, a.num_aux, a.num_public) == (other.num_cons, other.num_aux, other.num_public)
        for (d0, i0, p0), (d1, i1, p1) in zip(a.csr, other.csr):
            assert (d0 == d1).all() and (i0 == i1).all() and (p0 == p1).all()
    s0, s1 = frontend.sha256_step_circuit(bytes(64)), frontend.sha256_step_circuit(bytes(range(64)))
    for (d0, i0, p0), (d1, i1, p1) in zip(s0.csr, s1.csr):
        assert (d0 == d1).all() and (i0 == i1).all() and (p0 == p1).all()


def test_step_plan_equals_the_step_circuits_witness():
    plan = frontend.sha256_step_witness_plan()
    assert plan.msg_len == 64 and not plan.padded and plan.n_blocks == 1 and plan.n_pre == 512
    rng = np.random.default_rng(7)
    for block in [rng.bytes(64) for _ in range(4)] + [bytes(64)]:
        inst = frontend.sha256_step_circuit(block)
        w = plan.eval(block)
        assert (w == inst.witness).all(), np.nonzero(w != inst.witness)[0][:8]
        assert int(w[-1]) == 0  # x = 0


def test_plan_refusals():
    with pytest.raises(RuntimeError):
        frontend.sha256_witness_plan(0)  # no witness variable to place
    plan = frontend.sha256_witness_plan(3)
    with pytest.raises(ValueError):
        plan.eval(b"abcd")


def _fingerprint(inst):
    h = hashlib.sha256()
    for v in (inst.num_cons, inst.num_shared, inst.num_precommitted, inst.num_rest, inst.num_public, inst.addmany_rows, inst.multieq_rows):
        h.update(int(v).to_bytes(8, "little"))
    for d, i, p in inst.csr:
        for a in (d, i, p):
            h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.ascontiguousarray(inst.witness).tobytes())
    h.update(np.ascontiguousarray(inst.publics).tobytes())
    return h.hexdigest()


def test_generator_outputs_are_what_they_were_before_the_recorder():
    """The recorder is additive: dims, matrices, witness and publics of the generators, fingerprinted on the commit before it existed."""
    assert _fingerprint(frontend.sha256_circuit(b"abc")) == "8b544dd4f6061b0f0a59e674ca94debed3718039dbefb256fc3f9bca0b52d742"
    assert _fingerprint(frontend.sha256_circuit(bytes(range(150)))) == "2e99cbb899e18eb06f7a7a9784c02d731d45f28658b27c3a6d991cf01feb1da4"
    assert _fingerprint(frontend.sha256_step_circuit(bytes(range(64)))) == "647161d2c1bb4909a3da1b135c6cc4a9f326db0cfa800b3931e345d747a2d715"
    assert _fingerprint(frontend.sha256_rest_circuit(bytes(range(32)))) == "f9c1b3407e856cea80c24f5b649bf6ff1c21b0a4e461c0dca8958f4d1e809b7a"
