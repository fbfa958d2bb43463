"""SHA-256 witness generation on the device (sp_sha256_witness, spartan2_amd/csrc/kernels_witness.hpp) and the prep_prove entry points above it:
the elements the kernel writes equal the frontend generator's witness, and a proof whose witness never left the device is, word for word, the proof
of the existing path (frontend witness + sp_table_write_u64) and of the CPU oracle on the same tape."""
import hashlib

import numpy as np
import pytest

import oracle_lib as ol
from spartan2_amd import frontend, hip, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _msg(n, seed):
    return np.random.default_rng(seed).bytes(n)


def _digest_bits(msg):
    return np.array([(b >> (7 - k)) & 1 for b in hashlib.sha256(msg).digest() for k in range(8)], dtype=np.uint64)


@pytest.mark.parametrize("n", (3, 55, 56, 64, 150, 2048))
def test_kernel_witness_equals_the_frontends(ctx, n):
    msg = _msg(n, 40 + n)
    inst = frontend.sha256_circuit(msg)
    plan = hip.Sha256Plan(ctx, frontend.sha256_witness_plan(n))
    assert plan.n_aux == inst.num_aux
    t = hip.Table.zeros(ctx, plan.n_aux)
    dig = plan.witness([msg], [t])
    assert dig == [hashlib.sha256(msg).digest()]
    got = t.read(0, plan.n_aux)
    want = host.mont_limbs_from_u64(inst.witness)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]
    t.free()
    plan.free()


def test_five_messages_into_five_tables(ctx):
    n = 150
    msgs = [bytes(n), b"\xff" * n] + [_msg(n, 70 + i) for i in range(3)]
    plan = hip.Sha256Plan(ctx, frontend.sha256_witness_plan(n))
    tables = [hip.Table.zeros(ctx, plan.n_aux) for _ in msgs]
    digs = plan.witness(msgs, tables)
    for m, t, d in zip(msgs, tables, digs):
        assert d == hashlib.sha256(m).digest()
        assert (t.read(0, plan.n_aux) == host.mont_limbs_from_u64(frontend.sha256_circuit(m).witness)).all()
        t.free()
    # the step plan: raw blocks, the zero block among them
    splan = hip.Sha256Plan(ctx, frontend.sha256_step_witness_plan())
    blocks = [_msg(64, 90 + i) for i in range(4)] + [bytes(64)]
    tables = [hip.Table.zeros(ctx, splan.n_aux) for _ in blocks]
    splan.witness(blocks, tables)
    for b, t in zip(blocks, tables):
        assert (t.read(0, splan.n_aux) == host.mont_limbs_from_u64(frontend.sha256_step_circuit(b).witness)).all()
        t.free()
    plan.free()
    splan.free()


def test_nonzero_offset_leaves_the_rest_of_the_table_alone(ctx):
    n, off, tail = 56, 1000, 777
    msg = _msg(n, 5)
    plan = hip.Sha256Plan(ctx, frontend.sha256_witness_plan(n))
    rng = np.random.default_rng(3)
    fill = rng.integers(0, 1 << 62, size=(off + plan.n_aux + tail, 4), dtype=np.uint64)  # (canonical: the top limb stays below the modulus')
    t = hip.Table.from_host(ctx, fill)
    plan.witness([msg], [t], off=off)
    got = t.read(0, off + plan.n_aux + tail)
    assert (got[:off] == fill[:off]).all() and (got[off + plan.n_aux :] == fill[off + plan.n_aux :]).all()
    assert (got[off : off + plan.n_aux] == host.mont_limbs_from_u64(frontend.sha256_circuit(msg).witness)).all()
    # a witness that does not fit is refused before anything is launched
    with pytest.raises(hip.SpartanHipError, match="rc=-2"):
        plan.witness([msg], [t], off=off + tail + 1)
    assert (t.read(0, off) == fill[:off]).all()
    t.free()
    plan.free()


@pytest.mark.parametrize("msg", (b"abc", bytes(range(150)), _msg(2048, 2048)), ids=("abc", "150B", "2048B"))
def test_prep_prove_sha256_proof_equals_existing_path_and_oracle(ctx, msg):
    inst = frontend.sha256_circuit(msg)
    tape = ol.make_tape(21 + len(msg), 8192)
    osp = ol.OracleSpartan(inst)
    used_o = osp.prep_prove(tape)
    want, used_o2, _ = osp.prove(tape[used_o:])
    old = host.SpartanSNARK(ctx, inst)
    assert old.prep_prove(tape) == used_o
    old_words, _, _ = old.prove(tape[used_o:])
    # the key of ANOTHER message of this length: the structure depends on the length only
    new = host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(len(msg))))
    assert (new.vk_digest == old.vk_digest).all()
    assert new.prep_prove_sha256(msg, tape) == used_o
    assert (new.publics == _digest_bits(msg)).all() and (new.publics == inst.publics).all()
    for a, b, c in zip(new.prep_export(), old.prep_export(), osp.prep_export()):
        assert (a == b).all() and (a == c).all()
    got, used_g2, _ = new.prove(tape[used_o:])
    assert used_g2 == used_o2
    assert (got == old_words).all() and (got == want).all()
    assert osp.verify_words(got) == 0 and new.verify(got) == 0
    if len(msg) == 150:
        import pyverify

        g, g_s = host.from_label(b"ck", 2049), host.from_label(b"ck_s", 2)
        data = new.proof_to_bytes(got)
        assert pyverify.verify_bytes(inst, g[:2048], g[2048], g_s[0], g_s[1], data, vk_digest=new.vk_digest.tobytes()) == [int(v) for v in inst.publics]
    old.close()
    new.close()


def test_one_key_three_messages(ctx):
    n = 150
    sn = host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(n)))
    for k in range(3):
        msg = _msg(n, 300 + k)
        inst = frontend.sha256_circuit(msg)
        tape = ol.make_tape(500 + k, 8192)
        osp = ol.OracleSpartan(inst)
        used = osp.prep_prove(tape)
        want, _, _ = osp.prove(tape[used:])
        assert sn.prep_prove_sha256(msg, tape) == used
        assert (sn.publics == _digest_bits(msg)).all()
        got, _, _ = sn.prove(tape[used:])
        assert (got == want).all()
        assert osp.verify_words(got) == 0
    sn.close()


def test_neutronnova_prep_prove_sha256(ctx):
    blocks = [_msg(64, 800 + i) for i in range(4)]
    steps = [frontend.sha256_step_circuit(b) for b in blocks]
    core = frontend.sha256_step_circuit(bytes(64))
    onn = ol.OracleNeutronNova(steps, core)
    tape = ol.make_tape(4242, 32768)
    want, used, _ = onn.prove(tape)
    old = host.NeutronNovaZkSNARK(ctx, steps, core)
    assert old.prep_prove(tape) == used[0]
    old_words, _, _ = old.prove(tape[used[0]:])
    # a key set up from OTHER blocks: the step circuit is the same for every block
    other = [frontend.sha256_step_circuit(bytes([i]) * 64) for i in range(4)]
    new = host.NeutronNovaZkSNARK(ctx, other, core)
    assert (new.vk_digest == old.vk_digest).all()
    assert new.prep_prove_sha256(blocks, tape) == used[0]
    got, used_g, _ = new.prove(tape[used[0]:])
    assert used_g == used[1]
    assert (got == old_words).all() and (got == want).all()
    assert onn.verify_words(got) == 0 and new.verify(got) == 0
    old.close()
    new.close()


def test_plan_of_another_length_is_refused(ctx):
    sn = host.SpartanSNARK(ctx, frontend.sha256_circuit(b"abc"))
    tape = ol.make_tape(9, 8192)
    with pytest.raises(hip.SpartanHipError, match="rc=-2"):  # SP_ERR_INVALID_WITNESS_LENGTH
        sn.prep_prove_sha256(bytes(150), tape)
    assert sn.ps is None
    # ... and the context proves normally afterwards
    inst = frontend.sha256_circuit(b"abd")
    osp = ol.OracleSpartan(inst)
    used = osp.prep_prove(tape)
    want, _, _ = osp.prove(tape[used:])
    assert sn.prep_prove_sha256(b"abd", tape) == used
    got, _, _ = sn.prove(tape[used:])
    assert (got == want).all() and osp.verify_words(got) == 0
    sn.close()
