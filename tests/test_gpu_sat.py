"""GPU checks of is_sat (R1CSShape::is_sat / is_sat_relaxed, src/r1cs/mod.rs:358-394, :430-471) at every layer: the residual kernel on raw tables, the
relaxed form and Shape.is_sat on two circuits, SpartanSNARK.is_sat (both witness sources, a circuit with a verifier challenge, the commitment leg) and
NeutronNovaZkSNARK.is_sat. Every expected failing set is computed here from the CPU oracle's products (orc_shape_multiply_vec) with Python integers
mod p; nothing expected comes from the code under test."""
import hashlib

import numpy as np
import pytest

import oracle_lib as ol
from challenge_circuit import ChallengeCircuit
from spartan2_amd import frontend, hip, host
from spartan2_amd.host import pad_shape

pytestmark = pytest.mark.gpu
P = ol.MODULI[0]
RINV = pow(ol.R, -1, P)
UNSAT, BADCOMM = "R1CS is unsatisfiable", "Invalid commitment"


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


# ---- helpers: Python integers <-> limb arrays ------------------------------------------------------------------------------------------------------
def limbs_of_raw(vals):
    """Python integers < 2^256 -> (n, 4) uint64 limbs, as they are (no Montgomery conversion)"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def random_residues(rng, n):
    raw = rng.bytes(32 * n)
    return [int.from_bytes(raw[32 * i : 32 * i + 32], "little") % P for i in range(n)]


def check_report(rep, want_rows):
    want_rows = sorted(want_rows)
    print(f"num_failing {rep.num_failing} (want {len(want_rows)}), first {rep.first_failing[:4]}.. (want {want_rows[:4]}..)")
    assert rep.num_failing == len(want_rows)
    assert rep.first_failing == want_rows[:16]
    assert rep.ok == (not want_rows) and rep.reason == (UNSAT if want_rows else None)


def oracle_products(oshape, z):
    N = oshape.num_cons
    out = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
    z = np.ascontiguousarray(z, dtype=np.uint64)
    assert z.shape[0] == oshape.num_vars + oshape.num_extra
    assert ol.lib().orc_shape_multiply_vec(oshape.h, ol.p64(z), *(ol.p64(w) for w in out)) == 0
    return [ol.ints_of(w) for w in out]


def oracle_failing(oshape, z, u=1, E=None):
    """rows with Az Bz - u Cz - E != 0 mod p, from the oracle's products"""
    a, b, c = oracle_products(oshape, z)
    E = E if E is not None else [0] * len(a)
    return [i for i in range(len(a)) if (a[i] * b[i] - u * c[i] - E[i]) % P != 0]


def padded_z(oshape, witness, publics, challenges=()):
    """z = [W | 1 | X | challenges] in the padded layout (each witness segment at its padded offset), Montgomery limbs"""
    w = [int(x) for x in witness]
    s, p, r = oshape.num_shared_unpadded, oshape.num_precommitted_unpadded, oshape.num_rest_unpadded
    W = np.zeros((oshape.num_vars, 4), dtype=np.uint64)
    if s:
        W[:s] = ol.mont_array(w[:s])
    if p:
        W[oshape.num_shared : oshape.num_shared + p] = ol.mont_array(w[s : s + p])
    if r:
        W[oshape.num_shared + oshape.num_precommitted : oshape.num_shared + oshape.num_precommitted + r] = ol.mont_array(w[s + p : s + p + r])
    return np.concatenate([W, ol.mont_array([1] + [int(x) for x in publics] + [int(c) for c in challenges])])


def circuit(which):
    return frontend.synthetic_circuit(40, 0xDEADBEEF, num_public=3) if which == "synthetic" else frontend.sha256_circuit(b"abc")


# ---- 1. the residual kernel on raw tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, (1 << 20) + 3])
def test_residual_on_raw_tables(ctx, n):
    rng = np.random.default_rng(1000 + n % 977)
    # the limbs ARE the Montgomery forms a~ = a R, b~ = b R; the product's form is a~ b~ R^-1
    a, b = random_residues(rng, n), random_residues(rng, n)
    c = [x * y % P * RINV % P for x, y in zip(a, b)]
    az, bz, cz = (hip.Table.from_host(ctx, limbs_of_raw(v)) for v in (a, b, c))
    check_report(hip.r1cs_residual(ctx, az, bz, cz), [])
    assert hip.r1cs_residual(ctx, az, bz, cz, n=n).num_failing == 0
    sets = [[0], [n - 1]]
    if n >= 66:
        sets.append([63, 64, 65])
    if n >= 4096:
        sets.append(sorted(int(r) for r in np.random.default_rng(77).choice(n, size=40, replace=False)))
        sets.append(sorted(set(sets[-1]) | {0, n - 1, 63, 64, 65}))
    for rows in sets:
        for r in rows:
            cz.write(r, limbs_of_raw([(c[r] + 1) % P]))
        check_report(hip.r1cs_residual(ctx, az, bz, cz), rows)
        for r in rows:
            cz.write(r, limbs_of_raw([c[r]]))
    check_report(hip.r1cs_residual(ctx, az, bz, cz), [])
    # the batched form: instance 0 satisfied, instance 1 with one bad row
    bad_row = n // 2
    cz2 = hip.Table.from_host(ctx, limbs_of_raw(c[:bad_row] + [(c[bad_row] + 5) % P] + c[bad_row + 1 :]))
    reps = hip.r1cs_residual_batched(ctx, [az, az], [bz, bz], [cz, cz2])
    check_report(reps[0], [])
    check_report(reps[1], [bad_row])
    # a table shorter than n: InvalidInputLength
    with pytest.raises(hip.SpartanHipError, match="rc=-1"):
        hip.r1cs_residual(ctx, az, bz, cz, n=n + 1)
    for t in (az, bz, cz, cz2):
        t.free()


# ---- 2. the relaxed form ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["synthetic", "sha256_abc"])
def test_relaxed_form(ctx, which):
    inst = circuit(which)
    oshape = ol.OracleShape(inst)
    mats, dims = pad_shape(inst)
    shape = hip.Shape(ctx, mats, dims)
    rng = np.random.default_rng(21)
    N, ncols = oshape.num_cons, oshape.num_vars + oshape.num_extra
    z = ol.random_field_array(rng, ncols)
    u_limbs = ol.random_field_array(rng, 1)[0]
    u = ol.from_mont(u_limbs)
    a, b, c = oracle_products(oshape, z)
    E = [(a[i] * b[i] - u * c[i]) % P for i in range(N)]
    zt, Et = hip.Table.from_host(ctx, z), hip.Table.from_host(ctx, ol.mont_array(E))
    check_report(shape.is_sat(zt, u=u_limbs, E=Et), [])
    j = N // 3
    Et.write(j, ol.mont_array([(E[j] + 1) % P]))
    check_report(shape.is_sat(zt, u=u_limbs, E=Et), [j])
    Et.write(j, ol.mont_array([E[j]]))
    u2 = (u + 12345) % P
    want = [i for i in range(N) if (a[i] * b[i] - u2 * c[i] - E[i]) % P != 0]
    assert want, "a changed u must break the rows with Cz != 0"
    check_report(shape.is_sat(zt, u=ol.to_mont(u2), E=Et), want)
    # the same through the raw-table entry point, on products the device computed
    outs = [hip.Table.zeros(ctx, N) for _ in range(3)]
    shape.multiply_vec(zt, *outs)
    check_report(hip.r1cs_residual(ctx, *outs, u=u_limbs, E=Et), [])
    check_report(hip.r1cs_residual(ctx, *outs, u=ol.to_mont(u2), E=Et), want)
    # E alone (u = 1) and u alone (E = 0) against Python
    check_report(hip.r1cs_residual(ctx, *outs, E=Et), [i for i in range(N) if (a[i] * b[i] - c[i] - E[i]) % P != 0])
    check_report(hip.r1cs_residual(ctx, *outs, u=u_limbs), [i for i in range(N) if (a[i] * b[i] - u * c[i]) % P != 0])


# ---- 3. Shape.is_sat on the real assignment -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["synthetic", "sha256_abc"])
def test_shape_is_sat(ctx, which):
    inst = circuit(which)
    oshape = ol.OracleShape(inst)
    mats, dims = pad_shape(inst)
    shape = hip.Shape(ctx, mats, dims)
    z = padded_z(oshape, inst.witness, inst.publics)
    assert oracle_failing(oshape, z) == []
    check_report(shape.is_sat(hip.Table.from_host(ctx, z)), [])
    # one aux variable flipped
    w = inst.witness.copy()
    k = len(w) // 2
    w[k] = 1 - int(w[k]) if int(w[k]) in (0, 1) else int(w[k]) + 1
    zf = padded_z(oshape, w, inst.publics)
    want = oracle_failing(oshape, zf)
    assert want
    check_report(shape.is_sat(hip.Table.from_host(ctx, zf)), want)
    # a random z: the list is cut at 16
    zr = ol.random_field_array(np.random.default_rng(5), z.shape[0])
    want = oracle_failing(oshape, zr)
    assert len(want) > 16
    check_report(shape.is_sat(hip.Table.from_host(ctx, zr)), want)
    # a z of the wrong length: InvalidWitnessLength, as multiply_vec (:412-414)
    with pytest.raises(hip.SpartanHipError, match="rc=-2"):
        shape.is_sat(hip.Table.from_host(ctx, z[:-1]))


# ---- 4. SpartanSNARK.is_sat ------------------------------------------------------------------------------------------------------------------------------
MSG = bytes(range(64))


def _flip(witness, k):
    w = witness.copy()
    w[k] = 1 - int(w[k])
    return w


def test_spartan_is_sat_and_the_proof_after_it(ctx):
    inst = frontend.sha256_circuit(MSG)
    tape = ol.make_tape(11, 4096)
    osp = ol.OracleSpartan(inst)
    used = osp.prep_prove(tape)
    want, _, _ = osp.prove(tape[used:])
    gsp = host.SpartanSNARK(ctx, inst)
    with pytest.raises(hip.SpartanHipError):  # misuse: before prep_prove
        gsp.is_sat()
    assert gsp.prep_prove(tape) == used
    rep = gsp.is_sat()
    check_report(rep, [])
    assert rep.bad_commitment_rows == []
    assert gsp.is_sat().ok  # (a second call: the scratch it keeps is reused)
    got, _, _ = gsp.prove(tape[used:])
    assert (got == want).all(), "the proof after is_sat differs from the oracle's"
    assert gsp.is_sat().ok  # and after a prove
    # commitment leg: the stored rows with one row replaced by another valid point
    comm = gsp.prep_export()[0]
    assert comm.shape[0] > 5 and not (comm[3] == comm[5]).all()
    assert gsp.is_sat(commitment=comm).ok
    other = comm.copy()
    other[3] = comm[5]
    rep = gsp.is_sat(commitment=other)
    assert not rep.ok and rep.reason == BADCOMM and rep.bad_commitment_rows == [3] and rep.num_failing == 0
    with pytest.raises(hip.SpartanHipError):  # misuse: a wrong number of public values
        gsp.is_sat(publics=inst.publics[:-1])
    gsp.close()


def test_spartan_is_sat_names_the_rows_of_an_altered_witness(ctx):
    inst = frontend.sha256_circuit(MSG)
    oshape = ol.OracleShape(inst)
    assert int(inst.witness[5000]) in (0, 1)
    inst.witness = _flip(inst.witness, 5000)
    want = oracle_failing(oshape, padded_z(oshape, inst.witness, inst.publics))
    assert want
    tape = ol.make_tape(12, 4096)
    gsp = host.SpartanSNARK(ctx, inst)
    used = gsp.prep_prove(tape)
    rep = gsp.is_sat()
    check_report(rep, want)
    assert rep.bad_commitment_rows == []  # the commitment IS the commitment of that (wrong) witness
    # ... and what users see today: the proof from that state is rejected
    got, _, _ = gsp.prove(tape[used:])
    assert gsp.verify(got) != 0
    gsp.close()


def test_spartan_is_sat_after_prep_prove_sha256(ctx):
    inst = frontend.sha256_circuit(MSG)  # the key: any message of this length
    msg, other = bytes((7 * i + 1) & 0xFF for i in range(64)), bytes((3 * i + 2) & 0xFF for i in range(64))
    tape = ol.make_tape(13, 4096)
    gsp = host.SpartanSNARK(ctx, inst)
    gsp.prep_prove_sha256(msg, tape)
    mine = frontend.sha256_circuit(msg)
    bits = lambda m: [(hashlib.sha256(m).digest()[i // 8] >> (7 - i % 8)) & 1 for i in range(256)]
    assert [int(v) for v in gsp.publics] == bits(msg) == [int(v) for v in mine.publics]
    rep = gsp.is_sat()
    check_report(rep, [])
    assert rep.bad_commitment_rows == []
    # against another message's digest bits: the rows that bind the digest fail
    oshape = ol.OracleShape(mine)
    want = oracle_failing(oshape, padded_z(oshape, mine.witness, bits(other)))
    assert want
    check_report(gsp.is_sat(publics=np.array(bits(other), dtype=np.uint64)), want)
    check_report(gsp.is_sat(), [])
    gsp.close()


def test_spartan_is_sat_with_a_verifier_challenge(ctx):
    inst = ChallengeCircuit(120, seed=3)
    oshape = ol.OracleShape(inst)
    syn = inst.synthesize(ol.to_mont, ol.from_mont)
    tape = ol.make_tape(14, 8192)
    osp = ol.OracleSpartan(inst)
    used = osp.prep_prove(tape, is_small=False)
    want, _, _ = osp.prove(tape[used:], synthesize=syn)
    gsp = host.SpartanSNARK(ctx, inst)
    assert gsp.prep_prove(tape, is_small=False) == used
    ch = ol.random_field_array(np.random.default_rng(8), 1)  # any challenge: the constraints hold for every one
    c_int = ol.from_mont(ch[0])

    def z_for(rest_limbs):
        K = inst.K
        w = [int(v) for v in inst.witness[: 2 * K]] + ol.ints_of(rest_limbs)
        return padded_z(oshape, w, inst.publics, [c_int])

    assert oracle_failing(oshape, z_for(syn(ch))) == []
    rep = gsp.is_sat(challenges=ch, synthesize=syn)
    check_report(rep, [])
    assert rep.bad_commitment_rows == []

    def wrong(chs):
        rest = syn(chs).copy()
        rest[7] = ol.to_mont(ol.from_mont(rest[7]) + 1)
        return rest

    want_rows = oracle_failing(oshape, z_for(wrong(ch)))
    assert want_rows
    check_report(gsp.is_sat(challenges=ch, synthesize=wrong), want_rows)
    with pytest.raises(hip.SpartanHipError):  # misuse: the circuit has a challenge and none was given
        gsp.is_sat()
    got, _, _ = gsp.prove(tape[used:], synthesize=syn)
    assert (got == want).all(), "the proof after is_sat differs from the oracle's"
    gsp.close()


# ---- 5. NeutronNovaZkSNARK.is_sat ----------------------------------------------------------------------------------------------------------------------
def test_neutronnova_is_sat(ctx):
    steps = [frontend.sha256_step_circuit(bytes([i]) * 64) for i in range(4)]
    core = frontend.sha256_step_circuit(bytes(64))
    onn = ol.OracleNeutronNova(steps, core)
    tape = ol.make_tape(404, 32768)
    want, used, _ = onn.prove(tape)
    gnn = host.NeutronNovaZkSNARK(ctx, steps, core)
    with pytest.raises(hip.SpartanHipError):
        gnn.is_sat()
    assert gnn.prep_prove(tape) == used[0]
    reps = gnn.is_sat()
    assert len(reps) == 5
    for r in reps:
        check_report(r, [])
        assert r.bad_commitment_rows == []
    got, _, _ = gnn.prove(tape[used[0]:])
    assert (got == want).all(), "the proof after is_sat differs from the oracle's"
    # step 2's witness altered: only report 2 fails
    oshape = ol.OracleShape(steps[2])
    assert int(steps[2].witness[9000]) in (0, 1)
    steps[2].witness = _flip(steps[2].witness, 9000)
    want_rows = oracle_failing(oshape, padded_z(oshape, steps[2].witness, steps[2].publics))
    assert want_rows
    gnn.prep_prove(tape)
    reps = gnn.is_sat()
    for i, r in enumerate(reps):
        check_report(r, want_rows if i == 2 else [])
        assert r.bad_commitment_rows == []
    gnn.close()
