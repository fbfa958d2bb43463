"""GPU parity: sp_poly_abc_batch - evals_rx + poly_ABC of K proofs of one shape in one pass over interleaved eq tables - and the prove_batch options that
take it and the batched rest commitments. Every comparison is bit-exact against the CPU oracle (orc_eq_evals -> orc_shape_poly_abc per proof; the oracle's
proofs for the driver). The shapes are chosen for where the walk can go wrong: rest-only and tiny (cubic), every column short (5x7), one long column
served by a single block (40xDEADBEEF), a long column shared by four blocks behind the arrival counter (SHA-256, one block)."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import pyverify
from oracle_lib import lib as olib, p64
from spartan2_amd import frontend, hip, host
from spartan2_amd.host import pad_shape

pytestmark = pytest.mark.gpu

#          instance                                                       ell  long columns
SHAPES = {
    "cubic": (lambda: frontend.cubic_circuit(), 2, 0),
    "5x7": (lambda: frontend.synthetic_circuit(5, 7, num_public=2), 9, 0),
    "40xDEADBEEF": (lambda: frontend.synthetic_circuit(40, 0xDEADBEEF, num_public=3), 12, 1),
    "sha256_abc": (lambda: frontend.sha256_circuit(b"abc"), 15, 1),
}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens():
    return host.from_label(b"ck", 2049), host.from_label(b"ck_s", 2)


class Case:
    """one shape on the device and in the oracle, with a pool of (r_x, r) pairs whose oracle results are computed once and shared by the tests"""

    def __init__(self, ctx, name):
        make, ell, n_long = SHAPES[name]
        self.inst = make()
        self.oshape = ol.OracleShape(self.inst)
        mats, dims = pad_shape(self.inst)
        self.shape = hip.Shape(ctx, mats, dims)
        self.N, self.M = self.oshape.num_cons, self.oshape.num_vars
        self.ncols = self.M + self.oshape.num_extra
        self.ell = ell
        assert self.N == 1 << ell, (name, self.N)
        info = (ctypes.c_uint64 * 8)()
        assert hip.lib().sp_shape_info(self.shape.h, info) == 0
        assert int(info[6]) == n_long, (name, int(info[6]))
        self.KC = hip.poly_abc_batch_chunk()
        self.rng = np.random.default_rng(0xABC0 + ell)
        n = 2 * self.KC + 1
        self.r_x = ol.random_field_array(self.rng, n * ell).reshape(n, ell, 4)
        self.r = ol.random_field_array(self.rng, n)
        self.want = [self.oracle(self.r_x[k], self.r[k]) for k in range(n)]

    def oracle(self, r_x, r):
        """evals_from_points(r_x) -> bind_and_prepare_poly_ABC_full: 2 M elements (the first ncols of them are the compact form)"""
        r_x = np.ascontiguousarray(r_x, dtype=np.uint64).reshape(self.ell, 4)
        evals = np.zeros((self.N, 4), dtype=np.uint64)
        assert olib().orc_eq_evals(p64(r_x), ctypes.c_size_t(self.ell), p64(evals)) == 0
        out = np.zeros((2 * self.M, 4), dtype=np.uint64)
        assert olib().orc_shape_poly_abc(self.oshape.h, p64(evals), p64(np.ascontiguousarray(r)), ctypes.c_size_t(2 * self.M), p64(out)) == 0
        assert not out[self.ncols :].any()
        return out

    def dirty(self, ctx, n):
        return ol.random_field_array(self.rng, 16).repeat((n + 15) // 16, axis=0)[:n]

    def run(self, ctx, r_x, r, want, out_len, extra=3):
        """the batch on dirty tables of out_len + extra elements: the first out_len equal the oracle's, the rest are untouched"""
        K = len(want)
        dirt = [self.dirty(ctx, out_len + extra) for _ in range(K)]
        outs = [hip.Table.from_host(ctx, d) for d in dirt]
        self.shape.poly_abc_batch(r_x, r, out_len, outs)
        for k in range(K):
            got = outs[k].read(0, out_len + extra)
            assert (got[:out_len] == want[k][:out_len]).all(), f"proof {k} of {K} differs from the oracle's"
            assert (got[out_len:] == dirt[k][out_len:]).all(), f"proof {k} of {K}: elements past out_len were written"
            assert outs[k].info() == (out_len + extra, hip.SIZE_MAX, hip.SIZE_MAX)  # the length fields are left alone, as sp_poly_abc leaves them
        for t in outs:
            t.free()


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request, ctx):
    return Case(ctx, request.param)


def test_counts_and_lengths_equal_the_oracle(ctx, case):
    KC = case.KC
    for K in sorted({1, 2, KC - 1, KC, KC + 1, 2 * KC + 1} - {0}):
        for out_len in (case.ncols, 2 * case.M):
            case.run(ctx, case.r_x[:K], case.r[:K], case.want[:K], out_len)
    # count == 0 is a no-op
    case.shape.poly_abc_batch(np.zeros((0, case.ell, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), 2 * case.M, [])


def test_edge_values(ctx, case):
    ell, one = case.ell, ol.to_mont(1)
    rxA, rxB, rxC = case.r_x[0], case.r_x[1], case.r_x[2]
    r1, r2 = case.r[0], case.r[1]
    zero = np.zeros(4, dtype=np.uint64)
    pairs = [(rxA, r1), (rxA, r2), (rxB, r2), (rxC, zero), (np.zeros((ell, 4), dtype=np.uint64), case.r[3]), (np.tile(one, (ell, 1)), case.r[4])]
    want = [case.want[0]] + [case.oracle(x, r) for x, r in pairs[1:]]
    assert not (want[0] == want[1]).all() and not (want[1] == want[2]).all()
    case.run(ctx, np.stack([x for x, _ in pairs]), np.stack([r for _, r in pairs]), want, 2 * case.M)


def test_counters_are_left_at_zero(ctx, case):
    """the batch twice in a row, then interleaved with sp_poly_abc on the same context and shape"""
    K, M = case.KC + 1, case.M

    def single(k):
        out = hip.Table.from_host(ctx, case.dirty(ctx, 2 * M))
        rx = hip.Table.eq(ctx, case.r_x[k])
        case.shape.poly_abc(rx, case.r[k], 2 * M, out)
        assert (out.read(0, 2 * M) == case.want[k]).all()
        out.free()
        rx.free()

    case.run(ctx, case.r_x[:K], case.r[:K], case.want[:K], 2 * M)
    case.run(ctx, case.r_x[:K], case.r[:K], case.want[:K], 2 * M)
    single(0)
    case.run(ctx, case.r_x[1 : K + 1], case.r[1 : K + 1], case.want[1 : K + 1], 2 * M)
    single(K)
    case.run(ctx, case.r_x[:2], case.r[:2], case.want[:2], case.ncols)


def test_refusals_write_nothing(ctx):
    case = Case(ctx, "5x7")
    L, M, ell, ncols = hip.lib(), case.M, case.ell, case.ncols
    K = 5
    dirt = [case.dirty(ctx, 2 * M) for _ in range(K)]
    outs = [hip.Table.from_host(ctx, d) for d in dirt]
    short = hip.Table.from_host(ctx, dirt[0][: 2 * M - 1])
    r_x, r = np.ascontiguousarray(case.r_x[:K]), np.ascontiguousarray(case.r[:K])
    sz = ctypes.c_size_t

    def call(handles, n=K, rx=r_x, ell_=ell, rr=r, out_len=2 * M, c=ctx.h, s=case.shape.h):
        arr = (ctypes.c_void_p * len(handles))(*handles) if handles is not None else None
        rc = L.sp_poly_abc_batch(c, s, sz(n), p64(rx) if rx is not None else None, sz(ell_), p64(rr) if rr is not None else None, sz(out_len), arr)
        return rc, L.sp_last_error().decode()

    hs = [t.h for t in outs]
    refused = [
        (call(hs, c=None), None),
        (call(hs, s=None), None),
        (call(hs, rx=None), None),
        (call(hs, rr=None), None),
        (call(None), None),
        (call(hs[:3] + [None] + hs[4:]), 3),
        (call(hs, ell_=ell - 1), None),
        (call(hs, ell_=ell + 1), None),
        (call(hs, out_len=ncols - 1), None),
        (call(hs[:2] + [short.h] + hs[3:]), 2),
        (call(hs[:4] + [hs[1]]), 4),
    ]
    for (rc, msg), index in refused:
        assert rc == -1 and "poly_abc_batch" in msg, (rc, msg)
        if index is not None:
            assert msg.endswith(f", proof {index}"), msg
    for t, d in zip(outs, dirt):
        assert (t.read(0, 2 * M) == d).all(), "a refused call wrote to an output"
    assert (short.read(0, 2 * M - 1) == dirt[0][: 2 * M - 1]).all()
    # the context goes on proving
    case.run(ctx, r_x, r, case.want[:K], 2 * M)


# ---- the driver: prove_batch under all four combinations of the two options ------------------------------------------------------------------------
def oracles_prepped(insts, seed):
    osps, tapes, used = [], [], []
    for k, inst in enumerate(insts):
        osp = ol.OracleSpartan(inst)
        tape = ol.make_tape(seed + k, 1024)
        used.append(osp.prep_prove(tape))
        osps.append(osp)
        tapes.append(tape)
    return osps, tapes, used


def driver_instances(name):
    """-> (instance the key is made of, instances of the proofs, prep_prove_batch keywords, tape blocks)"""
    if name == "5x7":  # the rest segment is all padding: commit_zeros
        insts = [frontend.synthetic_circuit(5, 7, num_public=2, witness_seed=1000 * k) for k in range(3)]
        return insts[0], insts, dict(witnesses=insts), 4096
    if name == "5x7_rest":  # one shape, three witnesses, a non-empty rest segment: sp_hyrax_commit_batch on it
        insts = [frontend.synthetic_circuit(5, 7, num_public=2, shared_permille=200, precommitted_permille=500, witness_seed=1000 * k) for k in range(3)]
        assert insts[0].num_shared > 0 and insts[0].num_precommitted > 0 and insts[0].num_rest > 0
        return insts[0], insts, dict(witnesses=insts), 4096
    if name == "cubic":  # rest-only
        insts = [frontend.cubic_circuit() for _ in range(2)]
        assert insts[0].num_precommitted == 0 and insts[0].num_shared == 0
        return insts[0], insts, dict(witnesses=insts), 4096
    msgs = [bytes((37 * i + 11 * k + 3) % 256 for i in range(3)) for k in range(3)]  # device-generated witnesses
    return frontend.sha256_circuit(bytes(3)), [frontend.sha256_circuit(m) for m in msgs], dict(msgs=msgs), 8192


@pytest.mark.parametrize("name", ["5x7", "5x7_rest", "cubic", "sha256_3B"])
def test_prove_batch_under_every_combination_of_the_options(ctx, gens, name):
    key_inst, insts, prep_kw, blocks = driver_instances(name)
    K = len(insts)
    osps, prep_tapes, prep_used = oracles_prepped(insts, 4100)
    gsp = host.SpartanSNARK(ctx, key_inst)
    assert gsp.prep_prove_batch(prep_tapes, **prep_kw) == prep_used
    tapes = [ol.make_tape(4200 + k, blocks) for k in range(K)]
    want = [osps[k].prove(tapes[k]) for k in range(K)]  # once: every combination must make these proofs of these tapes
    lone_tape = ol.make_tape(4300, blocks)
    lone_want = osps[K - 1].prove(lone_tape)
    (g, g_s) = gens
    first = True
    for per_proof_polyabc in (False, True):
        for per_proof_rest_commit in (False, True):
            got, phases = gsp.prove_batch(tapes, per_proof_polyabc=per_proof_polyabc, per_proof_rest_commit=per_proof_rest_commit)
            assert len(got) == K and phases["total"] > 0
            for k, (words, used) in enumerate(got):
                leg = f"{name}: proof {k}, per_proof_polyabc={per_proof_polyabc}, per_proof_rest_commit={per_proof_rest_commit}"
                assert used == want[k][1], leg
                assert len(words) == len(want[k][0]) and (words == want[k][0]).all(), leg + " differs from the oracle's"
                assert gsp.verify(words) == 0, leg
                if first:
                    data = gsp.proof_to_bytes(words)
                    assert pyverify.verify_bytes(insts[k], g[:2048], g[2048], g_s[0], g_s[1], data, vk_digest=gsp.vk_digest.tobytes()) == [int(v) for v in insts[k].publics]
            first = False
            # a lone prove on one of the states still equals the oracle
            gsp.ps, gsp.publics = gsp.batch[K - 1]
            words, used, _ = gsp.prove(lone_tape)
            assert used == lone_want[1] and (words == lone_want[0]).all()
    # the driver's own choice makes the same proofs
    got, _ = gsp.prove_batch(tapes)
    for k, (words, used) in enumerate(got):
        assert used == want[k][1] and (words == want[k][0]).all()
    gsp.close()
