"""GPU parity: the lockstep sum-checks (sp_sumcheck_cubic3_lockstep / sp_sumcheck_quad_lockstep) - K instances over K table sets of one length, one
launch per round for all of them - against the CPU oracle PER INSTANCE, bit-exact: polynomials, challenges, final claims, the transcript afterwards.
Every instance has its own tables, its own tau and its own transcript (k extra absorbs in front, so no two instances draw equal challenges)."""
import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import p64
from spartan2_amd import hip
from test_gpu_sumcheck import oracle_cubic, oracle_quad, rand_table, satisfying_tables

pytestmark = pytest.mark.gpu

SEED = 0x10C5
FULL = (hip.SIZE_MAX, hip.SIZE_MAX)

# which launch form an ell exercises (kernels_lockstep.hpp): up to LS_SINGLE_MAX_PAIRS = 1024 pairs one block per instance does the whole round
# ("single"); above that the blocks leave partials, k_ls_sum_partials follows and the eq weights are factored (a chunk of pairs = one x_out) ("partials").
# There is no streaming form. ell = 12 is the smallest table whose first round has more than 1024 pairs; at 13 and 16 the left eq pyramid has levels.
CUBIC_FORMS = {1: "single", 2: "single", 3: "single", 7: "single", 11: "single (1024 pairs: the threshold)", 12: "partials + second stage (2 blocks)",
               13: "partials (2 rounds), left pyramid level 2", 16: "partials (5 rounds), the largest table of this file"}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def transcripts(ctx, label, K):
    """(device transcript k, oracle transcript k), both with k extra absorbs"""
    g, o = [], []
    for k in range(K):
        a, b = hip.Transcript(ctx, label), ol.Transcript(label)
        for j in range(k):
            a.absorb(b"extra", bytes([j, k]))
            b.absorb(b"extra", bytes([j, k]))
        g.append(a)
        o.append(b)
    return g, o


def oracle_cubic_on(tr, claim, taus, A, B, C):
    """oracle_cubic of test_gpu_sumcheck with the oracle transcript replaced by one that already carries the instance's extra absorbs"""
    import ctypes

    ell = len(taus)
    polys = np.zeros((ell, 3, 4), dtype=np.uint64)
    r = np.zeros((ell, 4), dtype=np.uint64)
    fin = np.zeros((3, 4), dtype=np.uint64)
    a, b, c = A.copy(), B.copy(), C.copy()
    assert ol.lib().orc_sumcheck_cubic3(p64(claim), p64(taus), ctypes.c_size_t(ell), p64(a), p64(b), p64(c), tr.h, p64(polys), p64(r), p64(fin)) == 0
    return polys, r, fin


def oracle_quad_on(tr, claim, rounds, A, effA, B, effB):
    import ctypes

    polys = np.zeros((rounds, 2, 4), dtype=np.uint64)
    r = np.zeros((rounds, 4), dtype=np.uint64)
    fin = np.zeros((2, 4), dtype=np.uint64)
    a, b = A.copy(), B.copy()
    assert ol.lib().orc_sumcheck_quad(p64(claim), ctypes.c_size_t(rounds), p64(a), ctypes.c_size_t(effA[0]), ctypes.c_size_t(effA[1]), p64(b), ctypes.c_size_t(effB[0]),
                                      ctypes.c_size_t(effB[1]), tr.h, p64(polys), p64(r), p64(fin)) == 0
    return polys, r, fin


def test_the_transcript_taking_oracles_are_the_imported_ones():
    """oracle_cubic_on / oracle_quad_on differ from test_gpu_sumcheck's oracle_cubic / oracle_quad only in whose transcript they use"""
    rng = np.random.default_rng(SEED)
    A, B, C = satisfying_tables(rng, 8)
    taus, claim = rand_table(rng, 3), np.zeros(4, dtype=np.uint64)
    for a, b in zip(oracle_cubic(claim, taus, A, B, C)[:3], oracle_cubic_on(ol.Transcript(b"sc"), claim, taus, A, B, C)):
        assert (a == b).all()
    for a, b in zip(oracle_quad(claim, 3, A, FULL, B, FULL), oracle_quad_on(ol.Transcript(b"sq"), claim, 3, A, FULL, B, FULL)):
        assert (a == b).all()


def run_cubic(ctx, rng, ell, K, zero_tau_at=None, dishonest=None):
    n = 1 << ell
    sets = [satisfying_tables(rng, n) for _ in range(K)]
    taus = np.stack([rand_table(rng, ell) for _ in range(K)])
    claims = np.zeros((K, 4), dtype=np.uint64)  # A o B = C: the zero-check claim 0 is honest
    if zero_tau_at is not None:
        k, i = zero_tau_at
        taus[k, i] = 0
    if dishonest is not None:
        claims[dishonest] = rand_table(rng, 1)[0]
    gtr, otr = transcripts(ctx, b"sc", K)
    want = [oracle_cubic_on(otr[k], claims[k], taus[k], *sets[k]) for k in range(K)]
    tabs = [[hip.Table.from_host(ctx, x) for x in s] for s in sets]
    polys, r, fin = hip.sumcheck_cubic3_lockstep(ctx, claims, taus, [t[0] for t in tabs], [t[1] for t in tabs], [t[2] for t in tabs], gtr)
    for k in range(K):
        assert (r[k] == want[k][1]).all(), (ell, K, k)
        assert (polys[k] == want[k][0]).all(), (ell, K, k)
        assert (fin[k] == want[k][2]).all(), (ell, K, k)
        assert (gtr[k].squeeze(b"after") == otr[k].squeeze(b"after")).all()
        for j in range(3):  # element 0 of each bound table is the final claim; the tables are one element long
            assert tabs[k][j].info()[0] == 1 and (tabs[k][j].read(0, 1)[0] == fin[k][j]).all()


@pytest.mark.parametrize("ell", sorted(CUBIC_FORMS))
def test_cubic_lockstep_matches_oracle_per_instance(ctx, ell):
    rng = np.random.default_rng(SEED + ell)
    for K in ((1, 2, 3, 5) if ell <= 12 else (2,)):
        run_cubic(ctx, rng, ell, K)


def test_cubic_lockstep_max_instances(ctx):
    run_cubic(ctx, np.random.default_rng(SEED + 64), 3, hip.LOCKSTEP_MAX)


@pytest.mark.parametrize("ell", [7, 12])
def test_cubic_one_instance_takes_the_tau_zero_fallback_and_one_a_dishonest_claim(ctx, ell):
    """instance 1 has tau_2 = 0 (fallback_three_inputs in that round, its neighbours derive from the claim); instance 2 proves a claim that is not the
    sum: it must still equal the oracle and leave instances 0, 1, 3 as they are"""
    run_cubic(ctx, np.random.default_rng(SEED + 100 + ell), ell, 4, zero_tau_at=(1, 2), dishonest=2)
    run_cubic(ctx, np.random.default_rng(SEED + 200 + ell), ell, 3, zero_tau_at=(0, 0))


def run_quad(ctx, rng, rounds, K, eff=FULL, junk=False):
    n = 1 << rounds
    half = n // 2
    lo, hi = min(eff[0], half), min(eff[1], half)
    sets, host_sets = [], []
    for _ in range(K):
        A, B = rand_table(rng, n), rand_table(rng, n)
        for t in (A, B):
            t[lo:half] = 0
            t[half + hi :] = 0
        sets.append((A, B))
        if junk:  # what the device memory holds past the effective lengths: not zeros
            A, B = A.copy(), B.copy()
            for t in (A, B):
                if lo < half:
                    t[lo:half] = rand_table(rng, half - lo)
                if hi < half:
                    t[half + hi :] = rand_table(rng, half - hi)
        host_sets.append((A, B))
    claims = rand_table(rng, K)
    gtr, otr = transcripts(ctx, b"sq", K)
    want = [oracle_quad_on(otr[k], claims[k], rounds, sets[k][0], eff, sets[k][1], eff) for k in range(K)]
    tabs = [[hip.Table.from_host(ctx, x) for x in s] for s in host_sets]
    if eff != FULL:
        for ta, tb in tabs:
            ta.set_len(n, *eff)
            tb.set_len(n, *eff)
    polys, r, fin = hip.sumcheck_quad_lockstep(ctx, claims, rounds, [t[0] for t in tabs], [t[1] for t in tabs], gtr)
    for k in range(K):
        assert (r[k] == want[k][1]).all(), (rounds, K, k)
        assert (polys[k] == want[k][0]).all(), (rounds, K, k)
        assert (fin[k] == want[k][2]).all(), (rounds, K, k)
        assert (gtr[k].squeeze(b"after") == otr[k].squeeze(b"after")).all()
        for j in range(2):
            assert tabs[k][j].info()[0] == 1 and (tabs[k][j].read(0, 1)[0] == fin[k][j]).all()
    return host_sets, claims, want


@pytest.mark.parametrize("rounds", [1, 2, 5, 11, 13])
def test_quad_lockstep_dense_matches_oracle_per_instance(ctx, rounds):
    """rounds 1 .. 11: one block per instance in every round; 13: the first two rounds leave partials for k_ls_sum_partials"""
    rng = np.random.default_rng(SEED + 300 + rounds)
    for K in (1, 2, 3, 5):
        run_quad(ctx, rng, rounds, K)


@pytest.mark.parametrize("rounds,M,extra", [(11, 1024, 5), (13, 4096, 300)])
def test_quad_lockstep_zero_structure_like_the_inner_sumcheck_with_junk_past_the_effective_lengths(ctx, rounds, M, extra):
    """(lo_eff, hi_eff) = (M, extra) as prove sets them on poly_ABC and z (sp_table_set_len(abc, 2 M, M, num_extra)), with NON-ZERO junk in memory past
    the effective lengths: elements there count as zero whatever memory holds.
    Checked on the parent first, as the issue asks: sp_sumcheck_quad itself gives the oracle's answer on the same junk at these shapes (its kernels
    read the high halves only below hi_eff: k_eval_quad's `id < hiA`, the bind's `i < both` / `i < lo` branches) - asserted below on one instance, so
    the lockstep form is held to what the single prover already does."""
    rng = np.random.default_rng(SEED + 400 + rounds)
    host_sets, claims, want = run_quad(ctx, rng, rounds, 3, eff=(M, extra), junk=True)
    A, B = host_sets[0]
    ta, tb = hip.Table.from_host(ctx, A), hip.Table.from_host(ctx, B)
    ta.set_len(2 * M, M, extra)
    tb.set_len(2 * M, M, extra)
    got = hip.sumcheck_quad(ctx, claims[0], rounds, ta, tb, hip.Transcript(ctx, b"sq"))  # instance 0 has no extra absorbs
    for g, w in zip(got, want[0]):
        assert (g == w).all()


def test_quad_lockstep_instances_with_different_zero_structure(ctx):
    """the effective lengths are per table, not per call: here A and B of one instance differ"""
    rng = np.random.default_rng(SEED + 500)
    rounds, n = 9, 512
    effs = [((256, 7), (256, 256)), ((100, 30), (256, 3)), (FULL, (0, 200))]
    sets, claims = [], rand_table(rng, len(effs))
    gtr, otr = transcripts(ctx, b"sq", len(effs))
    want, tabs = [], []
    for k, (ea, eb) in enumerate(effs):
        A, B = rand_table(rng, n), rand_table(rng, n)
        for t, e in ((A, ea), (B, eb)):
            lo, hi = min(e[0], n // 2), min(e[1], n // 2)
            t[lo : n // 2] = 0
            t[n // 2 + hi :] = 0
        want.append(oracle_quad_on(otr[k], claims[k], rounds, A, ea, B, eb))
        ta, tb = hip.Table.from_host(ctx, A), hip.Table.from_host(ctx, B)
        ta.set_len(n, *ea)
        tb.set_len(n, *eb)
        tabs.append((ta, tb))
    polys, r, fin = hip.sumcheck_quad_lockstep(ctx, claims, rounds, [t[0] for t in tabs], [t[1] for t in tabs], gtr)
    for k in range(len(effs)):
        assert (polys[k] == want[k][0]).all() and (r[k] == want[k][1]).all() and (fin[k] == want[k][2]).all(), k


def test_refusals_leave_tables_and_transcripts_alone(ctx):
    rng = np.random.default_rng(SEED + 600)
    ell, n = 4, 16
    data = [rand_table(rng, n) for _ in range(6)]
    t = [hip.Table.from_host(ctx, x) for x in data]
    short = hip.Table.from_host(ctx, rand_table(rng, 8))
    odd = [hip.Table.from_host(ctx, rand_table(rng, 12)) for _ in range(6)]
    tr = [hip.Transcript(ctx, b"sc") for _ in range(2)]
    ref = hip.Transcript(ctx, b"sc")
    claims, taus = np.zeros((2, 4), dtype=np.uint64), np.stack([rand_table(rng, ell) for _ in range(2)])
    A, B, C = [t[0], t[1]], [t[2], t[3]], [t[4], t[5]]

    def refused(match, fn, *a):
        with pytest.raises(hip.SpartanHipError, match="rc=-1.*" + match):
            fn(ctx, *a)

    cub, quad = hip.sumcheck_cubic3_lockstep, hip.sumcheck_quad_lockstep
    refused("count", cub, claims, taus, [], [], [], [])
    refused("count", quad, claims, ell, [], [], [])
    big = hip.LOCKSTEP_MAX + 1
    refused("count", cub, np.zeros((big, 4), dtype=np.uint64), np.zeros((big, ell, 4), dtype=np.uint64), [t[0]] * big, [t[1]] * big, [t[2]] * big, [tr[0]] * big)
    refused("count", quad, np.zeros((big, 4), dtype=np.uint64), ell, [t[0]] * big, [t[1]] * big, [tr[0]] * big)
    refused("null", cub, claims, taus, A, [t[2], None], C, tr)
    refused("null", cub, claims, taus, A, B, C, [tr[0], None])
    refused("null", quad, claims, ell, [None, t[1]], B, tr)
    refused("null", quad, claims, ell, A, B, [None, tr[1]])
    L = hip._lockstep_lib()
    polys, r, fin = np.zeros((2, ell, 3, 4), dtype=np.uint64), np.zeros((2, ell, 4), dtype=np.uint64), np.zeros((2, 3, 4), dtype=np.uint64)
    hA, hB, hC, hT = hip._handles(A), hip._handles(B), hip._handles(C), hip._handles(tr)
    for args in ((ctx.h, 2, None, p64(taus), ell, hA, hB, hC, hT, p64(polys), p64(r), p64(fin)), (ctx.h, 2, p64(claims), None, ell, hA, hB, hC, hT, p64(polys), p64(r), p64(fin)),
                 (ctx.h, 2, p64(claims), p64(taus), ell, None, hB, hC, hT, p64(polys), p64(r), p64(fin)), (ctx.h, 2, p64(claims), p64(taus), ell, hA, hB, hC, None, p64(polys), p64(r), p64(fin)),
                 (ctx.h, 2, p64(claims), p64(taus), ell, hA, hB, hC, hT, None, p64(r), p64(fin)), (ctx.h, 2, p64(claims), p64(taus), ell, hA, hB, hC, hT, p64(polys), p64(r), None)):
        assert L.sp_sumcheck_cubic3_lockstep(*args) == -1 and b"null" in L.sp_last_error()
    for args in ((ctx.h, 2, None, ell, hA, hB, hT, p64(polys), p64(r), p64(fin)), (ctx.h, 2, p64(claims), ell, hA, None, hT, p64(polys), p64(r), p64(fin)),
                 (ctx.h, 2, p64(claims), ell, hA, hB, hT, p64(polys), None, p64(fin))):
        assert L.sp_sumcheck_quad_lockstep(*args) == -1 and b"null" in L.sp_last_error()
    refused("differing length", cub, claims, taus, A, [t[2], short], C, tr)
    refused("differing length", quad, claims, ell, [short, t[1]], B, tr)
    refused("2\\^rounds", cub, claims, np.stack([rand_table(rng, 3) for _ in range(2)]), A, B, C, tr)  # 16 elements, ell = 3
    refused("2\\^rounds", quad, claims, 5, A, B, tr)
    refused("2\\^rounds", cub, claims, taus, odd[:2], odd[2:4], odd[4:], tr)  # 12 elements
    refused("2\\^rounds", quad, claims, ell, odd[:2], odd[2:4], tr)
    refused("same table", cub, claims, taus, A, B, [t[4], t[0]], tr)
    refused("same table", cub, claims, taus, [t[0], t[0]], B, C, tr)
    refused("same table", quad, claims, ell, A, [t[2], t[1]], tr)
    refused("same transcript", cub, claims, taus, A, B, C, [tr[0], tr[0]])
    refused("same transcript", quad, claims, ell, A, B, [tr[1], tr[1]])
    for x, tab in zip(data, t):
        assert tab.info()[0] == n and (tab.read() == x).all()
    for q in tr:
        assert (q.clone().squeeze(b"x") == ref.clone().squeeze(b"x")).all()
    # and the very same arguments, unrefused, still prove
    gtr, otr = transcripts(ctx, b"sc", 2)
    polys, r, fin = cub(ctx, claims, taus, A, B, C, gtr)
    for k in range(2):
        w = oracle_cubic_on(otr[k], claims[k], taus[k], data[k], data[2 + k], data[4 + k])
        assert (polys[k] == w[0]).all() and (r[k] == w[1]).all() and (fin[k] == w[2]).all()
