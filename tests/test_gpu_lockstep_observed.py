"""GPU parity: sp_sumcheck_cubic3_lockstep_observed / sp_sumcheck_quad_lockstep_observed - the lockstep sum-checks that report every round's challenges to
a hook of the caller - against the CPU oracle per instance and against the plain lockstep calls: polynomials, challenges, final claims and the
transcripts' next squeeze are identical, with a hook, with a null hook, and with a hook that queues device work (sp_hyrax_prove_batch_rows on an open
job of the same context). The hook sees round 0 .. rounds - 1 once each, in order, and its r is out_r's column of that round.
rounds / ell 1 and 3: one block per instance does the whole round; 12: the first round leaves partials for k_ls_sum_partials (2 blocks an instance)."""
import numpy as np
import pytest

from spartan2_amd import hip
from test_gpu_hyrax_prove_batch import check as check_openings, generators, instances
from test_gpu_lockstep_sumcheck import FULL, SEED, oracle_cubic_on, oracle_quad_on, transcripts
from test_gpu_sumcheck import rand_table, satisfying_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


class Seen:
    def __init__(self, also=None):
        self.rounds, self.r, self.also = [], [], also

    def __call__(self, rnd, r):
        self.rounds.append(rnd)
        self.r.append(r)
        if self.also:
            self.also(rnd, r)

    def check(self, rounds, out_r):
        assert self.rounds == list(range(rounds))
        for i, r in enumerate(self.r):
            assert (r == out_r[:, i]).all(), i


def run_quad(ctx, rounds, K, also=None):
    rng = np.random.default_rng(SEED + 7000 + 10 * rounds + K)
    n = 1 << rounds
    sets = [(rand_table(rng, n), rand_table(rng, n)) for _ in range(K)]
    claims = rand_table(rng, K)
    results = []
    for form in ("plain", "hook", "null"):
        gtr, otr = transcripts(ctx, b"sq", K)
        tabs = [[hip.Table.from_host(ctx, x) for x in s] for s in sets]
        seen = Seen(also) if form == "hook" else None
        got = hip.sumcheck_quad_lockstep(ctx, claims, rounds, [t[0] for t in tabs], [t[1] for t in tabs], gtr, observe=seen, observed=form != "plain")
        if seen:
            seen.check(rounds, got[1])
        for k in range(K):
            want = oracle_quad_on(otr[k], claims[k], rounds, sets[k][0], FULL, sets[k][1], FULL)
            for g, w in zip(got, (want[0], want[1], want[2])):
                assert (g[k] == w).all(), (form, rounds, K, k)
            assert (gtr[k].squeeze(b"after") == otr[k].squeeze(b"after")).all(), (form, k)
        results.append(got)
    for got in results[1:]:
        for a, b in zip(results[0], got):
            assert (a == b).all()


def run_cubic(ctx, ell, K):
    rng = np.random.default_rng(SEED + 8000 + 10 * ell + K)
    sets = [satisfying_tables(rng, 1 << ell) for _ in range(K)]
    taus = np.stack([rand_table(rng, ell) for _ in range(K)])
    claims = np.zeros((K, 4), dtype=np.uint64)
    results = []
    for form in ("plain", "hook", "null"):
        gtr, otr = transcripts(ctx, b"sc", K)
        tabs = [[hip.Table.from_host(ctx, x) for x in s] for s in sets]
        seen = Seen() if form == "hook" else None
        got = hip.sumcheck_cubic3_lockstep(ctx, claims, taus, [t[0] for t in tabs], [t[1] for t in tabs], [t[2] for t in tabs], gtr, observe=seen,
                                           observed=form != "plain")
        if seen:
            seen.check(ell, got[1])
        for k in range(K):
            want = oracle_cubic_on(otr[k], claims[k], taus[k], *sets[k])
            for g, w in zip(got, (want[0], want[1], want[2])):
                assert (g[k] == w).all(), (form, ell, K, k)
            assert (gtr[k].squeeze(b"after") == otr[k].squeeze(b"after")).all(), (form, k)
        results.append(got)
    for got in results[1:]:
        for a, b in zip(results[0], got):
            assert (a == b).all()


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("rounds", [1, 3, 12])
def test_quad_observed_is_the_plain_form_and_the_oracle(ctx, rounds, K):
    run_quad(ctx, rounds, K)


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("ell", [1, 3, 12])
def test_cubic_observed_is_the_plain_form_and_the_oracle(ctx, ell, K):
    run_cubic(ctx, ell, K)


def test_a_hook_that_queues_the_row_stage_changes_no_sumcheck_output(ctx):
    """the driver's use: an opening is open on the context and the hook hands it its row points in round 1 of a 3-round sum-check; the sum-check still
    equals the oracle and the plain form (run_quad), and the opening finished afterwards equals the oracle's"""
    g, g_s = generators(b"ck", 2049), generators(b"ck_s", 2)
    key, key_s = hip.CommitmentKey(ctx, g[:2048], g[2048]), hip.CommitmentKey(ctx, g_s[:1], g_s[1])
    insts = instances(12, 5)[:3]
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts]
    job = hip.OpeningJob(ctx, key, key_s, [i.comm for i in insts], tables, insts[0].n, [i.blinds for i in insts], [i.tape for i in insts])
    calls = []

    def rows(rnd, _r):
        if rnd == 1:
            job.rows(np.stack([i.point[:1] for i in insts]))
            calls.append(rnd)

    try:
        run_quad(ctx, 3, 2, also=rows)
        assert calls == [1]
        trs = [i.transcript(ctx) for i in insts]
        out = job.finish(key, key_s, trs, [i.comm for i in insts], tables, insts[0].n, [i.blinds for i in insts], np.stack([i.point for i in insts]),
                         np.stack([i.comm_eval.reshape(8) for i in insts]), np.stack([i.b_ev.reshape(4) for i in insts]), [i.tape for i in insts])
        check_openings(insts, out, trs)
    finally:
        job.drop()
