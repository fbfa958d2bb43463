"""GPU parity: the two batched ZK sum-checks of NeutronNova for `count` (step, core) pairs in lockstep (sp_sumcheck_cubic_outer_pow_batched_lockstep,
sp_sumcheck_quad_batched_lockstep). Every pair is held to the oracle's restatement on its own tables with its own transcript hook AND to the existing
single call (sp_sumcheck_cubic_outer_pow_batched / sp_sumcheck_quad_batched) on copies: the coefficients handed to the hook, the challenges, the final
claims, element 0 of every bound table and base_tau. Then the hook call order, a failing hook, and every refusal."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu
P = ol.MODULI[0]
PAIRS_MAX = 32
POOL = 1 << 14


@pytest.fixture(scope="module")
def ctx():
    from spartan2_amd import hip

    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """random field elements, made once: table j of a test is a window of the pool starting at an offset of its own"""
    return ol.random_field_array(np.random.default_rng(20261020), POOL)


def window(pool, j, n):
    at = (j * 389 + 17) % (POOL - n + 1)
    return pool[at : at + n].copy()


def recording(hook, log, pair):
    def h(rnd, cs, cc):
        r = hook(rnd, cs, cc)
        log.append((pair, rnd, cs.copy(), cc.copy(), np.asarray(r).copy()))
        return r

    return h


def same_log(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[1] == y[1]
        for u, v in zip(x[2:], y[2:]):
            assert (u == v).all(), (x[0], x[1])


# ---- cubic with the split power table -------------------------------------------------------------------------------------------------------------------
def cubic_pair(pool, num_rounds, p, satisfying_core=True):
    """pair p: its own tau, random step tables, core with C = A o B (or not)"""
    n = 1 << num_rounds
    ell, left, right = ol.tensor_decomp(n)
    tau = window(pool, 1000 + p, 1)[0]
    E = ol.pow_split_evals(tau, ell, left, right)
    step = [window(pool, 10 * p + m, n) for m in range(3)]
    core = [window(pool, 10 * p + 3 + m, n) for m in range(3)]
    if satisfying_core:
        a, b = ol.ints_of(core[0]), ol.ints_of(core[1])
        core[2] = ol.mont_array([x * y % P for x, y in zip(a, b)])
    e = ol.ints_of(E)
    sa, sb, sc = (ol.ints_of(t) for t in step)
    t_out = ol.to_mont(sum(e[k % left] * e[left + k // left] % P * ((sa[k] * sb[k] - sc[k]) % P) for k in range(n)) % P)
    return dict(pl=E[:left].copy(), pr=E[left:].copy(), step=step, core=core, t_out=t_out)


_cubic_cache = {}


def cubic_case(pool, num_rounds, count):
    """the pairs of a case with the oracle's answers (computed once per pair): pair 1 of a case of three has a core that does not satisfy"""
    out = []
    for p in range(count):
        sat = not (count == 3 and p == 1)
        key = (num_rounds, p, sat)
        if key not in _cubic_cache:
            pr = cubic_pair(pool, num_rounds, p, sat)
            log = []
            hook = recording(ol.batched_transcript_hook(ol.Transcript(b"c%d" % p)), log, p)
            pr["want"] = ol.prove_cubic_outer_pow_batched(num_rounds, pr["pl"], pr["pr"], pr["step"], pr["core"], pr["t_out"], 3, hook)
            pr["want_log"] = log
            _cubic_cache[key] = pr
        out.append(_cubic_cache[key])
    return out


def upload_cubic(ctx, pr):
    from spartan2_amd import hip

    return (hip.Table.from_host(ctx, pr["pl"]), hip.Table.from_host(ctx, pr["pr"]), [hip.Table.from_host(ctx, t) for t in pr["step"]],
            [hip.Table.from_host(ctx, t) for t in pr["core"]])


@pytest.mark.parametrize("num_rounds,count", [(nr, c) for nr in (2, 5, 12) for c in (1, 2, 3)] + [(5, PAIRS_MAX)])
def test_cubic_outer_pow_batched_lockstep(ctx, pool, num_rounds, count):
    from spartan2_amd import hip

    assert hip.LOCKSTEP_PAIRS_MAX == PAIRS_MAX
    pairs = cubic_case(pool, num_rounds, count)
    dev = [upload_cubic(ctx, pr) for pr in pairs]
    logs = [[] for _ in pairs]
    hooks = [recording(ol.batched_transcript_hook(ol.Transcript(b"c%d" % p)), logs[p], p) for p in range(count)]
    got_r = hip.sumcheck_cubic_outer_pow_batched_lockstep(ctx, num_rounds, [d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev], [d[3] for d in dev],
                                                          np.stack([pr["t_out"] for pr in pairs]), 3, hooks)
    for p, pr in enumerate(pairs):
        want_r, want_fin, want_base = pr["want"]
        tl, tr_, ts, tc = dev[p]
        assert (got_r[p] == want_r).all(), p
        got_fin = np.stack([t.read(0, 1)[0] for t in ts + tc])
        assert (got_fin == want_fin).all(), p
        assert (tl.read(0, 1)[0] == want_base).all(), p
        same_log(logs[p], pr["want_log"])
        if p < 3:  # the existing single call on copies (every pair of the small cases, the first three of the full argument block)
            sl, sr, ss, sc = upload_cubic(ctx, pr)
            slog = []
            one_r = hip.sumcheck_cubic_outer_pow_batched(ctx, num_rounds, sl, sr, ss, sc, pr["t_out"], 3,
                                                         recording(ol.batched_transcript_hook(ol.Transcript(b"c%d" % p)), slog, p))
            assert (one_r == got_r[p]).all()
            assert (np.stack([t.read(0, 1)[0] for t in ss + sc]) == got_fin).all()
            assert (sl.read(0, 1)[0] == tl.read(0, 1)[0]).all()
            same_log(slog, logs[p])


# ---- quadratic --------------------------------------------------------------------------------------------------------------------------------------------
def quad_pair(pool, num_rounds, p):
    """pair p: tables A0 A1 B0 B1 with the zero structure of poly_ABC / z where there is room for it -> (the tables as the oracle sees them, what device
    memory holds: junk past the effective lengths, (lo_eff, hi_eff) or None, the claims)"""
    n = 1 << num_rounds
    half = n // 2
    T = [window(pool, 7 * p + m, n) for m in range(4)]
    eff = None
    if num_rounds >= 4:
        eff = (half - 1 - p % 3, max(1, half // 8) + p % 2)  # (lo_eff, hi_eff): odd, differing between pairs
        for t in T:
            t[eff[0] : half] = 0
            t[half + eff[1] :] = 0
    mem = [t.copy() for t in T]
    if eff:
        for m, t in enumerate(mem):
            t[eff[0] : half] = window(pool, 500 + m, half - eff[0])
            t[half + eff[1] :] = window(pool, 600 + m, half - eff[1])
    claims = np.stack([window(pool, 2000 + 2 * p, 1)[0], window(pool, 2001 + 2 * p, 1)[0]])
    return dict(T=T, mem=mem, eff=eff, claims=claims)


_quad_cache = {}


def quad_case(pool, num_rounds, count):
    out = []
    for p in range(count):
        key = (num_rounds, p)
        if key not in _quad_cache:
            pr = quad_pair(pool, num_rounds, p)
            log = []
            pr["want"] = ol.prove_quad_batched(pr["claims"], num_rounds, *pr["T"], 7, recording(ol.batched_transcript_hook(ol.Transcript(b"q%d" % p)), log, p))
            pr["want_log"] = log
            _quad_cache[key] = pr
        out.append(_quad_cache[key])
    return out


def upload_quad(ctx, pr, num_rounds):
    from spartan2_amd import hip

    tabs = [hip.Table.from_host(ctx, t) for t in pr["mem"]]
    if pr["eff"]:
        for t in tabs:
            t.set_len(1 << num_rounds, *pr["eff"])
    return tabs


@pytest.mark.parametrize("num_rounds,count", [(nr, c) for nr in (1, 4, 12, 13) for c in (1, 2, 3, PAIRS_MAX)])
def test_quad_batched_lockstep(ctx, pool, num_rounds, count):
    from spartan2_amd import hip

    pairs = quad_case(pool, num_rounds, count)
    dev = [upload_quad(ctx, pr, num_rounds) for pr in pairs]
    logs = [[] for _ in pairs]
    hooks = [recording(ol.batched_transcript_hook(ol.Transcript(b"q%d" % p)), logs[p], p) for p in range(count)]
    got_r, got_fin = hip.sumcheck_quad_batched_lockstep(ctx, np.stack([pr["claims"] for pr in pairs]), num_rounds, [d[0] for d in dev], [d[1] for d in dev],
                                                        [d[2] for d in dev], [d[3] for d in dev], 7, hooks)
    for p, pr in enumerate(pairs):
        want_r, want_fin = pr["want"]
        assert (got_r[p] == want_r).all(), p
        assert (got_fin[p] == want_fin).all(), p
        assert (np.stack([t.read(0, 1)[0] for t in dev[p]]) == want_fin).all(), p
        same_log(logs[p], pr["want_log"])
        if p < 3:
            tabs = upload_quad(ctx, pr, num_rounds)
            slog = []
            one_r, one_fin = hip.sumcheck_quad_batched(ctx, pr["claims"], num_rounds, *tabs, 7, recording(ol.batched_transcript_hook(ol.Transcript(b"q%d" % p)), slog, p))
            assert (one_r == got_r[p]).all() and (one_fin == got_fin[p]).all()
            assert (np.stack([t.read(0, 1)[0] for t in tabs]) == got_fin[p]).all()
            same_log(slog, logs[p])


# ---- the hooks ----------------------------------------------------------------------------------------------------------------------------------------------
def test_hooks_run_rounds_ascending_and_pairs_ascending_within_a_round(ctx, pool):
    from spartan2_amd import hip

    order = []

    def hook_of(p, tr):
        inner = ol.batched_transcript_hook(tr)

        def h(rnd, cs, cc):
            order.append((rnd, p))
            return inner(rnd, cs, cc)

        return h

    nr, count = 5, 3
    cub = [upload_cubic(ctx, pr) for pr in cubic_case(pool, nr, count)]
    hip.sumcheck_cubic_outer_pow_batched_lockstep(ctx, nr, [d[0] for d in cub], [d[1] for d in cub], [d[2] for d in cub], [d[3] for d in cub],
                                                  np.stack([pr["t_out"] for pr in cubic_case(pool, nr, count)]), 3,
                                                  [hook_of(p, ol.Transcript(b"o")) for p in range(count)])
    assert order == [(3 + i, p) for i in range(nr) for p in range(count)]
    order.clear()
    pairs = quad_case(pool, 4, count)
    dev = [upload_quad(ctx, pr, 4) for pr in pairs]
    hip.sumcheck_quad_batched_lockstep(ctx, np.stack([pr["claims"] for pr in pairs]), 4, [d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev],
                                       [d[3] for d in dev], 7, [hook_of(p, ol.Transcript(b"o")) for p in range(count)])
    assert order == [(7 + j, p) for j in range(4) for p in range(count)]


@pytest.mark.parametrize("kind", ["cubic", "quad"])
def test_a_failing_hook_ends_the_call_with_its_code_and_no_hook_runs_after_it(ctx, pool, kind):
    from spartan2_amd import hip

    calls = []

    def hook_of(p):
        inner = ol.batched_transcript_hook(ol.Transcript(b"f"))

        def h(rnd, cs, cc):
            calls.append((rnd, p))
            if (rnd, p) == (1, 1):
                return -7
            return inner(rnd, cs, cc)

        return h

    hooks = [hook_of(p) for p in range(3)]
    with pytest.raises(hip.SpartanHipError, match=r"rc=-7: .*the round hook failed, pair 1"):
        if kind == "cubic":
            pairs = cubic_case(pool, 5, 3)
            dev = [upload_cubic(ctx, pr) for pr in pairs]
            hip.sumcheck_cubic_outer_pow_batched_lockstep(ctx, 5, [d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev], [d[3] for d in dev],
                                                          np.stack([pr["t_out"] for pr in pairs]), 0, hooks)
        else:
            pairs = quad_case(pool, 4, 3)
            dev = [upload_quad(ctx, pr, 4) for pr in pairs]
            hip.sumcheck_quad_batched_lockstep(ctx, np.stack([pr["claims"] for pr in pairs]), 4, [d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev],
                                               [d[3] for d in dev], 0, hooks)
    assert calls == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_tables_alone(ctx, pool):
    from spartan2_amd import hip

    L = hip._batched_lockstep_lib()
    sz = ctypes.c_size_t
    nr, n = 4, 16
    ell, left, right = ol.tensor_decomp(n)
    data = {}
    called = []

    def tab(name, length):
        data[name] = window(pool, len(data), length)
        return hip.Table.from_host(ctx, data[name])

    pl = [tab("pl%d" % p, left) for p in range(2)]
    pr = [tab("pr%d" % p, right) for p in range(2)]
    six = [[tab("t%d_%d" % (m, p), n) for p in range(2)] for m in range(6)]
    short = tab("short", 8)
    wide = tab("wide", 2 * left)
    everything = dict(zip(list(data), pl + pr + [t for col in six for t in col] + [short, wide]))

    def hook(rnd, cs, cc):
        called.append(rnd)
        return np.zeros(4, dtype=np.uint64)

    cb, users = hip._pair_hooks([hook, hook])
    t_out, claims = np.zeros((2, 4), dtype=np.uint64), np.zeros((2, 2, 4), dtype=np.uint64)
    out_r, fin = np.zeros((2, nr, 4), dtype=np.uint64), np.zeros((2, 4, 4), dtype=np.uint64)
    H = hip._handles

    def cubic(count=2, rounds=nr, pow_left=pl, pow_right=pr, cols=six, t=hip.p64(t_out), hk=cb, us=users, r=hip.p64(out_r), c=ctx.h):
        arrs = [None if col is None else H(col) for col in cols]
        return L.sp_sumcheck_cubic_outer_pow_batched_lockstep(c, sz(count), sz(rounds), None if pow_left is None else H(pow_left), None if pow_right is None else H(pow_right),
                                                              *arrs, t, sz(0), hk, us, r)

    def quad(count=2, rounds=nr, cols=six[:4], cl=hip.p64(claims), hk=cb, us=users, r=hip.p64(out_r), f=hip.p64(fin), c=ctx.h):
        arrs = [None if col is None else H(col) for col in cols]
        return L.sp_sumcheck_quad_batched_lockstep(c, sz(count), cl, sz(rounds), *arrs, sz(0), hk, us, r, f)

    def swapped(cols, m, p, t):
        out = [list(col) for col in cols]
        out[m][p] = t
        return out

    def nulled(cols, m):
        return [None if i == m else col for i, col in enumerate(cols)]

    null_hook = hip.ROUND_HOOK()
    many = lambda col: [col[0]] * (PAIRS_MAX + 1)
    cases = [
        ("count must be 1 .. SP_LOCKSTEP_PAIRS_MAX", lambda: cubic(count=0)),
        ("count must be 1 .. SP_LOCKSTEP_PAIRS_MAX", lambda: cubic(count=PAIRS_MAX + 1, pow_left=many(pl), pow_right=many(pr), cols=[many(col) for col in six])),
        ("count must be 1 .. SP_LOCKSTEP_PAIRS_MAX", lambda: quad(count=0)),
        ("count must be 1 .. SP_LOCKSTEP_PAIRS_MAX", lambda: quad(count=PAIRS_MAX + 1, cols=[many(col) for col in six[:4]])),
        ("null hook", lambda: cubic(hk=null_hook)),
        ("null hook", lambda: quad(hk=null_hook)),
        ("null argument", lambda: cubic(c=None)),
        ("null argument", lambda: cubic(pow_left=None)),
        ("null argument", lambda: cubic(pow_right=None)),
        ("null argument", lambda: cubic(t=None)),
        ("null argument", lambda: cubic(us=None)),
        ("null argument", lambda: cubic(r=None)),
        ("null argument", lambda: quad(c=None)),
        ("null argument", lambda: quad(cl=None)),
        ("null argument", lambda: quad(us=None)),
        ("null argument", lambda: quad(r=None)),
        ("null argument", lambda: quad(f=None)),
        ("null table, pair 1", lambda: cubic(pow_left=[pl[0], None])),
        ("null table, pair 0", lambda: cubic(pow_right=[None, pr[1]])),
        ("tables must have 2^num_rounds elements", lambda: cubic(rounds=0)),
        ("tables must have 2^num_rounds elements", lambda: cubic(rounds=3)),
        ("tables must have 2^num_rounds elements", lambda: quad(rounds=5)),
        ("tables must have 2^num_rounds elements, pair 1", lambda: cubic(cols=swapped(six, 2, 1, short))),
        ("tables must have 2^num_rounds elements, pair 1", lambda: quad(cols=swapped(six[:4], 3, 1, short))),
        ("pow tables must factor 2^num_rounds, pair 1", lambda: cubic(pow_left=[pl[0], wide])),
        ("pow tables must factor 2^num_rounds, pair 0", lambda: cubic(pow_right=[short if right != 8 else wide, pr[1]])),
        ("the same table twice, pairs 0 and 1", lambda: cubic(cols=swapped(six, 4, 1, six[4][0]))),
        ("the same table twice, pairs 0 and 0", lambda: cubic(cols=swapped(six, 1, 0, six[0][0]))),
        ("the same table twice, pairs 0 and 1", lambda: cubic(pow_left=[pl[0], pl[0]])),
        ("the same table twice, pairs 0 and 1", lambda: quad(cols=swapped(six[:4], 0, 1, six[2][0]))),
    ]
    cases += [("null argument", lambda m=m: cubic(cols=nulled(six, m))) for m in range(6)]
    cases += [("null table, pair 1", lambda m=m: cubic(cols=swapped(six, m, 1, None))) for m in range(6)]
    cases += [("null argument", lambda m=m: quad(cols=nulled(six[:4], m))) for m in range(4)]
    cases += [("null table, pair 0", lambda m=m: quad(cols=swapped(six[:4], m, 0, None))) for m in range(4)]
    for want, call in cases:
        assert call() == -1, want
        msg = hip.lib().sp_last_error().decode()
        assert want in msg and "(lockstep)" in msg, (want, msg)
    assert not called
    assert not out_r.any() and not fin.any()
    for name, t in everything.items():
        assert len(t) == data[name].shape[0], name
        assert (t.read() == data[name]).all(), name
    # and the same arguments, unrefused, run
    assert cubic() == 0 and len(called) == 2 * nr
