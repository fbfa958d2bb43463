"""GPU parity: sp_hyrax_commit_batch - PCS::commit (hyrax_pc.rs:207-300) of the same segment of K polynomials on one key in one pass. Every polynomial's
rows must be WORD FOR WORD the oracle's (orc_hyrax_commit) and sp_hyrax_commit's on that polynomial alone: canonical affine coordinates, no tolerance.
The rows are built by hand so that every class of row (all zero, 0/1, values below 2^64, full field) meets every other at the same row index across
the polynomials of a batch. No case reaches comb_min_rows() digit rows: no test builds the comb table."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import lib as olib, p64, to_mont
from spartan2_amd import hip

pytestmark = pytest.mark.gpu
SEED = 0xC0BA7C
W = 2048
CLASSES = "ZBSF"  # all zero, 0/1, < 2^64, full field
SEGMENTS = {"3rows": 3 * W, "2rows+100": 2 * W + 100, "100": 100}
TAIL = 50  # elements of the table behind the segment


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def generators(label, n):
    g = np.zeros((n, 8), dtype=np.uint64)
    olib().orc_from_label(label, ctypes.c_size_t(n), p64(g))
    return g


@pytest.fixture(scope="module")
def key(ctx):
    g = generators(b"ck", W + 1)
    return hip.CommitmentKey(ctx, g[:W], g[W])


@pytest.fixture(scope="module")
def pool():
    """a few rows of every class, made once: polynomials are assembled from them"""
    rng = np.random.default_rng(SEED)
    one = to_mont(1)
    rows = {"Z": [np.zeros((W, 4), dtype=np.uint64)], "B": [], "S": [], "F": []}
    small = ol.mont_array([int(x) for x in rng.integers(2, 1 << 63, size=W)])
    full = ol.random_field_array(rng, W)
    for j in range(5):
        b = np.zeros((W, 4), dtype=np.uint64)
        b[rng.integers(0, 2, size=W) == 1] = one
        rows["B"].append(b)
        rows["S"].append(np.roll(small, 37 * j, axis=0))
        rows["F"].append(np.roll(full, 101 * j, axis=0))
    rows["S"][1][5:] = 0  # one small row with a single value and a zero tail
    return rows, ol.random_field_array(rng, 64), ol.random_field_array(rng, TAIL)


def classes_of(k, nrows, pattern):
    if pattern == "mixed":  # row r of polynomial k: every class meets every other at row 0 from K = 4 on; at most two digit rows a polynomial
        return [CLASSES[(k + r) % 4] for r in range(nrows)]
    return [("F" if k % 2 == 0 else "S")] * nrows  # "heavy": three digit rows of one class in a polynomial


_cache = {}


def polynomial(pool, k, n, pattern):
    """(elements (n, 4), blinds (rows, 4), the oracle's rows) of polynomial k for a segment of n elements - the same whatever batch it is part of"""
    keyid = (k, n, pattern)
    if keyid not in _cache:
        rows_pool, blind_pool, _ = pool
        nrows = (n + W - 1) // W
        cls = classes_of(k, nrows, pattern)
        v = np.concatenate([rows_pool[c][(k + r) % len(rows_pool[c])] for r, c in enumerate(cls)])[:n].copy()
        blinds = np.ascontiguousarray(blind_pool[(7 * k) % 32 : (7 * k) % 32 + nrows]).copy()
        for r, c in enumerate(cls):
            if c == "Z":
                blinds[r] = 0  # a zero row with a zero blind: the identity, written as (0, 0)
                break
        ok = ctypes.c_void_p(olib().orc_hyrax_setup(b"ck", ctypes.c_size_t(W)))
        want = np.zeros((nrows, 8), dtype=np.uint64)
        assert olib().orc_hyrax_commit(ok, p64(v), ctypes.c_size_t(n), p64(blinds), 0, p64(want)) == 0
        olib().orc_hyrax_free(ok)
        _cache[keyid] = (v, blinds, want, cls)
    return _cache[keyid]


def tables_of(ctx, pool, polys, off):
    junk = pool[2]
    return [hip.Table.from_host(ctx, np.concatenate([junk[:off], v, junk])) for v, _, _, _ in polys]


def check_batch(ctx, key, pool, K, n, off, pattern="mixed", singles=True):
    polys = [polynomial(pool, k, n, pattern) for k in range(K)]
    tabs = tables_of(ctx, pool, polys, off)
    got = hip.hyrax_commit_batch(ctx, key, tabs, off, n, [b for _, b, _, _ in polys])
    assert len(got) == K
    for k, (_, blinds, want, cls) in enumerate(polys):
        assert (got[k] == want).all(), f"polynomial {k} ({''.join(cls)}) differs from the oracle"
        if singles:
            assert (key.commit(tabs[k], off, n, blinds) == got[k]).all(), f"polynomial {k} differs from sp_hyrax_commit"
    return polys, got


@pytest.mark.parametrize("off", [0, 7])
@pytest.mark.parametrize("seg", sorted(SEGMENTS))
@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_batch_equals_oracle_and_single_calls(ctx, key, pool, K, seg, off):
    polys, got = check_batch(ctx, key, pool, K, SEGMENTS[seg], off)
    if seg == "3rows" and K == 5:
        # the batched digit path where the single calls take the latency path: at most two digit rows of a class in a polynomial, more in the batch
        cls = [p[3] for p in polys]
        assert all(c.count("F") <= 2 and c.count("S") <= 2 for c in cls) and sum(c.count("F") for c in cls) > 2 and sum(c.count("S") for c in cls) > 2
        # every class meets every other at row 0
        assert {c[0] for c in cls} == set(CLASSES)
        # the identity
        assert cls[0][0] == "Z" and not polys[0][1][0].any() and not got[0][0].any()


def test_a_polynomial_with_three_digit_rows(ctx, key, pool):
    polys, _ = check_batch(ctx, key, pool, 3, 3 * W, 7, pattern="heavy")
    assert polys[0][3] == ["F"] * 3 and polys[1][3] == ["S"] * 3


def test_batch_larger_than_one_chunk_of_workspace(ctx, key, pool):
    """two polynomials of three rows fit a chunk: five polynomials are three chunks (2, 2, 1)"""
    before = hip.hyrax_commit_batch_workspace()
    assert before == 1 << 23
    try:
        assert hip.hyrax_commit_batch_workspace(2 * 3 * W) == 2 * 3 * W
        check_batch(ctx, key, pool, 5, 3 * W, 7, singles=False)
        check_batch(ctx, key, pool, 5, 2 * W + 100, 0, singles=False)
        # a polynomial that alone exceeds the workspace: the single call per polynomial
        assert hip.hyrax_commit_batch_workspace(W) == W
        check_batch(ctx, key, pool, 2, 3 * W, 0, singles=False)
    finally:
        assert hip.hyrax_commit_batch_workspace(1 << 40) == 1 << 23  # (capped at the default)
    check_batch(ctx, key, pool, 5, 3 * W, 7, singles=False)


def test_narrow_key_takes_the_loop(ctx):
    """a 16-base key (per-base tables): K = 3 through the single-polynomial path"""
    g = generators(b"nk", 17)
    nkey = hip.CommitmentKey(ctx, g[:16], g[16])
    rng = np.random.default_rng(SEED + 16)
    n, K = 16 * 3 + 5, 3
    ok = ctypes.c_void_p(olib().orc_hyrax_setup(b"nk", ctypes.c_size_t(16)))
    vs, bls, wants = [], [], []
    for k in range(K):
        v = ol.random_field_array(rng, n)
        v[16 * ((k + 1) % 3) : 16 * ((k + 1) % 3) + 16] = 0  # a zero row, at another index in each
        v[:3] = to_mont(1)
        b = ol.random_field_array(rng, 4)
        want = np.zeros((4, 8), dtype=np.uint64)
        assert olib().orc_hyrax_commit(ok, p64(v), ctypes.c_size_t(n), p64(b), 0, p64(want)) == 0
        vs.append(v), bls.append(b), wants.append(want)
    olib().orc_hyrax_free(ok)
    tabs = [hip.Table.from_host(ctx, np.concatenate([np.zeros((5, 4), dtype=np.uint64), v])) for v in vs]
    got = hip.hyrax_commit_batch(ctx, nkey, tabs, 5, n, bls)
    for k in range(K):
        assert (got[k] == wants[k]).all()
        assert (nkey.commit(tabs[k], 5, n, bls[k]) == got[k]).all()


def test_refusals_leave_the_context_usable(ctx, key, pool):
    L = hip.lib()
    n, off, K = 100, 7, 2
    polys = [polynomial(pool, k + 1, n, "mixed") for k in range(K)]
    tabs = tables_of(ctx, pool, polys, off)
    short = hip.Table.from_host(ctx, polys[0][0][:60])
    bl = [p[1] for p in polys]
    outs = [np.zeros((1, 8), dtype=np.uint64) for _ in range(K)]
    sz = ctypes.c_size_t

    def arr_t(ts):
        return (ctypes.c_void_p * K)(*[t.h if t is not None else None for t in ts])

    def arr_u(xs):
        return (hip.c_u64p * K)(*[p64(x) if x is not None else None for x in xs])

    def call(count, t, o, nn, b, out):
        return L.sp_hyrax_commit_batch(ctx.h, key.h, sz(count), t, sz(o), sz(nn), b, out)

    cases = [
        ("count must be at least 1", lambda: call(0, arr_t(tabs), off, n, arr_u(bl), arr_u(outs))),
        ("null argument", lambda: call(K, None, off, n, arr_u(bl), arr_u(outs))),
        ("null argument", lambda: call(K, arr_t(tabs), off, n, arr_u(bl), None)),
        ("null table, polynomial 1", lambda: call(K, arr_t([tabs[0], None]), off, n, arr_u(bl), arr_u(outs))),
        ("null output, polynomial 0", lambda: call(K, arr_t(tabs), off, n, arr_u(bl), arr_u([None, outs[1]]))),
        ("range exceeds the table, polynomial 1", lambda: call(K, arr_t([tabs[0], short]), off, n, arr_u(bl), arr_u(outs))),
        ("range exceeds the table, polynomial 0", lambda: call(K, arr_t(tabs), off + (1 << 20), n, arr_u(bl), arr_u(outs))),
        ("null blinds", lambda: call(K, arr_t(tabs), off, n, None, arr_u(outs))),
        ("null blinds, polynomial 1", lambda: call(K, arr_t(tabs), off, n, arr_u([bl[0], None]), arr_u(outs))),
    ]
    for text, f in cases:
        assert f() == -1, text
        assert text.encode() in L.sp_last_error(), (text, L.sp_last_error())
        assert not any(o.any() for o in outs), "a refused call wrote rows"
        got = hip.hyrax_commit_batch(ctx, key, tabs, off, n, bl)  # a good call on the same context
        for k in range(K):
            assert (got[k] == polys[k][2]).all(), text
    # n == 0: nothing to commit, nothing written, no blinds needed
    assert call(K, arr_t(tabs), off, 0, None, arr_u(outs)) == 0 and not any(o.any() for o in outs)
