"""GPU parity on EDGE-VALUED tables: the sum-check provers (single and lockstep), bind_top, the eq table, the dot product, the matrix-vector product and
the round-0 products path through the C ABI against the CPU oracle, bit-exact. The other GPU tests fill their tables with ol.random_field_array; such
values never take the rare branch of the scalar field's reduction (tests/edge_values.py), never bring a lazy sum near its upper range (raw limbs
average p / 2) and never leave one wave of k_eval_products_stream with an all-zero P0 next to one without. Here every table is drawn from a palette of
0, 1, -1 and the raw limb patterns p - 1, (p - 1) / 2 and 2^255. Claims are dishonest throughout: parity, not soundness, is what is checked."""
import ctypes

import numpy as np
import pytest

import edge_values as ev
import oracle_lib as ol
from oracle_lib import lib as olib, p64
from spartan2_amd import frontend, hip, host
from test_gpu_lockstep_sumcheck import oracle_cubic_on, oracle_quad_on, transcripts
from test_gpu_sumcheck import oracle_bind, oracle_cubic, oracle_quad

pytestmark = pytest.mark.gpu

SEED = 0xED6E
FULL = (hip.SIZE_MAX, hip.SIZE_MAX)
ZERO, ONE, MINUS_ONE, RAW_MAX = np.zeros(4, dtype=np.uint64), ev.mont(1), ev.mont(ev.P - 1), ev.raw_max()
EDGE_SCALARS = {"0": ZERO, "1": ONE, "-1": MINUS_ONE, "raw p-1": RAW_MAX}

# "one_x_max": A = Montgomery one, B = raw p - 1: every product A[i] B[i] has the raw limbs p - 1, so the lazy 9-word sums are as large as they get
PATTERNS = ["one_x_max", "all_max", "lo_zero_hi_max", "lo_max_hi_zero", "mix"]
ELLS = [4, 10, 13, 16]  # 4: single-block tail and host hand-over; 10, 13, 16: block partials and the multi-block tail
ELL_STREAM = 20         # the smallest size at which k_eval_*_stream and k_bind_eval_*_stream both run: q = len / 4 = 2^18 = STREAM_MIN_Q


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def rng_for(*key):
    return np.random.default_rng([SEED, *key])


def rand_elem(rng):
    return ev.random_rows(rng, 1)[0]


def tables(pattern, rng, n, count=3):
    """`count` tables of n rows"""
    half = n // 2
    if pattern == "one_x_max":
        out = [ev.constant_table(n, ONE), ev.constant_table(n, RAW_MAX), np.zeros((n, 4), dtype=np.uint64)]
    elif pattern == "all_max":
        out = [ev.constant_table(n, RAW_MAX) for _ in range(3)]
    elif pattern == "all_zero":
        out = [np.zeros((n, 4), dtype=np.uint64) for _ in range(3)]
    elif pattern in ("lo_zero_hi_max", "lo_max_hi_zero"):
        t = ev.constant_table(n, RAW_MAX)
        if pattern == "lo_zero_hi_max":
            t[:half] = 0
        else:
            t[half:] = 0
        out = [t.copy() for _ in range(3)]
    else:
        pal = ev.palette(rng)
        out = [ev.palette_table(rng, n, pal, weights=[3] * 6 + [1] * (len(pal) - 6)) for _ in range(3)]
    return out[:count]


def to_device(ctx, tabs):
    return [hip.Table.from_host(ctx, t) for t in tabs]


# ---- the single provers ----------------------------------------------------------------------------------------------------------------------------
def check_cubic(ctx, rng, ell, A, B, C, taus=None):
    taus = ev.random_rows(rng, ell) if taus is None else taus
    claim = rand_elem(rng)
    want_polys, want_r, want_fin, otr = oracle_cubic(claim, taus, A, B, C)
    tr = hip.Transcript(ctx, b"sc")
    polys, r, fin = hip.sumcheck_cubic3(ctx, claim, taus, *to_device(ctx, (A, B, C)), tr)
    assert (r == want_r).all()
    assert (polys == want_polys).all()
    assert (fin == want_fin).all()
    assert (tr.squeeze(b"after") == otr.squeeze(b"after")).all()


def check_quad(ctx, rng, rounds, A, B, eff=FULL):
    claim = rand_elem(rng)
    want = oracle_quad(claim, rounds, A, eff, B, eff)
    ta, tb = (hip.Table.from_host(ctx, t, *eff) for t in (A, B))
    got = hip.sumcheck_quad(ctx, claim, rounds, ta, tb, hip.Transcript(ctx, b"sq"))
    for g, w in zip(got, want):
        assert (g == w).all()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("ell", ELLS)
def test_cubic_on_edge_tables(ctx, ell, pattern):
    rng = rng_for(1, ell, PATTERNS.index(pattern))
    check_cubic(ctx, rng, ell, *tables(pattern, rng, 1 << ell))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("ell", ELLS)
def test_quad_on_edge_tables(ctx, ell, pattern):
    rng = rng_for(2, ell, PATTERNS.index(pattern))
    check_quad(ctx, rng, ell, *tables(pattern, rng, 1 << ell, 2))


def test_cubic_streaming_kernels_on_a_palette_mix(ctx):
    rng = rng_for(3)
    check_cubic(ctx, rng, ELL_STREAM, *tables("mix", rng, 1 << ELL_STREAM))


def test_quad_streaming_kernels_on_the_largest_lazy_sums(ctx):
    """2^19 products of raw limbs p - 1 per accumulator: 256 per block partial, 2^11 partials in k_sum_partials_lazy"""
    rng = rng_for(4)
    check_quad(ctx, rng, ELL_STREAM, *tables("one_x_max", rng, 1 << ELL_STREAM, 2))


def test_quad_sparse_streaming_kernel_on_a_palette_mix(ctx):
    """the inner sum-check's zero structure (M, extra) = (2^19, 257): round 0 in k_eval_quad_stream, the first bind in k_bind_eval_quad_stream_sparse"""
    rng = rng_for(5)
    M, extra = 1 << 19, 257
    A, B = tables("mix", rng, 2 * M, 2)
    A[M + extra :] = 0
    B[M + extra :] = 0
    check_quad(ctx, rng, 20, A, B, eff=(M, extra))


TAU_VALUES = ["0", "1", "-1"]


@pytest.mark.parametrize("which", TAU_VALUES + ["rotating"])
@pytest.mark.parametrize("ell", [6, 13])
def test_cubic_with_edge_taus(ctx, ell, which):
    """tau = 0 (the three-sum fallback), 1 (eq(tau, 0) = 0) and -1 at the first, a middle and the last round, the other rounds random; "rotating" puts
    one of each at those three rounds"""
    rng = rng_for(6, ell, (TAU_VALUES + ["rotating"]).index(which))
    taus = ev.random_rows(rng, ell)
    at = (0, ell // 2, ell - 1)
    for j, i in enumerate(at):
        taus[i] = EDGE_SCALARS[TAU_VALUES[j] if which == "rotating" else which]
    check_cubic(ctx, rng, ell, *tables("mix", rng, 1 << ell), taus=taus)


# ---- the lockstep provers: one instance constant-max, one all-zero, one a palette mix ----------------------------------------------------------------
@pytest.mark.parametrize("ell", [7, 12])
def test_cubic_lockstep_on_edge_tables(ctx, ell):
    rng = rng_for(7, ell)
    n, K = 1 << ell, 3
    sets = [tables(p, rng, n) for p in ("one_x_max", "all_zero", "mix")]
    taus = np.stack([ev.random_rows(rng, ell) for _ in range(K)])
    claims = ev.random_rows(rng, K)
    gtr, otr = transcripts(ctx, b"sc", K)
    want = [oracle_cubic_on(otr[k], claims[k], taus[k], *sets[k]) for k in range(K)]
    tabs = [to_device(ctx, s) for s in sets]
    polys, r, fin = hip.sumcheck_cubic3_lockstep(ctx, claims, taus, [t[0] for t in tabs], [t[1] for t in tabs], [t[2] for t in tabs], gtr)
    for k in range(K):
        assert (r[k] == want[k][1]).all(), k
        assert (polys[k] == want[k][0]).all(), k
        assert (fin[k] == want[k][2]).all(), k
        assert (gtr[k].squeeze(b"after") == otr[k].squeeze(b"after")).all()


@pytest.mark.parametrize("rounds", [7, 12])
def test_quad_lockstep_on_edge_tables(ctx, rounds):
    rng = rng_for(8, rounds)
    n, K = 1 << rounds, 3
    sets = [tables(p, rng, n, 2) for p in ("one_x_max", "all_zero", "mix")]
    claims = ev.random_rows(rng, K)
    gtr, otr = transcripts(ctx, b"sq", K)
    want = [oracle_quad_on(otr[k], claims[k], rounds, sets[k][0], FULL, sets[k][1], FULL) for k in range(K)]
    tabs = [to_device(ctx, s) for s in sets]
    polys, r, fin = hip.sumcheck_quad_lockstep(ctx, claims, rounds, [t[0] for t in tabs], [t[1] for t in tabs], gtr)
    for k in range(K):
        assert (r[k] == want[k][1]).all(), k
        assert (polys[k] == want[k][0]).all(), k
        assert (fin[k] == want[k][2]).all(), k
        assert (gtr[k].squeeze(b"after") == otr[k].squeeze(b"after")).all()


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(EDGE_SCALARS))
@pytest.mark.parametrize("logn", [1, 7, 15])
def test_bind_top_with_edge_challenges(ctx, logn, which):
    rng = rng_for(9, logn)
    n, r = 1 << logn, EDGE_SCALARS[which]
    for pattern in ("mix", "all_max", "lo_zero_hi_max", "lo_max_hi_zero"):
        Z = tables(pattern, rng, n, 1)[0]
        t = hip.Table.from_host(ctx, Z)
        t.bind_top(r)
        want, lo, hi = oracle_bind(Z, hip.SIZE_MAX, hip.SIZE_MAX, r)
        assert t.info() == (n // 2, lo, hi), pattern
        assert (t.read() == want).all(), pattern


@pytest.mark.parametrize("ell", [1, 10, 11, 16])
def test_eq_table_with_edge_points(ctx, ell):
    rng = rng_for(10, ell)
    edge = np.stack([EDGE_SCALARS[k] for k in sorted(EDGE_SCALARS)])
    points = [np.stack([e]) for e in edge] if ell == 1 else []
    if ell > 1:
        for _ in range(3):  # every edge value somewhere, the rest drawn from the edge values and two random elements
            r = ev.palette_table(rng, ell, np.concatenate([edge, ev.random_rows(rng, 2)]))
            r[rng.permutation(ell)[: len(edge)]] = edge
            points.append(r)
        points.append(np.ascontiguousarray(np.tile(MINUS_ONE, (ell, 1))))
        points.append(np.ascontiguousarray(np.tile(RAW_MAX, (ell, 1))))
    for r in points:
        want = np.zeros((1 << ell, 4), dtype=np.uint64)
        olib().orc_eq_evals(p64(r), ctypes.c_size_t(ell), p64(want))
        assert (hip.Table.eq(ctx, r).read() == want).all()


@pytest.mark.parametrize("n", [1, 1000, 5000])
def test_table_dot_on_constant_max_tables(ctx, n):
    for a_row, b_row in ((ONE, RAW_MAX), (RAW_MAX, RAW_MAX), (MINUS_ONE, RAW_MAX)):
        a, b = ev.constant_table(n, a_row), ev.constant_table(n, b_row)
        want = np.zeros(4, dtype=np.uint64)
        olib().orc_field_dot(0, p64(a), p64(b), ctypes.c_size_t(n), p64(want))
        assert (hip.table_dot(ctx, hip.Table.from_host(ctx, a), hip.Table.from_host(ctx, b), n) == want).all()


def test_multiply_vec_on_a_palette_z(ctx):
    inst = frontend.synthetic_circuit(40, 77, num_public=3, shared_permille=200, precommitted_permille=500)
    mats, dims = host.pad_shape(inst)
    oshape = ol.OracleShape(inst)
    shape = hip.Shape(ctx, mats, dims)
    N, ncols = dims["num_cons"], oshape.num_vars + oshape.num_extra
    rng = rng_for(11)
    pal = ev.palette(rng)
    for weights in (None, [0, 0, 0, 1] + [0] * (len(pal) - 4), [6] * 6 + [1] * (len(pal) - 6)):  # a mix, every entry raw p - 1, mostly edge values
        z = ev.palette_table(rng, ncols, pal, weights)
        got = [hip.Table.zeros(ctx, N) for _ in range(3)]
        shape.multiply_vec(hip.Table.from_host(ctx, z), *got)
        want = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
        assert olib().orc_shape_multiply_vec(oshape.h, p64(z), *(p64(w) for w in want)) == 0
        for g, w in zip(got, want):
            assert (g.read(0, N) == w).all()


# ---- the products path: round 1's per-pair products P0 = A o B - C (low half), P1 = (A_hi - A_lo) o (B_hi - B_lo) supplied -----------------------------
# k_eval_products_stream skips the P0 accumulator of a wave whose P0 entries are all zero. A lane of the PPT-chunk form holds the entries
# block * 256 PPT + k * 256 + thread, k < PPT, so a wave's entries are PPT runs of 64. The form with PPT = 4 needs half >= 2^16, half % 1024 == 0 and, with
# the factored eq tables of round 1, 2^s >= 1024 for s = ell - ell / 2: that is ell >= 19. At ell = 17 (s = 9) and below the blocks hold one chunk.
PRODUCT_ELLS = [12, 17, 19]
ZERO_PATTERNS = ["all_zero", "none_zero", "alternating_runs", "lane_0", "lane_63", "last_chunk"]


def products_ppt(ell):
    return 4 if ell >= 19 else 1


@pytest.fixture(scope="module")
def product_base():
    """per ell: random A, B, C with, in Python integers, the satisfying low half of C and the two product tables"""
    cache = {}

    def get(ell):
        if ell not in cache:
            rng = rng_for(12, ell)
            n, h = 1 << ell, 1 << (ell - 1)
            A, B, C = (ev.random_rows(rng, n) for _ in range(3))
            a, b, c = ev.rows_to_ints(A), ev.rows_to_ints(B), ev.rows_to_ints(C)
            ab = [ev.mont_mul(a[i], b[i]) for i in range(h)]
            p0 = ev.ints_to_rows([(ab[i] - c[i]) % ev.P for i in range(h)])
            p1 = ev.ints_to_rows([ev.mont_mul((a[i + h] - a[i]) % ev.P, (b[i + h] - b[i]) % ev.P) for i in range(h)])
            assert p0.all(axis=1).any() and all(x != y for x, y in zip(ab[:64], c[:64]))  # random C: P0 is non-zero
            cache[ell] = (A, B, C, ev.ints_to_rows(ab), p0, p1)
        return cache[ell]

    return get


def zero_mask(pattern, ell):
    """which of the 2^(ell-1) entries of P0 are zero (C = A o B there)"""
    h, ppt = 1 << (ell - 1), products_ppt(ell)
    idx = np.arange(h)
    if pattern == "all_zero":
        return np.ones(h, dtype=bool)
    if pattern == "none_zero":
        return np.zeros(h, dtype=bool)
    if pattern == "alternating_runs":  # 64-aligned runs: a zero wave next to a non-zero one in every block
        return (idx // 64) % 2 == 0
    if pattern in ("lane_0", "lane_63"):  # every other wave non-zero in that one lane of its first run only, the rest zero
        lane = 0 if pattern == "lane_0" else 63
        wave_first_run = (idx % (256 * ppt)) < 256
        return ~(wave_first_run & (idx % 64 == lane) & ((idx // 64) % 2 == 1))
    assert pattern == "last_chunk"  # non-zero only in the last 256 of every 1024: the last of a block's four chunks where the block has four
    return (idx % 1024) < 768


def wave_is_zero(mask, ell):
    """per wave of k_eval_products_stream, whether all its P0 entries are zero"""
    ppt = products_ppt(ell)
    m = mask.reshape(-1, ppt, 4, 64)  # block, chunk, wave, lane
    return m.all(axis=(1, 3)).reshape(-1)


@pytest.mark.parametrize("pattern", ZERO_PATTERNS)
@pytest.mark.parametrize("ell", PRODUCT_ELLS)
def test_round0_products_with_zero_and_non_zero_waves(ctx, product_base, ell, pattern):
    """sp_sumcheck_cubic3_round0 against oracle_cubic on (A, B, C), which never sees p0 or p1"""
    A, B, C, AB, P0, P1 = product_base(ell)
    h = 1 << (ell - 1)
    mask = zero_mask(pattern, ell)
    C = C.copy()
    C[:h][mask] = AB[mask]
    p0 = P0.copy()
    p0[mask] = 0
    waves = wave_is_zero(mask, ell)
    if pattern == "all_zero":
        assert waves.all()
    elif pattern == "none_zero" or (pattern == "last_chunk" and products_ppt(ell) == 4):
        assert not waves.any()  # four chunks per block: every wave holds three zero runs and a non-zero one, and the skip must not be taken
    else:
        assert waves.any() and not waves.all()  # one launch with both kinds of wave
    assert ((p0 == 0).all(axis=1) == mask).all()
    rng = rng_for(13, ell, ZERO_PATTERNS.index(pattern))
    taus, claim = ev.random_rows(rng, ell), rand_elem(rng)
    want_polys, want_r, want_fin, _ = oracle_cubic(claim, taus, A, B, C)
    tabs = to_device(ctx, (A, B, C, p0, P1))
    polys, r, fin = hip.sumcheck_cubic3_round0(ctx, claim, taus, *tabs, hip.Transcript(ctx, b"sc"))
    assert (r == want_r).all()
    assert (polys == want_polys).all()
    assert (fin == want_fin).all()
