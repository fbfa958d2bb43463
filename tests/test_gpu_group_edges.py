"""GPU: P + P, P - P and identity operands inside the MSM kernels, at the tree levels where uniform inputs never put them (probability ~2^-256).

Every base is k_i H with a known discrete log, built by the ORACLE's fixed-base multiplication (tests/group_edges.py DlogPoints), so the expected
result of every call is (sum s_i k_i mod N) H: the sum in Python integers, one oracle fixed-base multiplication - independent of any MSM, ours or the
oracle's. Where the oracle has the operation the result is compared with orc_msm as well. All comparisons are bit-exact on canonical affine coordinates.

The cases of the table walks (k_multi_mul_coop, k_multi_mul_wide), of the fixed-base walk of h, of K11 (k_msm_bucket_sum, k_msm_window_reduce_coop, the
host Horner) and of the batched-row path (k_msm_bucket_sum_shared / _grouped, k_msm_window_reduce_seg, k_msm_horner_rows) are the lists
test_group_edges_cpu.py proves to reach every (stage, class) cell of their replays. The tree sums of k_msm_binary_rows and k_sum_rows_of_points, the row
path of PCS::commit and the general Pippenger behind sp_msm_points get structured inputs against the dlog reference without a coverage claim (the
Pippenger's order inside a bucket depends on block scheduling and has no deterministic replay at all)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import group_edges as ge
import oracle_lib as ol
from group_edges import N
from oracle_lib import lib as olib, p64
from spartan2_amd import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pts():
    return ge.DlogPoints()


def oracle_msm(scalars, bases):
    out = np.zeros(8, dtype=np.uint64)
    assert olib().orc_msm(p64(np.ascontiguousarray(scalars)), p64(np.ascontiguousarray(bases)), ctypes.c_size_t(scalars.shape[0]), ctypes.c_size_t(1), p64(out)) == 0
    return out


# ---- FixedBaseTables.multi_mul: the cooperative walk ------------------------------------------------------------------------------------------------
def _run_coop_cases(ctx, pts, n, groups):
    cases = [c for c in ge.coop_cases() if c[0] == n and c[1] == groups]
    assert cases
    k = cases[0][3]
    bases = pts.points(k)
    t = hip.FixedBaseTables(ctx, bases)
    pts.need([ge.dot(k, s) for *_, s in cases])
    try:
        for i, (_, _, name, kk, s) in enumerate(cases):
            assert kk == k
            sc = ol.mont_array(s)
            want = pts.point(ge.dot(k, s))
            got = t.multi_mul(sc)
            assert (got == want).all(), f"n={n} {name}: the walk's sum is not (sum s_i k_i) H"
            assert (t.multi_mul(sc) == want).all(), f"n={n} {name}: second run on the same ticket / sequence counter"  # the ticket reset after an exceptional join
            if i % 4 == 0 or n <= 8:
                assert (oracle_msm(sc, bases) == want).all(), f"n={n} {name}: the oracle's MSM disagrees with the dlog reference"
    finally:
        t.close()


@pytest.mark.parametrize("n", [n for n, g in ge.COOP_SIZES if g])
def test_multi_mul_cooperative_walk_at_every_cell(ctx, pts, n):
    """k_multi_mul_coop at n = 4, 8 (the smallest join), 130 (33 blocks: groups of 5 added on the host), 516 (groups of 17) and 1022 (the largest size
    below the wide kernel): every case twice. With the groups on (the default) no join has more than 32 block sums."""
    _run_coop_cases(ctx, pts, n, True)


def test_multi_mul_cooperative_walk_with_one_join_on_the_device(ctx, pts):
    """SPARTAN_WALK_GROUPS=0 (read once per process, hence a child process): n = 516 is 129 blocks joined by ONE last block - the only shape that runs
    the + 128 take-in loop and the join levels 64 and 32 of k_multi_mul_coop."""
    if os.environ.get("SPARTAN_WALK_GROUPS", "1")[:1] == "0":
        for n, g in ge.COOP_SIZES:
            if not g:
                _run_coop_cases(ctx, pts, n, False)
        return
    args = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", f"{os.path.join('tests', 'test_gpu_group_edges.py')}::{test_multi_mul_cooperative_walk_with_one_join_on_the_device.__name__}"]
    r = subprocess.run(args, cwd=ROOT, env=dict(os.environ, SPARTAN_WALK_GROUPS="0", SPARTAN_TEST_CHILD="1"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]


def test_multi_mul_wide_walk_at_every_cell(ctx, pts):
    """k_multi_mul_wide just above the launcher's switch (capi_group.hip multi_mul_wide_min = 1024; tests/test_gpu_group.py runs 1022, the largest size
    below it, and so does the cooperative test above): the cases test_group_edges_cpu.py proves to reach every reachable cell of its replay - twin and
    opposite scalars inside one block at every distance at which two scalars meet (the lane-private xyzz_add_mixed, the shuffle-by-32 xyzz_add, the
    cooperative levels), shifted scalars for the byte-pair levels, and equal / opposite block sums in different blocks for the join. Every case twice."""
    k = ge.wide_bases(ge.WIDE_N)
    cases = ge.wide_scalar_cases()
    assert ge.WIDE_N >= ge.MM_WIDE_MIN > 1022
    bases = pts.points(k)
    t = hip.FixedBaseTables(ctx, bases)
    pts.need([ge.dot(k, s) for _, s in cases])
    try:
        for i, (name, s) in enumerate(cases):
            sc = ol.mont_array(s)
            want = pts.point(ge.dot(k, s))
            assert (t.multi_mul(sc) == want).all(), name
            assert (t.multi_mul(sc) == want).all(), name + " (second run)"
            if i % 8 == 0:
                assert (oracle_msm(sc, bases) == want).all(), name
    finally:
        t.close()


@pytest.mark.parametrize("r_last", [0, 1])
def test_multi_mul_eq_with_a_degenerate_last_level(ctx, pts, r_last):
    """sp_fbtables_multi_mul_begin_eq at k = 3 with r_3 in {0, 1}: half the expanded scalars are zero, the other half repeat P[idx / 2]; with P[0] = P[1]
    and base 2 = base 0, base 3 = -base 1, the items of scalars 0 and 2 of block 0 are equal (r_3 = 0) and those of scalars 1 and 3 opposite (r_3 = 1)
    at the walk's first level."""
    nfixed = 8
    k = [v or 1 for v in ge.uniform_values(nfixed + 1, 51)]
    k[2], k[3], k[6] = k[0], N - k[1], k[4]
    P = ge.uniform_values(4, 52)
    P[1] = P[0]
    s0, s1 = ge.uniform_values(2, 53)
    s = [P[i // 2] * (r_last if i % 2 else 1 - r_last) % N for i in range(nfixed)] + [(s0 + r_last * (s1 - s0)) % N]
    t = hip.FixedBaseTables(ctx, pts.points(k))
    want = pts.point(ge.dot(k, s))
    try:
        for _ in range(2):
            assert (t.multi_mul_eq(ol.mont_array(P), nfixed, ol.mont_array([s0, s1]), ol.to_mont(r_last)) == want).all()
        assert (t.multi_mul(ol.mont_array(s)) == want).all()
    finally:
        t.close()


# ---- CommitmentKey.fixed_base_mul_h ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h_key(ctx, pts):
    kappa = ge.uniform_values(1, 61)[0]
    return hip.CommitmentKey(ctx, pts.points(ge.uniform_values(2, 62)), pts.point(kappa)), kappa


@pytest.mark.parametrize("n", ge.FB_SIZES)
def test_fixed_base_mul_h_on_sparse_scalars(ctx, pts, h_key, n):
    """k_fixed_base_rows_coop_mapped (n = 70) and k_fixed_base_rows_coop (n = 600) on a key whose h is kappa H: scalars with one non-zero byte in each
    position, two non-zero bytes, a and a 256^m - the identity on either side of every tree level (P = +-Q cannot occur with one base: group_edges
    FB_UNREACHABLE). Synchronous and _begin / _finish."""
    key, kappa = h_key
    s = ge.fixed_base_scalars(n)
    want = pts.points([v * kappa % N for v in s])
    sc = ol.mont_array(s)
    assert (key.fixed_base_mul_h(sc) == want).all()
    assert (key.fixed_base_mul_h_finish(key.fixed_base_mul_h_begin(sc)) == want).all()
    assert (key.fixed_base_mul_h(sc[::-1].copy()) == want[::-1]).all()


# ---- sp_msm / sp_msm_small below the Pippenger switch: K11 -----------------------------------------------------------------------------------------------
def test_msm_at_every_cell_of_the_bucket_method(ctx, pts):
    """sp_msm below 4096 points (k_msm_digits / k_msm_sort_digits, k_msm_bucket_sum, k_msm_window_reduce_coop, the host Horner) on the cases
    test_group_edges_cpu.py proves to reach every cell of its replay: bucket contents chosen at will (up to 24 points: 16 equal points in one bucket,
    equal and opposite buckets `off` apart for every scan level, a suffix sum that equals or negates its partner at every tree level) and the
    families at n = 2, 9, 64, 1000 - all scalars equal (one bucket per window) over twin and anti-twin bases, twins and anti-twins with equal scalars,
    a window sum that is +-256 times the Horner accumulator, zero scalars, identity bases."""
    for name, k, s in ge.k11_cases():
        bases, sc = pts.points(k), ol.mont_array(s)
        want = pts.point(ge.dot(k, s))
        assert (hip.msm(ctx, sc, bases) == want).all(), name
        assert (oracle_msm(sc, bases) == want).all(), name


@pytest.mark.parametrize("n", [2, 9, 64, 1000])
def test_msm_small_with_one_digit_per_scalar(ctx, pts, n):
    """sp_msm_small_u64 at bits = 8 over twin and anti-twin bases: every scalar has one digit, twins with one scalar land in one bucket."""
    rng = np.random.default_rng(80 + n)
    for sign in (1, -1):
        k, _ = ge.twin(n, 1, sign=sign)
        u = rng.integers(0, 256, size=n, dtype=np.uint64)
        u[1::2] = u[0::2][: len(u[1::2])]
        for small in (u, np.full(n, 200, dtype=np.uint64), np.full(n, 1, dtype=np.uint64)):
            want = pts.point(ge.dot(k, [int(v) for v in small]))
            assert (hip.msm_small(ctx, small, pts.points(k)) == want).all(), (sign, int(small[0]))


# ---- shared weights: the batched-row path ----------------------------------------------------------------------------------------------------------------
def _shared_case(pts, rows):
    s, named = ge.shared_rows_case(rows)
    bases = np.stack([pts.points(k) for _, k in named])
    want = pts.points([ge.dot(k, s) for _, k in named])
    return s, named, bases, want


@pytest.mark.parametrize("rows", [1, 3, 64, 65])
def test_msm_shared_weights_at_every_cell_of_the_batched_row_path(ctx, pts, rows):
    """sp_msm_shared_weights at n = 256: rows 1 and 3 take k_msm_bucket_sum + k_msm_window_reduce_coop, 64 rows k_msm_bucket_sum_shared +
    k_msm_window_reduce_seg with the Horner on the host, 65 rows the same with k_msm_horner_rows. The rows are group_edges.shared_rows_case: one
    weight vector, every row its own bases - the bucket chains, run / acc, the x tree, rr / y and the final jac_add(x, 16 y) of the segmented
    reduction and acc 2^8 + W_w of the Horner, each at its doubling and identity exits, a row of identities - with a uniform row after every two, so
    one wave holds exceptional and generic lanes side by side."""
    s, named, bases, want = _shared_case(pts, rows)
    sc = ol.mont_array(s)
    got = hip.msm_shared_weights(ctx, sc, bases)
    bad = [named[r][0] for r in range(rows) if not (got[r] == want[r]).all()]
    assert not bad, bad
    assert (oracle_msm(sc, bases[rows - 1]) == want[rows - 1]).all()


@pytest.mark.parametrize("horner", [0, hip.MSM_GROUPED_HORNER_HOST, hip.MSM_GROUPED_HORNER_DEVICE])
def test_msm_shared_weights_grouped_at_every_cell(ctx, pts, horner):
    """sp_msm_shared_weights_grouped with 2 groups of 54 rows (every case of group_edges.row_specs; from 64 rows in all the call takes
    k_msm_bucket_sum_grouped, tests/test_gpu_msm_shared_weights_grouped.py), the window Horner on either side: group 0 is the crafted rows under
    their weights, group 1 the same bases under uniform weights."""
    rows = 54
    s, named, bases, want = _shared_case(pts, rows)
    assert {name for name, _ in ge.row_specs()} <= {name for name, _ in named}
    s2 = ge.uniform_values(256, 91)
    want2 = pts.points([ge.dot(k, s2) for _, k in named])
    assert 64 <= 2 * rows <= hip.msm_shared_weights_group_rows()
    got = hip.msm_shared_weights_grouped(ctx, np.stack([ol.mont_array(s), ol.mont_array(s2)]), np.stack([bases, bases]), horner=horner)
    bad = [(g, named[r][0]) for g, w in ((0, want), (1, want2)) for r in range(rows) if not (got[g][r] == w[r]).all()]
    assert not bad, bad


# ---- sp_msm_points: the general Pippenger -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 8, 13])
def test_msm_points_with_twins_and_one_bucket(ctx, pts, window):
    """kernels_pippenger.hpp at n = 4096: 64 twin pairs and 64 anti-twin pairs with equal scalars and a block of 300 equal scalars over twin bases.
    Dlog reference only: the order of additions inside a bucket depends on block scheduling, so there is no replay and no coverage claim."""
    n = 4096
    k, s = ge.uniform_values(n, 95), ge.uniform_values(n, 96)
    k = [v or 1 for v in k]
    for i in range(64):
        a, b = 100 + 2 * i, 101 + 2 * i
        k[b], s[b] = k[a], s[a]
        a, b = 1000 + 2 * i, 3000 + i  # anti-twins far apart
        k[b], s[b] = N - k[a], s[a]
    for i in range(300):
        s[2000 + i] = s[2000]
        if i % 2:
            k[2000 + i] = k[2000 + i - 1]
    got = hip.msm_points(ctx, hip.Table.from_host(ctx, ol.mont_array(s)), 0, n, hip.Points(ctx, pts.points(k)), 0, window)
    assert (got == pts.point(ge.dot(k, s))).all()


# ---- commitments over a structured key ------------------------------------------------------------------------------------------------------------------
def _key_case(ctx, pts, width):
    k = ge.key_dlogs(width)
    kappa = ge.uniform_values(1, 97)[0]
    key = hip.CommitmentKey(ctx, pts.points(k), pts.point(kappa))
    rows = ge.key_rows(width)
    rows += [(f"uniform_{i}", dict(enumerate(ge.uniform_values(width, 200 + i)))) for i in range(21)]  # enough full rows for the batched path
    blinds = ge.key_blinds(rows, k, kappa)
    want = pts.points([(sum(v * k[c] for c, v in cols.items()) + b * kappa) % N for (_, cols), b in zip(rows, blinds)])
    return key, k, kappa, rows, blinds, want


def _row_scalars(width, cols):
    s = [0] * width
    for c, v in cols.items():
        s[c] = v
    return s


@pytest.mark.parametrize("width", [32, 128])
def test_commit_over_a_key_with_twin_anti_twin_and_identity_columns(ctx, pts, width):
    """PCS::commit on a key of k_i H with twins, anti-twins and an identity column; the reference is the dlog dot product plus the blind's term.
    width 32: per-base table walks (k_fixed_base_rows_coop) and k_sum_rows_of_points - the tree over a row's 33 points, the blind's term at its first
    level. width 128: bit rows through k_msm_binary_rows (a twin pair, an anti-twin pair, all columns, none), full rows through the batched digit
    path, the blind's term added on the host. Blinds that make h * blind the row's own point or its negation."""
    key, k, kappa, rows, blinds, want = _key_case(ctx, pts, width)
    v = ol.mont_array([x for _, cols in rows for x in _row_scalars(width, cols)])
    got = key.commit(hip.Table.from_host(ctx, v), 0, len(rows) * width, ol.mont_array(blinds))
    bad = [rows[r][0] for r in range(len(rows)) if not (got[r] == want[r]).all()]
    assert not bad, bad
    # two full rows on their own: the single-MSM path per row
    two = [i for i, (name, _) in enumerate(rows) if name in ("full_twins_adjacent", "full_anti_twins_half_apart")]
    v2 = ol.mont_array([x for i in two for x in _row_scalars(width, rows[i][1])])
    got2 = key.commit(hip.Table.from_host(ctx, v2), 0, 2 * width, ol.mont_array([blinds[i] for i in two]))
    assert (got2 == want[two]).all()


def test_commit_small_over_the_structured_key(ctx, pts):
    """sp_hyrax_commit_small on the width-32 key: the host walk (few non-zero scalars) and the device form (more than six)."""
    key, k, kappa, rows, blinds, want = _key_case(ctx, pts, 32)
    for r, (name, cols) in enumerate(rows):
        got = key.commit_small(ol.mont_array(_row_scalars(32, cols)), ol.to_mont(blinds[r]))
        assert (got == want[r]).all(), name
