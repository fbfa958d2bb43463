"""The crafted inputs of tests/group_edges.py reach every exit of every addition of the replayed kernels - and uniform inputs reach none of the
P = +-Q exits. No GPU, no oracle: the replays run the kernels' addition orders on the discrete logs.

  coverage   across the cases test_gpu_group_edges.py runs (the same list, imported from group_edges), every replay reports every cell
             (stage, class) except an UNREACHABLE set that is proved in group_edges and must be EXACTLY what is never reported
  the gap    uniform inputs of the same sizes report no `equal` and no `opposite` cell
  the replay its final dlog is sum s_i k_i mod N on crafted and uniform inputs"""
import collections

import pytest

import group_edges as ge
from group_edges import N


def _coop_cells(cases):
    cells = collections.Counter()
    for n, groups, name, k, s in cases:
        c, final = ge.replay_multi_mul_coop(k, s, groups)
        assert final == ge.dot(k, s), (n, groups, name)
        cells.update(c)
    return cells


@pytest.fixture(scope="module")
def coop_crafted():
    return _coop_cells(ge.coop_cases())


def test_cooperative_walk_cases_reach_every_cell(coop_crafted):
    want = {(st, c) for st in ge.COOP_STAGES for c in ge.CLASSES}
    assert set(coop_crafted) <= want, set(coop_crafted) - want
    missing = want - set(coop_crafted)
    assert missing == set(ge.COOP_UNREACHABLE), sorted(missing ^ set(ge.COOP_UNREACHABLE))


def test_cooperative_walk_on_uniform_inputs_never_meets_equal_or_opposite_points():
    cells = _coop_cells([(n, g, "uniform", ge.uniform_values(n, 100 + n), ge.uniform_values(n, 200 + n)) for n, g in ge.COOP_SIZES])
    assert {st for st, _ in cells} == set(ge.COOP_STAGES)
    assert not [c for c in cells if c[1] in ("equal", "opposite")]


def _wide_cells(k, scalar_lists):
    cells = collections.Counter()
    for name, s in scalar_lists:
        c, final = ge.replay_multi_mul_wide(k, s)
        assert final == ge.dot(k, s), name
        cells.update(c)
    return cells


def test_wide_walk_cases_reach_every_reachable_cell():
    cells = _wide_cells(ge.wide_bases(ge.WIDE_N), ge.wide_scalar_cases())
    want = {(st, c) for st in ge.WIDE_STAGES for c in ge.CLASSES}
    assert set(cells) <= want, set(cells) - want
    missing = want - set(cells)
    assert missing == set(ge.WIDE_UNREACHABLE), sorted(missing ^ set(ge.WIDE_UNREACHABLE))


def test_wide_walk_on_uniform_inputs_never_meets_equal_or_opposite_points():
    cells = _wide_cells(ge.uniform_values(ge.WIDE_N, 400), [("uniform", ge.uniform_values(ge.WIDE_N, 401 + i)) for i in range(3)])
    assert {st for st, _ in cells} == set(ge.WIDE_STAGES)
    assert not [c for c in cells if c[1] in ("equal", "opposite")]


def _cells(replay, cases, order):
    cells = collections.Counter()
    for name, k, s in cases:
        c, final = replay(k, s, order)
        assert final == ge.dot(k, s), name
        cells.update(c)
    return cells


# The order of the entries INSIDE a bucket is the order in which the sort's atomics land: the conditions hold for thread order and for its reverse.
@pytest.mark.parametrize("order", ["index", "reverse"])
def test_k11_cases_reach_every_cell(order):
    cells = _cells(ge.replay_msm_k11, ge.k11_cases(), order)
    want = {(st, c) for st in ge.K11_STAGES for c in ge.CLASSES}
    assert set(cells) <= want, set(cells) - want
    assert want - set(cells) == set(ge.K11_UNREACHABLE), sorted((want - set(cells)) ^ set(ge.K11_UNREACHABLE))


def test_k11_on_uniform_inputs_never_meets_equal_or_opposite_points():
    """at 64 and 1000 points; at 2 and 9 most buckets are empty, neighbouring suffix sums are equal and the window reduction doubles by accident"""
    cases = [(f"uniform_{n}", ge.uniform_values(n, 500 + n), ge.uniform_values(n, 600 + n)) for n in (64, 1000)]
    cells = _cells(ge.replay_msm_k11, cases, "index")
    assert not [c for c in cells if c[1] in ("equal", "opposite")]
    small = _cells(ge.replay_msm_k11, [("uniform_2", ge.uniform_values(2, 502), ge.uniform_values(2, 602))], "index")
    assert [c for c in small if c[1] == "equal" and c[0].startswith("wtree")]


def _row_cases(rows=65):
    s, named = ge.shared_rows_case(rows)
    return [(name, k, s) for name, k in named]


@pytest.mark.parametrize("order", ["index", "reverse"])
def test_batched_row_cases_reach_every_cell(order):
    cases = _row_cases()
    assert {name for name, _ in ge.row_specs()} <= {name for name, _, _ in cases}  # 65 rows hold every spec (and so do the 64 of the other GPU case)
    assert {name for name, _ in ge.row_specs()} <= {name for name, _, _ in _row_cases(64)}
    cells = _cells(ge.replay_batched_row, cases, order)
    want = {(st, c) for st in ge.ROW_STAGES for c in ge.CLASSES}
    assert set(cells) <= want, set(cells) - want
    assert want - set(cells) == set(ge.ROW_UNREACHABLE), sorted((want - set(cells)) ^ set(ge.ROW_UNREACHABLE))


def test_batched_rows_on_uniform_inputs_meet_equal_points_in_one_place_only():
    """256 uniform weights leave about one bucket in eight empty. An empty bucket right below a segment's first non-empty one makes acc == run in
    k_msm_window_reduce_seg's `acc += run` - the one P = Q exit ordinary inputs of this size do take (a 2048-column key fills every bucket and takes
    none). Every other `equal` and every `opposite` cell is out of their reach."""
    s = ge.uniform_values(256, 700)
    cells = _cells(ge.replay_batched_row, [(f"uniform_{r}", ge.uniform_values(256, 701 + r), s) for r in range(8)], "index")
    assert {st for st, _ in cells} == set(ge.ROW_STAGES)
    assert {c for c in cells if c[1] in ("equal", "opposite")} == {("seg_acc", "equal")}


def _fb_cells(scalar_lists, wbits):
    cells = collections.Counter()
    kappa = ge.uniform_values(1, 5)[0]
    for s in scalar_lists:
        c, outs = ge.replay_fixed_base(kappa, s, wbits)
        assert outs == [v * kappa % N for v in s]
        cells.update(c)
    return cells


@pytest.mark.parametrize("wbits", [8, 16])
def test_fixed_base_cases_reach_every_reachable_cell(wbits):
    cells = _fb_cells([ge.fixed_base_scalars(n) for n in ge.FB_SIZES], wbits)
    want = {(st, c) for st in ge.FB_STAGES[wbits] for c in ge.CLASSES}
    unreachable = {cell for cell in ge.FB_UNREACHABLE if cell[0] in ge.FB_STAGES[wbits]}
    assert set(cells) <= want
    assert want - set(cells) == unreachable, sorted((want - set(cells)) ^ unreachable)


@pytest.mark.parametrize("wbits", [8, 16])
def test_fixed_base_on_uniform_scalars_never_meets_an_identity_below_the_first_levels(wbits):
    """a uniform scalar has a zero byte now and then (the first level sees an identity operand), but a zero run of 8 bytes or more - an identity at
    the last two levels - with probability 2^-64"""
    cells = _fb_cells([ge.uniform_values(n, 300 + n) for n in ge.FB_SIZES], wbits)
    assert {c for st, c in cells if st in ge.FB_STAGES[wbits][-2:]} == {"generic"}
    assert not [c for c in cells if c[1] in ("equal", "opposite")]


def test_classify_and_digits():
    assert [ge.classify(a, b) for a, b in ((0, 5), (0, 0), (5, 0), (5, 5), (5, N - 5), (5, N + 5), (5, 6), (N, 3))] == [
        "left_id", "left_id", "right_id", "equal", "opposite", "equal", "generic", "left_id"]
    for s in ge.uniform_values(50, 1) + [0, 1, 127, 128, 255, 256, N - 1, (N + 1) // 2, (N - 1) // 2, (1 << 255) - 1]:
        assert sum(d << (8 * j) for j, d in enumerate(ge.byte_digits(s))) == s
        f, neg = ge.fold_sign(s)
        assert f < 1 << 255 and (N - f if neg else f) % N == s and (not neg or f < s)
        dg = ge.signed_digits(f)
        assert all(-128 <= d <= 127 for d in dg) and sum(d << (8 * w) for w, d in enumerate(dg)) == f


def test_families_do_what_they_claim():
    for delta in (1, 2, 4):
        k, s = ge.twin(64, delta)
        a, _ = ge.anti_twin(64, delta)
        assert k[delta] == k[0] and s[delta] == s[0] and (a[delta] + a[0]) % N == 0
    k, s = ge.one_bucket(64)
    assert len(set(s)) == 1 and k[1] == k[0]
    for sign in (1, -1):
        k, s = ge.horner_collision(9, sign)
        assert (s[0] * k[0] - sign * s[1] * k[1]) % N == 0 and s[0] == 256 * s[1]  # the same point, or its negation, one window apart
        k, s = ge.seg_collision(9, sign)
        x, y = (15 * k[1] + k[0]) % N, k[0]  # acc_0 + acc_1 and run_1
        assert ge.classify(x, 16 * y) == ("equal" if sign > 0 else "opposite")
