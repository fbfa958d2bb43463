"""Coverage of the edge-value operand pool (tests/edge_values.py) is a condition, checked here without a GPU: pairs of pool values must reach every
branch of the scalar field's Montgomery reduction (fe_redc_p256 and the conditional subtraction behind it), uniform pairs demonstrably do not, and
every self-check transform of the device evaluator is exercised. Python integers only; nothing of the library runs here."""
import collections

import pytest

import edge_values as ev


@pytest.fixture(scope="module")
def pairs():
    return ev.pool_pairs(ev.N_PAIRS)


def test_pool_is_canonical_and_has_its_parts():
    pool = ev.operand_pool()
    assert all(0 <= v < ev.P for v in pool) and 3000 <= len(pool) <= 4500
    have = set(pool)
    for v in (0, 1, ev.P - 1, ev.P - 64, 1 << 255, ev.P - (1 << 255), ev.R % ev.P, ev.R * ev.R % ev.P, ev.P - ev.R % ev.P, ev.P - ev.R * ev.R % ev.P):
        assert v in have
    assert ev.operand_pool() == pool  # seeded
    base = ev.operand_pool(ev.P_BASE)
    assert all(0 <= v < ev.P_BASE for v in base) and ev.P_BASE - 1 in base


def test_redc_class_restates_the_reduction():
    """on values with a known answer: T = 0; T = (p - 1)^2, the largest product; T = a 2^256 for which the quotient is 0 and r = a"""
    assert ev.redc_class(0) == (0, False, False)
    ev.redc_class((ev.P - 1) ** 2)  # its assertions (divisibility, the closed form, the ranges of k and r) are the check
    assert ev.redc_class((ev.P - 1) << 256) == (0, False, False)
    assert ev.redc_class(ev.P << 256) == (0, True, False)
    assert ev.redc_class((ev.R - 1) << 256) == (0, True, False)
    for a, b in ev.pool_pairs(2000, seed=7):
        k, ge_p, ge_r = ev.redc_class(a * b)
        assert (ge_p and not ge_r) == ev.in_window(a, b)


def test_pool_pairs_reach_all_twelve_classes(pairs):
    hits = collections.Counter(ev.redc_class(a * b) for a, b in pairs)
    assert set(hits) == set(ev.ALL_CLASSES)
    for cls in ev.ALL_CLASSES:
        assert hits[cls] >= ev.MIN_HITS, (cls, hits[cls])


def test_uniform_pairs_never_reach_the_window():
    """why the pool exists: p <= r < 2^256 is 2^-32 of the range, and there fe_cond_sub_p_top must subtract although nothing carried"""
    hits = collections.Counter(ev.redc_class(a * b) for a, b in ev.uniform_pairs(ev.N_PAIRS))
    for k in (-1, 0, 1, 2):
        assert hits[(k, True, False)] == 0
    assert sum(hits.values()) == ev.N_PAIRS


def test_every_transform_is_taken(pairs):
    assert [name for name, _ in ev.transforms] == ["identity", "(p - a, b)", "(a, p - b)", "(p - a, p - b)"]
    hits = collections.Counter(ev.pick_transform(a, b) for a, b in pairs)
    for i in range(1, len(ev.transforms)):
        assert hits[i] >= ev.MIN_HITS, (ev.transforms[i][0], hits[i])
    # the rule itself, on every pair that took a transform: the transformed pair is canonical and lands in the window, no earlier transform does
    for a, b in pairs[:20000]:
        i = ev.pick_transform(a, b)
        x, y = ev.transforms[i][1](a, b)
        assert 0 <= x < ev.P and 0 <= y < ev.P
        if i:
            assert ev.in_window(x, y) and not ev.in_window(a, b)
            for j in range(1, i):
                u, v = ev.transforms[j][1](a, b)
                assert not (u < ev.P and v < ev.P and ev.in_window(u, v))


def test_carry_chain_pairs_send_k_across_seven_words():
    """the crafted family reaches what pool pairs cannot: a borrow of k = -1 through seven zero words, a carry of k = 1 and k = 2 through seven words of ones"""
    hits = collections.Counter()
    for a, b in ev.carry_chain_pairs():
        assert 0 <= a < ev.P and 0 < b < ev.P
        k, r = ev.redc_parts(a * b)
        low = (r - k) % (1 << 224)  # the low seven words of the sum the header adds k to
        if low == 0 or low == (1 << 224) - 1:
            hits[(k, low == 0)] += 1
    assert hits[(-1, True)] >= 20 and hits[(1, False)] >= 20 and hits[(2, False)] >= 20, hits


def test_palette_and_tables():
    import numpy as np

    rng = np.random.default_rng(3)
    pal = ev.palette(rng)
    assert pal.shape == (16, 4) and pal.dtype == np.uint64
    vals = ev.rows_to_ints(pal)
    assert vals[:6] == [0, ev.R % ev.P, (ev.P - 1) * ev.R % ev.P, ev.P - 1, (ev.P - 1) // 2, 1 << 255] and all(v < ev.P for v in vals)
    t = ev.palette_table(rng, 1 << 12, pal)
    assert t.shape == (1 << 12, 4) and set(ev.rows_to_ints(t)) == set(vals)
    heavy = ev.palette_table(rng, 1000, pal, weights=[1] + [0] * 15)
    assert not heavy.any()
    assert (ev.constant_table(5, ev.raw_max()) == ev.to_limbs64(ev.P - 1)).all()
    assert ev.from_limbs32(ev.to_limbs32(ev.P - 2)) == ev.P - 2 and (ev.ints_to_rows([ev.P - 2])[0] == ev.to_limbs64(ev.P - 2)).all()
    assert all(v < ev.P for v in ev.rows_to_ints(ev.random_rows(rng, 4096)))
