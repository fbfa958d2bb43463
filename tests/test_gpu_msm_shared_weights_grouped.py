"""GPU parity for sp_msm_shared_weights_grouped: `groups` shared-weights MSMs (msm.rs:228-356) of one shape in one pass. Every group of every case is
checked against oracle/neutronnova.hpp (orc_msm_shared_weights) and against hip.msm_shared_weights on the same inputs, word for word. The shapes cross
the 64-row boundary between the per-group latency form and the grouped kernels, one of them runs two chunks of groups, and the weights hold a 1, a 0,
p - 1, two groups with one weight vector and one all-zero group."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import lib as olib, p64, to_mont
from spartan2_amd import hip

pytestmark = pytest.mark.gpu
SEED = 0x6A09E667
P = ol.MODULI[0]
SPECIALS = (1, 0, P - 1)
# (groups, rows, n)
SHAPES = [(1, 80, 16), (2, 32, 2), (3, 22, 7), (5, 13, 33), (64, 1, 32), (3, 5, 4),
          (4, 32, 3), (3, 43, 3)]  # 128 and 129 rows in all: the last batch whose window Horner runs on host threads, the first that runs it on the device
POOL = max(g * r * n for g, r, n in SHAPES)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """one list of curve points for every case (read-only)"""
    gens = np.zeros((POOL, 8), dtype=np.uint64)
    olib().orc_from_label(b"fold", ctypes.c_size_t(POOL), p64(gens))
    gens.setflags(write=False)
    return gens


def make_weights(rng, groups, n):
    w = ol.random_field_array(rng, groups * n).reshape(groups, n, 4)
    for g in range(groups):
        for j in range(3):  # positions 1.. hold a 1, a 0 and p - 1, rotated by group so that every n >= 2 sees all three
            if 1 + j < n:
                w[g, 1 + j] = to_mont(SPECIALS[(g + j) % 3])
    if groups >= 2:
        w[1] = w[0]  # two groups with one weight vector (their bases differ)
    if groups >= 3:
        w[groups - 1] = 0  # an all-zero group: every row is the identity
    return w


def oracle_rows(w, bases):
    rows, n = bases.shape[0], bases.shape[1]
    want = np.zeros((rows, 8), dtype=np.uint64)
    olib().orc_msm_shared_weights(p64(np.ascontiguousarray(w)), ctypes.c_size_t(n), p64(np.ascontiguousarray(bases.reshape(-1))), ctypes.c_size_t(rows), p64(want))
    return want


def check_case(ctx, pts, groups, rows, n, seed, aux=False):
    rng = np.random.default_rng(seed)
    bases = np.ascontiguousarray(pts[: groups * rows * n].reshape(groups, rows, n, 8))
    w = make_weights(rng, groups, n)
    got = hip.msm_shared_weights_grouped(ctx, w, bases, aux=aux)
    assert got.shape == (groups, rows, 8)
    for g in range(groups):
        assert (got[g] == oracle_rows(w[g], bases[g])).all(), f"group {g} differs from the oracle"
        assert (got[g] == hip.msm_shared_weights(ctx, w[g], bases[g])).all(), f"group {g} differs from the single call"
    if groups >= 3:
        assert not got[groups - 1].any()  # the identity as the single call writes it


@pytest.mark.parametrize("groups,rows,n", SHAPES)
def test_grouped_equals_oracle_and_single_call(ctx, pool, groups, rows, n):
    check_case(ctx, pool, groups, rows, n, SEED + groups * 1000 + rows)


def test_auxiliary_lane(ctx, pool):
    check_case(ctx, pool, 3, 22, 7, SEED + 1, aux=True)


@pytest.mark.parametrize("groups,rows,n", [(2, 32, 2), (4, 32, 3), (3, 43, 3)])
def test_window_horner_on_either_side(ctx, pool, groups, rows, n):
    """sp_msm_shared_weights_grouped_opts: the Horner on host threads and in one launch, on both sides of the row count that decides by default"""
    rng = np.random.default_rng(SEED + 5 + rows)
    bases = np.ascontiguousarray(pool[: groups * rows * n].reshape(groups, rows, n, 8))
    w = make_weights(rng, groups, n)
    want = np.stack([oracle_rows(w[g], bases[g]) for g in range(groups)])
    for side in (hip.MSM_GROUPED_HORNER_HOST, hip.MSM_GROUPED_HORNER_DEVICE):
        assert (hip.msm_shared_weights_grouped(ctx, w, bases, horner=side) == want).all()


def test_two_chunks(ctx, pool):
    cap = hip.msm_shared_weights_group_rows()
    rows, n = 64, 2
    groups = cap // rows + 1  # one group more than a launch takes
    assert groups * rows == cap + rows and groups * rows * n <= POOL
    check_case(ctx, pool, groups, rows, n, SEED + 2)


def test_output_hygiene_and_noops(ctx, pool):
    L = hip.lib()
    sz = ctypes.c_size_t
    groups, rows, n = 3, 22, 7
    rng = np.random.default_rng(SEED + 3)
    bases = np.ascontiguousarray(pool[: groups * rows * n].reshape(groups, rows, n, 8))
    w = make_weights(rng, groups, n)
    want = hip.msm_shared_weights_grouped(ctx, w, bases)
    junk = np.uint64(0xA5A5A5A5A5A5A5A5)
    tail = 64
    out = np.full(groups * rows * 8 + tail, junk, dtype=np.uint64)
    assert L.sp_msm_shared_weights_grouped(ctx.h, p64(w), sz(n), p64(bases.reshape(-1)), sz(rows), sz(groups), p64(out)) == 0
    assert (out[: groups * rows * 8].reshape(groups, rows, 8) == want).all()
    assert (out[groups * rows * 8 :] == junk).all()
    # groups == 0 or rows == 0: nothing is written
    out[:] = junk
    assert L.sp_msm_shared_weights_grouped(ctx.h, p64(w), sz(n), p64(bases.reshape(-1)), sz(rows), sz(0), p64(out)) == 0
    assert L.sp_msm_shared_weights_grouped(ctx.h, p64(w), sz(n), p64(bases.reshape(-1)), sz(0), sz(groups), p64(out)) == 0
    assert (out == junk).all()
    # n == 0: the output is zeroed, as by the single call, and nothing past it
    assert L.sp_msm_shared_weights_grouped(ctx.h, p64(w), sz(0), p64(bases.reshape(-1)), sz(rows), sz(groups), p64(out)) == 0
    assert not out[: groups * rows * 8].any() and (out[groups * rows * 8 :] == junk).all()


def test_refusals(ctx, pool):
    L = hip.lib()
    sz = ctypes.c_size_t
    groups, rows, n = 2, 32, 2
    bases = np.ascontiguousarray(pool[: groups * rows * n])
    w = make_weights(np.random.default_rng(SEED + 4), groups, n)
    junk = np.uint64(0x5A5A5A5A5A5A5A5A)
    out = np.full(groups * rows * 8, junk, dtype=np.uint64)
    for f in (L.sp_msm_shared_weights_grouped, L.sp_msm_shared_weights_grouped_aux):
        for c, pw, pb, po in ((None, p64(w), p64(bases), p64(out)), (ctx.h, None, p64(bases), p64(out)), (ctx.h, p64(w), None, p64(out)), (ctx.h, p64(w), p64(bases), None)):
            assert f(c, pw, sz(n), pb, sz(rows), sz(groups), po) == -1
            assert b"msm_shared_weights_grouped" in L.sp_last_error()
        # sizes no launch could index
        assert f(ctx.h, p64(w), sz(1 << 31), p64(bases), sz(rows), sz(groups), p64(out)) == -1
        assert f(ctx.h, p64(w), sz(n), p64(bases), sz(1 << 31), sz(groups), p64(out)) == -1
        assert f(ctx.h, p64(w), sz(n), p64(bases), sz(rows), sz(1 << 40), p64(out)) == -1
        assert f(ctx.h, p64(w), sz(1 << 30), p64(bases), sz(1 << 20), sz(1), p64(out)) == -1  # rows * n past what the workspaces are sized for
    f = L.sp_msm_shared_weights_grouped_opts  # the same null checks, and flags other than 0, 1, 2
    for c, pw, pb, po, flags in ((None, p64(w), p64(bases), p64(out), 0), (ctx.h, None, p64(bases), p64(out), 1), (ctx.h, p64(w), None, p64(out), 2), (ctx.h, p64(w), p64(bases), None, 0),
                                 (ctx.h, p64(w), p64(bases), p64(out), 3), (ctx.h, p64(w), p64(bases), p64(out), 1 << 31)):
        assert f(c, pw, sz(n), pb, sz(rows), sz(groups), po, ctypes.c_uint(flags)) == -1
        assert b"msm_shared_weights_grouped" in L.sp_last_error()
    assert (out == junk).all()
