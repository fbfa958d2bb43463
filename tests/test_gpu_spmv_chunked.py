"""GPU parity: sp_multiply_vec_chunked - multiply_vec_batched (src/r1cs/sparse.rs:237-302) with chunks of SPMV_KC vectors sharing one walk over A, B and C
(k_spmv3_multi). Az, Bz, Cz of every vector must equal the oracle's orc_shape_multiply_vec word for word, at counts on both sides of a chunk boundary,
on a synthetic circuit and on the one-block SHA-256 circuit (whose 32-bit additions are the rows the whole wave walks)."""
import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import lib as olib, p64
from spartan2_amd import frontend, hip
from spartan2_amd.host import pad_shape

pytestmark = pytest.mark.gpu
SEED = 0xDEADBEEF


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["synthetic", "sha256_1block"])
def case(request, ctx):
    """the shape on the device, 2 KC + 3 vectors (the real z first) and the oracle's products of each, computed once"""
    inst = frontend.synthetic_circuit(40, SEED, num_public=3) if request.param == "synthetic" else frontend.sha256_circuit(b"abc")
    oshape = ol.OracleShape(inst)
    mats, dims = pad_shape(inst)
    shape = hip.Shape(ctx, mats, dims)
    N, M, ncols = oshape.num_cons, oshape.num_vars, oshape.num_vars + oshape.num_extra
    Wt = np.zeros((M, 4), dtype=np.uint64)
    Wt[oshape.num_shared : oshape.num_shared + len(inst.witness)] = ol.mont_array([int(x) for x in inst.witness])
    z_real = np.concatenate([Wt, ol.mont_array([1] + [int(x) for x in inst.publics])])
    rng = np.random.default_rng(SEED)
    rnd = ol.random_field_array(rng, ncols)
    KC = hip.SPMV_KC
    zs = [z_real] + [np.ascontiguousarray(np.roll(rnd, 17 * j, axis=0)) for j in range(2 * KC + 2)]
    wants = []
    for z in zs:
        want = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
        assert olib().orc_shape_multiply_vec(oshape.h, p64(z), *(p64(w) for w in want)) == 0
        wants.append(want)
    tabs = [hip.Table.from_host(ctx, z) for z in zs]
    dirt = ol.random_field_array(rng, 64)
    return dict(shape=shape, N=N, ncols=ncols, zs=zs, wants=wants, tabs=tabs, dirt=dirt)


def dirty(ctx, case):
    """an output table full of something else"""
    return hip.Table.from_host(ctx, np.resize(case["dirt"], (case["N"], 4)))


def test_chunk_size_is_the_library_s():
    assert hip.SPMV_KC == hip.multiply_vec_chunk() >= 2


@pytest.mark.parametrize("count", ["1", "KC", "KC+1", "2KC+3"])
def test_chunked_equals_oracle(ctx, case, count):
    KC = hip.SPMV_KC
    n = {"1": 1, "KC": KC, "KC+1": KC + 1, "2KC+3": 2 * KC + 3}[count]
    outs = [[dirty(ctx, case) for _ in range(n)] for _ in range(3)]
    case["shape"].multiply_vec_chunked(case["tabs"][:n], *outs)
    for k in range(n):
        for m in range(3):
            assert len(outs[m][k]) == case["N"]
            assert (outs[m][k].read() == case["wants"][k][m]).all(), f"vector {k}, matrix {'ABC'[m]}"


def test_the_same_input_table_twice_in_one_call(ctx, case):
    KC = hip.SPMV_KC
    order = [0, 1, 0] + list(range(2, KC)) + [1]  # the table at two positions of one chunk, and again in the next
    outs = [[dirty(ctx, case) for _ in order] for _ in range(3)]
    case["shape"].multiply_vec_chunked([case["tabs"][j] for j in order], *outs)
    for k, j in enumerate(order):
        for m in range(3):
            assert (outs[m][k].read() == case["wants"][j][m]).all(), f"position {k} (vector {j}), matrix {'ABC'[m]}"


def test_refusals_name_the_vector(ctx, case):
    shape, N = case["shape"], case["N"]
    outs = [[hip.Table.zeros(ctx, N) for _ in range(3)] for _ in range(3)]
    longer = hip.Table.from_host(ctx, np.concatenate([case["zs"][1], case["zs"][1][:1]]))
    with pytest.raises(hip.SpartanHipError, match=r"rc=-2: multiply_vec_chunked: z has the wrong length, vector 2"):
        shape.multiply_vec_chunked([case["tabs"][0], case["tabs"][1], longer], *outs)
    short = hip.Table.zeros(ctx, N - 1)
    bz = [outs[1][0], short, outs[1][2]]
    with pytest.raises(hip.SpartanHipError, match=r"rc=-1: multiply_vec_chunked: output table too short, vector 1"):
        shape.multiply_vec_chunked(case["tabs"][:3], outs[0], bz, outs[2])
    for m in range(3):  # a refused call has written nothing
        assert not outs[m][0].read().any()
    shape.multiply_vec_chunked(case["tabs"][:3], *outs)
    for k in range(3):
        for m in range(3):
            assert (outs[m][k].read() == case["wants"][k][m]).all()
