"""GPU parity: sp_nifs_layers_batch (k_nifs_layers) - the NIFS layers of every instance of every state in one launch, z = [W | 1 | X] never assembled.
Every layer must equal the oracle's orc_shape_multiply_vec of the assembled z word for word, padding clones included, at (count, n) on both sides of the
chunk (KC = sp_nifs_layers_chunk()): on synthetic_circuit(8, num_public=3), whose tail is indexed beyond the 1, and on sha256_step_circuit, whose 32-bit
additions are the rows the whole wave walks. W is random field elements (one vector is the real witness), X is random. Nothing expected comes from the
code under test, except where two forms of it are compared with each other (the NIFS prove behind the layers)."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import lib as olib, p64
from spartan2_amd import frontend, hip, host
from spartan2_amd.host import pad_shape

pytestmark = pytest.mark.gpu
SEED = 0x5EED1A7E
NVEC = 9  # vectors per shape: (3, 3) takes them all


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def make_case(ctx, name, nvec):
    """the shape on the device, nvec (W, X) pairs - the real witness first - as device tables, and the oracle's products of each assembled z, computed once"""
    inst = frontend.synthetic_circuit(8, SEED, num_public=3) if name == "synthetic" else frontend.sha256_step_circuit(bytes(range(64)))
    oshape = ol.OracleShape(inst)
    mats, dims = pad_shape(inst)
    shape = hip.Shape(ctx, mats, dims)
    N, M, d = oshape.num_cons, oshape.num_vars, oshape.num_public
    assert oshape.num_challenges == 0 and oshape.num_rest_unpadded == 0 and oshape.num_shared == 0  # the witness is the precommitted segment, at offset 0
    rng = np.random.default_rng(SEED)
    W_real = np.zeros((M, 4), dtype=np.uint64)
    W_real[: len(inst.witness)] = ol.mont_array([int(x) for x in inst.witness])
    Ws = [W_real] + [ol.random_field_array(rng, M) for _ in range(nvec - 1)]
    Xs = [ol.mont_array([int(x) for x in inst.publics]).reshape(d, 4)] + [ol.random_field_array(rng, d).reshape(d, 4) for _ in range(nvec - 1)]
    one = ol.mont_array([1])
    wants = []
    for W, X in zip(Ws, Xs):
        z = np.ascontiguousarray(np.concatenate([W, one, X]))
        want = [np.zeros((N, 4), dtype=np.uint64) for _ in range(3)]
        assert olib().orc_shape_multiply_vec(oshape.h, p64(z), *(p64(w) for w in want)) == 0
        wants.append(want)
    assert any(w.any() for w in wants[0]) and not (wants[1][0] == wants[2][0]).all()
    tabs = [hip.Table.from_host(ctx, W) for W in Ws]
    _, left, right = ol.tensor_decomp(N)
    return dict(name=name, oshape=oshape, shape=shape, dims=dims, N=N, M=M, d=d, Ws=Ws, Xs=Xs, wants=wants, tabs=tabs, left=left, right=right,
                junk=ol.random_field_array(rng, 64))


@pytest.fixture(scope="module")
def case(ctx):
    return make_case(ctx, "synthetic", NVEC)


@pytest.fixture(scope="module")
def sha_case(ctx):
    return make_case(ctx, "sha256_step", 6)


def n_padded_of(n):
    return max(2, 1 << (n - 1).bit_length())


def fresh_nifs(ctx, case, n, junk=True):
    """an object whose layers hold something else"""
    nf = hip.Nifs(ctx, n_padded_of(n), case["left"], case["right"])
    if junk:
        fill = np.resize(case["junk"], (case["N"], 4))
        for which in range(3):
            for b in range(nf.n_padded):
                nf.layer(which, b).write(0, fill)
    return nf


def layers_of(nf, N):
    out = []
    for b in range(nf.n_padded):
        views = [nf.layer(which, b) for which in range(3)]
        for v in views:
            assert v.info() == (N, hip.SIZE_MAX, hip.SIZE_MAX)  # length and zero-structure hints: what sp_multiply_vec leaves on a layer view
        out.append([v.read() for v in views])
    return out


def check_state(case, nf, n, vec_of_instance):
    """layer b of `nf` is the oracle's product of vector vec_of_instance[b < n ? b : 0]"""
    got = layers_of(nf, case["N"])
    for b in range(nf.n_padded):
        j = vec_of_instance[b if b < n else 0]
        for m in range(3):
            assert (got[b][m] == case["wants"][j][m]).all(), f"layer {b} (vector {j}), matrix {'ABC'[m]}"


def run(ctx, case, count, n, order=None):
    order = list(range(count * n)) if order is None else order
    objs = [fresh_nifs(ctx, case, n) for _ in range(count)]
    hip.nifs_layers_batch(ctx, case["shape"], objs, n, [case["tabs"][j] for j in order], np.stack([case["Xs"][j] for j in order]))
    for k, nf in enumerate(objs):
        check_state(case, nf, n, order[k * n : (k + 1) * n])
    return objs


def test_chunk_size_is_the_library_s():
    assert hip.nifs_layers_chunk() >= 2


# (count, n) around the chunk KC = 4: one chunk not full; one padding clone; three clones over two chunks; a chunk spanning two objects; a ragged last
# chunk; every vector with clones in between
@pytest.mark.parametrize("count,n", [(1, 2), (1, 3), (1, 5), (2, 2), (3, 2), (3, 3)])
def test_layers_equal_oracle(ctx, case, count, n):
    for nf in run(ctx, case, count, n):
        nf.free()


@pytest.mark.parametrize("count,n", [(1, 2), (2, 3)])
def test_layers_equal_oracle_sha256_step(ctx, sha_case, count, n):
    """the rows the whole wave walks; (2, 3): clones, a chunk spanning both objects"""
    for nf in run(ctx, sha_case, count, n):
        nf.free()


def test_one_table_in_two_states(ctx, case):
    """the same W table (and X) as instance 0 of state 0, instance 1 of state 1 and, through the padding, two further layers"""
    for nf in run(ctx, case, 2, 3, order=[1, 2, 3, 4, 1, 2]):
        nf.free()


def test_nifs_prove_behind_the_layers(ctx, case):
    """sp_nifs_prepare_small + NeutronNovaNIFS::prove on an object filled here gives the outputs of one built by nifs_prepare (sp_multiply_vec per layer)"""
    n, M, N = 3, case["M"], case["N"]
    L = olib()
    okey = ctypes.c_void_p(L.orc_hyrax_setup(b"ck", ctypes.c_size_t(2048)))
    ck_aff, h_aff = np.zeros((2048, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    L.orc_hyrax_key_export(okey, p64(ck_aff), p64(h_aff))
    ck = hip.CommitmentKey(ctx, ck_aff, h_aff)
    rows = (M + 2047) // 2048
    assert rows * 2048 == M
    rng = np.random.default_rng(SEED + 1)
    r_W = np.stack([ol.random_field_array(rng, rows) for _ in range(n)])
    comms = np.zeros((n, rows, 8), dtype=np.uint64)
    for k in range(n):
        assert L.orc_hyrax_commit(okey, p64(case["Ws"][k]), ctypes.c_size_t(M), p64(r_W[k]), 0, p64(comms[k])) == 0
    L.orc_hyrax_free(okey)
    tabs, X = case["tabs"][:n], np.stack(case["Xs"][:n])
    outs = []
    for form in ("nifs_prepare", "layers_batch"):
        if form == "nifs_prepare":
            prepared = host.nifs_prepare(ctx, case["shape"], case["dims"], X, tabs, True)
        else:
            nf = fresh_nifs(ctx, case, n)
            hip.nifs_layers_batch(ctx, case["shape"], [nf], n, tabs, X)
            nf.prepare_small()
            prepared = nf.h
        outs.append(host.nifs_prove(ctx, case["shape"], case["dims"], ck, comms, X, tabs, r_W, True, hip.Transcript(ctx, b"neutronnova_prove"),
                                    ol.transcript_round_hook(ol.Transcript(b"vc")), prepared=prepared))
        if form == "nifs_prepare":
            host.nifs_free(prepared)
        else:
            nf.free()
    a, b = outs
    for key in ("polys", "r_bs", "E_eq", "tail", "folded_rW", "folded_X", "folded_comm"):
        assert (a[key] == b[key]).all(), key
    for key, cnt in (("A", N), ("B", N), ("C", N), ("folded_W", M)):
        assert (a[key].read(0, cnt) == b[key].read(0, cnt)).all(), key
    assert a["polys"].any()


def test_refusals_leave_the_layers_untouched(ctx, case):
    shape, N, M, d = case["shape"], case["N"], case["M"], case["d"]
    L, sz = hip.lib(), ctypes.c_size_t
    n = 2
    objs = [fresh_nifs(ctx, case, n) for _ in range(2)]
    before = [layers_of(nf, N) for nf in objs]
    tabs = case["tabs"][:4]
    X = np.ascontiguousarray(np.stack(case["Xs"][:4])).reshape(-1)
    narr = lambda os_: (ctypes.c_void_p * len(os_))(*[o.h if o is not None else None for o in os_])
    tarr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.h if t is not None else None for t in ts])

    def refused(rc, msg, *args):
        assert L.sp_nifs_layers_batch(*args) == rc
        assert msg in L.sp_last_error(), L.sp_last_error()

    refused(-1, b"sp_nifs_layers_batch: count must be at least 1", ctx.h, shape.h, sz(0), narr(objs), sz(n), tarr(tabs), p64(X))
    refused(-1, b"sp_nifs_layers_batch: null argument", ctx.h, shape.h, sz(2), None, sz(n), tarr(tabs), p64(X))
    refused(-1, b"sp_nifs_layers_batch: null argument", ctx.h, shape.h, sz(2), narr(objs), sz(n), None, p64(X))
    refused(-1, b"sp_nifs_layers_batch: null argument", ctx.h, None, sz(2), narr(objs), sz(n), tarr(tabs), p64(X))
    refused(-1, b"sp_nifs_layers_batch: null public values", ctx.h, shape.h, sz(2), narr(objs), sz(n), tarr(tabs), None)
    refused(-1, b"sp_nifs_layers_batch: null sp_nifs, state 1", ctx.h, shape.h, sz(2), narr([objs[0], None]), sz(n), tarr(tabs), p64(X))
    refused(-1, b"sp_nifs_layers_batch: null table, state 1, instance 0", ctx.h, shape.h, sz(2), narr(objs), sz(n), tarr([tabs[0], tabs[1], None, tabs[3]]), p64(X))
    longer = hip.Table.from_host(ctx, np.concatenate([case["Ws"][1], case["Ws"][1][:1]]))
    refused(-2, b"sp_nifs_layers_batch: W does not have num_vars elements, state 1, instance 1", ctx.h, shape.h, sz(2), narr(objs), sz(n),
            tarr([tabs[0], tabs[1], tabs[2], longer]), p64(X))
    # an object with fewer layers than instances (n = 3 into n_padded = 2) and one whose layers are not num_cons long
    X3 = np.ascontiguousarray(np.stack(case["Xs"][:6])).reshape(-1)
    refused(-1, b"sp_nifs_layers_batch: n_padded is smaller than the number of instances, state 0", ctx.h, shape.h, sz(2), narr(objs), sz(3), tarr(case["tabs"][:6]), p64(X3))
    half = hip.Nifs(ctx, 2, case["left"] // 2, case["right"])
    refused(-1, b"sp_nifs_layers_batch: the layers do not have num_cons elements, state 1", ctx.h, shape.h, sz(2), narr([objs[0], half]), sz(n), tarr(tabs), p64(X))
    half.free()
    # a shape with a verifier challenge
    chal_dims = dict(case["dims"])
    chal_dims["num_public"], chal_dims["num_challenges"] = d - 1, 1
    chal_shape = hip.Shape(ctx, pad_shape(frontend.synthetic_circuit(8, SEED, num_public=3))[0], chal_dims)
    refused(-1, b"sp_nifs_layers_batch: a shape with verifier challenges", ctx.h, chal_shape.h, sz(2), narr(objs), sz(n), tarr(tabs), p64(X))
    for nf, want in zip(objs, before):  # nothing was written
        got = layers_of(nf, N)
        for b in range(nf.n_padded):
            for m in range(3):
                assert (got[b][m] == want[b][m]).all()
    hip.nifs_layers_batch(ctx, shape, objs, n, tabs, np.stack(case["Xs"][:4]))  # and the objects still serve
    for k, nf in enumerate(objs):
        check_state(case, nf, n, [2 * k, 2 * k + 1])
        nf.free()
