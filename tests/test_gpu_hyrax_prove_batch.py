"""GPU parity: sp_hyrax_prove_batch - K instances of HyraxPCS::prove on one key, opened in one pass - against the CPU oracle's HyraxPCS::prove +
InnerProductArgumentLinear::prove (hyrax_pc.rs:387-478, ipa.rs:125-170) per instance: every output word, and the transcript's next squeeze. Every
instance has its own random polynomial, blinds, point, claimed evaluation, tape and transcript, and every transcript is warmed with a different absorb.

Which case reaches which form of the driver and its kernels (spartan2_amd/csrc/capi_opening_batch.hip, kernels_opening_batch.hpp):
  npt 9    one row, 512 columns on the 2048-wide key: k_ob_walk with delta vectors only (grid.y = K) and zero scalars between the polynomial's width
           and h; k_ob_mask / k_ob_z with two blocks an instance; no k_ob_rowmat; comm_LZ is the commitment's one row
  npt 11   one row, key-wide: as above with every scalar of the key
  npt 12   two rows: k_ob_rowmat with fewer rows than one pass of a block, k_ob_walk with 2 K vectors (comm_LZ's scalars from device memory)
  npt 13   four rows; npt 16: 32 rows (still one pass)
  npt 18   128 rows: k_ob_rowmat's loop with two loads in flight (rows > 64)
  K = 64   the maximum count: 128 walks in one launch at npt 12
  K = 1, SPARTAN_KEY_TABLES=0: the per-instance loop over sp_hyrax_prove
There is ONE form of the walk: keys of fewer than 1023 columns (k_multi_mul_coop's shape) take the per-instance loop, covered by the 256-wide case."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import lib as olib, p64
from spartan2_amd import frontend, hip, host

pytestmark = pytest.mark.gpu
SEED = 0x0B47C4
INVALID_INPUT_LENGTH = "rc=-1:"


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
    g = generators(b"ck", 2049)
    return hip.CommitmentKey(ctx, g[:2048], g[2048])


@pytest.fixture(scope="module")
def key_s(ctx):
    g = generators(b"ck_s", 2)
    return hip.CommitmentKey(ctx, g[:1], g[1])


class Instance:
    """one opening: inputs, and the oracle's output words and next squeeze for a transcript warmed with `warm` (and squeezed once first: pre_squeeze)"""

    def __init__(self, npt, k, width=2048, label=b"ck", pre_squeeze=False, share=None):
        rng = np.random.default_rng(SEED + 1000 * npt + k)
        self.npt, self.n = npt, 1 << npt
        self.rows = max(1, self.n // width)
        self.cols = self.n // self.rows
        if share is None:
            self.poly = ol.random_field_array(rng, self.n)
            self.blinds = ol.random_field_array(rng, self.rows)
        else:
            self.poly, self.blinds = share.poly, share.blinds
        self.point = ol.random_field_array(rng, npt)
        self.ev, self.b_ev = ol.random_field_array(rng, 1), ol.random_field_array(rng, 1)  # (the prover does not check the claimed evaluation)
        self.tape = ol.make_tape(SEED + 100 * npt + k, self.cols + 2 + k)  # (longer than needed by k blocks: only cols + 2 are consumed)
        self.warm = b"warm %d" % k
        okey = ctypes.c_void_p(olib().orc_hyrax_setup(label, ctypes.c_size_t(width)))
        okey_s = ctypes.c_void_p(olib().orc_hyrax_setup(b"ck_s", ctypes.c_size_t(1)))
        if share is None:
            self.comm = np.zeros((self.rows, 8), dtype=np.uint64)
            assert olib().orc_hyrax_commit(okey, p64(self.poly), ctypes.c_size_t(self.n), p64(self.blinds), 0, p64(self.comm)) == 0
        else:
            self.comm = share.comm
        self.comm_eval = np.zeros((1, 8), dtype=np.uint64)
        assert olib().orc_hyrax_commit(okey_s, p64(self.ev), ctypes.c_size_t(1), p64(self.b_ev), 0, p64(self.comm_eval)) == 0
        self.want = np.zeros(16 + 4 * self.cols + 8, dtype=np.uint64)
        otr = ctypes.c_void_p(olib().orc_transcript_new(b"pcs"))
        assert olib().orc_transcript_absorb(otr, b"x", self.warm, ctypes.c_size_t(len(self.warm))) == 0
        sq = np.zeros(4, dtype=np.uint64)
        if pre_squeeze:
            assert olib().orc_transcript_squeeze(otr, b"n", 0, p64(sq)) == 0
        assert olib().orc_hyrax_prove(okey, okey_s, otr, p64(self.comm), ctypes.c_size_t(self.rows), p64(self.poly), ctypes.c_size_t(self.n), p64(self.blinds),
                                      p64(self.point), ctypes.c_size_t(npt), p64(self.comm_eval), p64(self.b_ev),
                                      self.tape.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_size_t(self.tape.shape[0]), p64(self.want)) == 0
        self.want_next = np.zeros(4, dtype=np.uint64)
        assert olib().orc_transcript_squeeze(otr, b"n", 0, p64(self.want_next)) == 0
        olib().orc_transcript_free(otr)
        olib().orc_hyrax_free(okey)
        olib().orc_hyrax_free(okey_s)

    def transcript(self, ctx):
        tr = hip.Transcript(ctx, b"pcs")
        tr.absorb(b"x", self.warm)
        return tr


@functools.lru_cache(maxsize=None)
def instances(npt, count):
    """the first `count` instances at npt: computed once, shared by every case that needs them, never changed"""
    return tuple(Instance(npt, k) for k in range(count))


def call(ctx, key, key_s, insts, trs=None, tables=None):
    trs = [i.transcript(ctx) for i in insts] if trs is None else trs
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts] if tables is None else tables
    out = hip.hyrax_prove_batch(ctx, key, key_s, trs, [i.comm for i in insts], tables, insts[0].n, [i.blinds for i in insts], np.stack([i.point for i in insts]),
                                np.stack([i.comm_eval.reshape(8) for i in insts]), np.stack([i.b_ev.reshape(4) for i in insts]), [i.tape for i in insts])
    return out, trs


def check(insts, out, trs):
    for k, i in enumerate(insts):
        assert (out[k] == i.want).all(), f"instance {k} differs from the oracle's opening"
        assert (trs[k].squeeze(b"n") == i.want_next).all(), f"instance {k}: transcript state"


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("npt", [9, 11, 12, 13, 16])
def test_batch_is_the_oracles_opening_per_instance(ctx, key, key_s, npt, K):
    insts = instances(npt, 5)[:K]
    check(insts, *call(ctx, key, key_s, insts))


def test_tall_polynomials(ctx, key, key_s):
    """128 rows: more than one pass of a k_ob_rowmat block"""
    insts = instances(18, 2)
    check(insts, *call(ctx, key, key_s, insts))


def test_maximum_count(ctx, key, key_s):
    insts = instances(12, hip.LOCKSTEP_MAX)
    check(insts, *call(ctx, key, key_s, insts))
    # ... and a smaller batch on the same context afterwards (the workspaces shrink in use, the tickets are back at zero)
    check(insts[:3], *call(ctx, key, key_s, insts[:3]))


def test_one_instance_is_the_single_form(ctx, key, key_s):
    i = instances(13, 5)[4]
    out, trs = call(ctx, key, key_s, [i])
    tr = i.transcript(ctx)
    single = key.prove(key_s, tr, i.comm, hip.Table.from_host(ctx, i.poly), i.n, i.blinds, i.point, i.comm_eval, i.b_ev, i.tape)
    assert (out[0] == single).all() and (trs[0].squeeze(b"n") == tr.squeeze(b"n")).all()
    assert (single == i.want).all()


def test_without_key_tables_the_batch_is_the_per_proof_loop(ctx, key, key_s, monkeypatch):
    monkeypatch.setenv("SPARTAN_KEY_TABLES", "0")
    insts = instances(13, 5)[:3]
    out, trs = call(ctx, key, key_s, insts)
    for k, i in enumerate(insts):
        tr = i.transcript(ctx)
        single = key.prove(key_s, tr, i.comm, hip.Table.from_host(ctx, i.poly), i.n, i.blinds, i.point, i.comm_eval, i.b_ev, i.tape)
        assert (out[k] == single).all(), k
    check(insts, out, trs)


def test_narrow_key_takes_the_per_instance_loop(ctx, key_s):
    """a 256-wide key with four rows: below the walk's 1023 columns, so sp_hyrax_prove per instance - the same words as the oracle"""
    g = generators(b"ck256", 257)
    key256 = hip.CommitmentKey(ctx, g[:256], g[256])
    insts = [Instance(10, k, width=256, label=b"ck256") for k in range(3)]
    assert insts[0].rows == 4
    check(insts, *call(ctx, key256, key_s, insts))


def test_the_same_table_in_two_instances(ctx, key, key_s):
    a = instances(13, 5)[0]
    b = Instance(13, 7, share=a)
    assert not (a.point == b.point).all() and not (a.tape[:64] == b.tape[:64]).all()
    table = hip.Table.from_host(ctx, a.poly)
    check([a, b], *call(ctx, key, key_s, [a, b], tables=[table, table]))


def test_an_announced_opening_is_retracted_not_consumed(ctx, key, key_s):
    insts = instances(13, 5)[:3]
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts]
    a = insts[0]
    key.prove_announce(a.comm, tables[0], a.n, a.blinds, a.tape)
    check(insts, *call(ctx, key, key_s, insts, tables=tables))
    tr = a.transcript(ctx)
    single = key.prove(key_s, tr, a.comm, tables[0], a.n, a.blinds, a.point, a.comm_eval, a.b_ev, a.tape)
    assert (single == a.want).all() and (tr.squeeze(b"n") == a.want_next).all()


def test_refusals_change_nothing(ctx, key, key_s):
    """every refusal of the header, each SP_ERR_INVALID_INPUT_LENGTH with its reason; after each, every transcript squeezes what an untouched twin
    squeezes; at the end a correct call on the same transcripts and tables equals the oracle (whose transcripts were squeezed as often)"""
    npt = 12
    insts = [Instance(npt, 20 + k, pre_squeeze=True) for k in range(2)]
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts]
    short = hip.Table.from_host(ctx, insts[0].poly[: insts[0].n // 2])
    comms, blinds, tapes = [i.comm for i in insts], [i.blinds for i in insts], [i.tape for i in insts]
    points = np.stack([i.point for i in insts])
    cev, bev = np.stack([i.comm_eval.reshape(8) for i in insts]), np.stack([i.b_ev.reshape(4) for i in insts])
    n = insts[0].n

    def refused(why, trs, key_eval=key_s, **kw):
        """trs: an index into a fresh set of distinct transcripts (instance k % 2's warm-up), or None; every fresh transcript is compared afterwards"""
        a = dict(comm_rows=comms, polys=tables, n=n, blinds=blinds, points=points, comm_evals=cev, blind_evals=bev, rngs=tapes)
        a.update(kw)
        fresh = [insts[k % 2].transcript(ctx) for k in range(max(2, len(trs)))]
        trs = [fresh[t] if isinstance(t, int) else t for t in trs]
        with pytest.raises(hip.SpartanHipError, match=why) as e:
            hip.hyrax_prove_batch(ctx, key, key_eval, trs, a["comm_rows"], a["polys"], a["n"], a["blinds"], a["points"], a["comm_evals"], a["blind_evals"], a["rngs"])
        assert INVALID_INPUT_LENGTH in str(e.value)
        twins = [i.transcript(ctx).squeeze(b"n") for i in insts]
        for k, t in enumerate(fresh):
            assert (t.squeeze(b"n") == twins[k % 2]).all(), why

    refused("count must be", [])
    many = [k % 2 for k in range(hip.LOCKSTEP_MAX + 1)]  # one more than the maximum, every transcript its own object: only the count is wrong
    pick = lambda xs: [xs[k] for k in many]
    refused("count must be", list(range(len(many))), comm_rows=pick(comms), polys=pick(tables), blinds=pick(blinds), points=np.stack(pick(points)),
            comm_evals=np.stack(pick(cev)), blind_evals=np.stack(pick(bev)), rngs=pick(tapes))
    refused("null transcript, instance 1", [0, None])
    refused("null table, instance 0", [0, 1], polys=[None, tables[1]])
    refused("null commitment, instance 1", [0, 1], comm_rows=[comms[0], None])
    refused("null blinds, instance 0", [0, 1], blinds=[None, blinds[1]])
    refused("null randomness stream, instance 1", [0, 1], rngs=[tapes[0], None])
    refused("null argument", [0, 1], comm_evals=None)
    refused("null argument", [0, 1], blind_evals=None)
    refused("Expected 2\\^point.len\\(\\) elements", [0, 1], points=points[:, :-1])  # n != 2^npt
    refused("Expected 2\\^point.len\\(\\) elements in poly, instance 0", [0, 1], polys=[short, tables[1]])  # n above a table's capacity
    refused("one commitment row and one blind per matrix row", [0, 1], comm_rows=[np.concatenate([c, c[:1]]) for c in comms])
    refused("fewer than cols \\+ 2 blocks, instance 1", [0, 1], rngs=[tapes[0], tapes[1][: insts[1].cols + 1]])
    refused("same transcript twice", [0, 0])
    refused("ck_eval must be a narrow key with tables", [0, 1], key_eval=key)
    # the correct call, on transcripts that have been squeezed once like the oracle's
    trs = [i.transcript(ctx) for i in insts]
    for t in trs:
        t.squeeze(b"n")
    check(insts, *call(ctx, key, key_s, insts, trs=trs, tables=tables))


def prove_batch_both_ways(ctx, insts, gsp, prep_tapes, prep_used, osps, seed, **prep):
    assert gsp.prep_prove_batch(prep_tapes, **prep) == prep_used
    tapes = [ol.make_tape(seed + k, 8192) for k in range(len(insts))]
    batched, _ = gsp.prove_batch(tapes)
    looped, _ = gsp.prove_batch(tapes, per_proof_opening=True)
    for k in range(len(insts)):
        want, want_used, _ = osps[k].prove(tapes[k])
        for words, used in (batched[k], looped[k]):
            assert used == want_used and len(words) == len(want) and (words == want).all(), k
    gsp.close()


def oracles_prepped(insts, seed):
    osps, tapes, used = [], [], []
    for k, inst in enumerate(insts):
        osp = ol.OracleSpartan(inst)
        tape = ol.make_tape(seed + k, 1024)
        used.append(osp.prep_prove(tape))
        osps.append(osp)
        tapes.append(tape)
    return osps, tapes, used


def test_prove_batch_with_either_opening_is_the_oracles_proof_synthetic(ctx):
    insts = [frontend.synthetic_circuit(witness_seed=1000 * k, n_groups=5, seed=7, num_public=2) for k in range(3)]
    osps, prep_tapes, prep_used = oracles_prepped(insts, 1900)
    prove_batch_both_ways(ctx, insts, host.SpartanSNARK(ctx, insts[0]), prep_tapes, prep_used, osps, 1950, witnesses=insts)


def test_prove_batch_with_either_opening_is_the_oracles_proof_sha256(ctx):
    msgs = [bytes((37 * i + 11 * k + 3) % 256 for i in range(3)) for k in range(3)]
    insts = [frontend.sha256_circuit(m) for m in msgs]
    osps, prep_tapes, prep_used = oracles_prepped(insts, 1700)
    prove_batch_both_ways(ctx, insts, host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(3))), prep_tapes, prep_used, osps, 1750, msgs=msgs)
