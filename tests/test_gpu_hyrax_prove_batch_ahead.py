"""GPU parity: a batch opened ahead - sp_hyrax_prove_batch_begin / _rows / _finish (spartan2_amd/csrc/capi_opening_batch.hip) - against the CPU oracle's
HyraxPCS::prove + InnerProductArgumentLinear::prove per instance (orc_hyrax_prove: every output word and the transcript's next squeeze) and against one
sp_hyrax_prove_batch call on fresh transcripts. The instances are those of test_gpu_hyrax_prove_batch.py (2048-wide key; own polynomial, blinds, point,
tape and warmed transcript per instance), computed once and shared.

Which case reaches which form:
  npt 9    one row, 512 of 2048 columns: zero scalars up to h in the delta walk; no row stage (_rows is a no-op, comm_LZ is the commitment's row)
  npt 11   one row, key-wide: every scalar of the key
  npt 12   two rows (nvr = 1): k_ob_rowmat below one pass, k_ob_walk over the comm_LZ vectors alone (vector base K)
  npt 13   four rows
  npt 18   128 rows: k_ob_rowmat's loop with two loads in flight
  K = 64   the maximum count at npt 12
Every (npt, K) runs three ways that must give the same words: _begin, _rows, _finish; _begin, _finish (the row stage queued by _finish); _begin, a
context synchronise, _rows, _finish (the row stage queued on an idle device). The warmed transcripts have absorbed since their last squeeze, so the
commitment is hashed by _finish; the lifecycle tests use squeezed-once transcripts, for which the sponge hashed ahead by _begin is installed."""
import ctypes
import functools

import numpy as np
import pytest

from oracle_lib import lib as olib, p64
from spartan2_amd import hip
from test_gpu_hyrax_prove_batch import INVALID_INPUT_LENGTH, Instance, call, check, generators, instances

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def key(ctx):
    g = generators(b"ck", 2049)
    return hip.CommitmentKey(ctx, g[:2048], g[2048])


@pytest.fixture(scope="module")
def key_s(ctx):
    g = generators(b"ck_s", 2)
    return hip.CommitmentKey(ctx, g[:1], g[1])


def nvr_of(i):
    return i.rows.bit_length() - 1


def begin(ctx, key, key_s, insts, tables):
    return hip.OpeningJob(ctx, key, key_s, [i.comm for i in insts], tables, insts[0].n, [i.blinds for i in insts], [i.tape for i in insts])


def finish(job, key, key_s, insts, tables, trs):
    return job.finish(key, key_s, trs, [i.comm for i in insts], tables, insts[0].n, [i.blinds for i in insts], np.stack([i.point for i in insts]),
                      np.stack([i.comm_eval.reshape(8) for i in insts]), np.stack([i.b_ev.reshape(4) for i in insts]), [i.tape for i in insts])


def row_points(insts):
    return np.stack([i.point[: nvr_of(i)] for i in insts])


def ahead(ctx, key, key_s, insts, way, tables=None, trs=None):
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts] if tables is None else tables
    trs = [i.transcript(ctx) for i in insts] if trs is None else trs
    job = begin(ctx, key, key_s, insts, tables)
    if way == "rows":
        job.rows(row_points(insts))
    elif way == "rows_after_sync":
        ctx.synchronize()
        job.rows(row_points(insts))
    else:
        assert way == "no_rows"
    return finish(job, key, key_s, insts, tables, trs), trs


@functools.lru_cache(maxsize=None)
def first(npt, K):
    """the first K instances at npt, on top of the sets test_gpu_hyrax_prove_batch.py already computes (5 an npt, 2 at npt 18, 64 at npt 12)"""
    have = instances(npt, hip.LOCKSTEP_MAX if K > 5 else 2 if npt == 18 else 5)
    return (have + tuple(Instance(npt, k) for k in range(len(have), K)))[:K]


WAYS = ("rows", "no_rows", "rows_after_sync")
CASES = [(npt, K) for npt in (9, 11, 12, 13) for K in (2, 3, 5)] + [(18, 2), (18, 3), (18, 5), (12, hip.LOCKSTEP_MAX)]


@pytest.mark.parametrize("npt,K", CASES)
def test_three_ways_are_the_oracles_openings_and_the_batched_calls(ctx, key, key_s, npt, K):
    insts = first(npt, max(K, 5))[:K]
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts]
    plain, plain_trs = call(ctx, key, key_s, insts, tables=tables)
    check(insts, plain, plain_trs)
    for way in WAYS:
        out, trs = ahead(ctx, key, key_s, insts, way, tables=tables)
        assert (out == plain).all(), way
        check(insts, out, trs)


def test_a_sponge_hashed_ahead_serves_transcripts_that_were_squeezed_last(ctx, key, key_s):
    """transcripts squeezed once after their warm-up have absorbed nothing since: _finish installs the sponges _begin hashed"""
    insts = [Instance(12, 20 + k, pre_squeeze=True) for k in range(3)]
    for way in WAYS:
        trs = [i.transcript(ctx) for i in insts]
        for t in trs:
            t.squeeze(b"n")
        check(insts, *ahead(ctx, key, key_s, insts, way, trs=trs))


def oracle_opening(i, comm):
    """the oracle's opening of instance i with `comm` in place of its commitment (the prover hashes the commitment it is given) -> (words, next squeeze)"""
    okey = ctypes.c_void_p(olib().orc_hyrax_setup(b"ck", ctypes.c_size_t(2048)))
    okey_s = ctypes.c_void_p(olib().orc_hyrax_setup(b"ck_s", ctypes.c_size_t(1)))
    otr = ctypes.c_void_p(olib().orc_transcript_new(b"pcs"))
    assert olib().orc_transcript_absorb(otr, b"x", i.warm, ctypes.c_size_t(len(i.warm))) == 0
    want, want_next = np.zeros_like(i.want), np.zeros(4, dtype=np.uint64)
    assert olib().orc_hyrax_prove(okey, okey_s, otr, p64(comm), ctypes.c_size_t(i.rows), p64(i.poly), ctypes.c_size_t(i.n), p64(i.blinds), p64(i.point),
                                  ctypes.c_size_t(i.npt), p64(i.comm_eval), p64(i.b_ev), i.tape.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                  ctypes.c_size_t(i.tape.shape[0]), p64(want)) == 0
    assert olib().orc_transcript_squeeze(otr, b"n", 0, p64(want_next)) == 0
    olib().orc_transcript_free(otr)
    olib().orc_hyrax_free(okey)
    olib().orc_hyrax_free(okey_s)
    return want, want_next


@pytest.mark.parametrize("what", ["rng", "blinds", "table", "commitment", "rows"])
def test_finish_given_something_else_opens_what_it_is_given(ctx, key, key_s, what):
    """_begin (and _rows) see instance 1 with one input that differs from what _finish is given; _finish must open what IT is given. For the
    commitment the address stays and the words behind it change in between (the job compares by value)."""
    insts = list(instances(12, 5)[:3])
    other = instances(12, 5)[4]
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts]
    comms, blinds, tapes, polys = [i.comm for i in insts], [i.blinds for i in insts], [i.tape for i in insts], list(tables)
    rows = row_points(insts)
    if what == "rng":
        tapes[1] = other.tape
    elif what == "blinds":
        blinds[1] = other.blinds
    elif what == "table":
        polys[1] = hip.Table.from_host(ctx, other.poly)
    elif what == "commitment":
        comms[1] = np.ascontiguousarray(insts[1].comm.copy(), dtype=np.uint64)
    else:
        rows = rows.copy()
        rows[1] = other.point[:1]
    job = hip.OpeningJob(ctx, key, key_s, comms, polys, insts[0].n, blinds, tapes)
    job.rows(rows)
    trs = [i.transcript(ctx) for i in insts]
    if what != "commitment":
        check(insts, finish(job, key, key_s, insts, tables, trs), trs)
        return
    assert job.comm_rows[1].ctypes.data == comms[1].ctypes.data
    comms[1][:] = other.comm
    want, want_next = oracle_opening(insts[1], comms[1])
    assert not (want == insts[1].want).all()
    out = job.finish(key, key_s, trs, comms, tables, insts[0].n, [i.blinds for i in insts], np.stack([i.point for i in insts]),
                     np.stack([i.comm_eval.reshape(8) for i in insts]), np.stack([i.b_ev.reshape(4) for i in insts]), [i.tape for i in insts])
    assert (out[1] == want).all() and (trs[1].squeeze(b"n") == want_next).all()
    check([insts[0], insts[2]], out[[0, 2]], [trs[0], trs[2]])


def test_count_one_and_the_narrow_key_go_through_the_job_calls(ctx, key, key_s):
    i = instances(13, 5)[4]
    for way in WAYS:
        check([i], *ahead(ctx, key, key_s, [i], way))
    g = generators(b"ck256", 257)
    key256 = hip.CommitmentKey(ctx, g[:256], g[256])
    insts = [Instance(10, k, width=256, label=b"ck256") for k in range(3)]
    assert insts[0].rows == 4
    for way in WAYS:
        check(insts, *ahead(ctx, key256, key_s, insts, way))


def single(ctx, key, key_s, i, table):
    tr = i.transcript(ctx)
    out = key.prove(key_s, tr, i.comm, table, i.n, i.blinds, i.point, i.comm_eval, i.b_ev, i.tape)
    assert (out == i.want).all() and (tr.squeeze(b"n") == i.want_next).all()


def test_drop_leaves_the_context_to_the_plain_calls(ctx, key, key_s):
    insts = instances(12, 5)[:3]
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts]
    job = begin(ctx, key, key_s, insts, tables)
    job.rows(row_points(insts))
    job.drop()
    check(insts, *call(ctx, key, key_s, insts, tables=tables))
    job = begin(ctx, key, key_s, insts, tables)
    job.drop()
    single(ctx, key, key_s, insts[0], tables[0])
    check(insts, *ahead(ctx, key, key_s, insts, "rows", tables=tables))


def test_one_job_per_context(ctx, key, key_s):
    insts = instances(12, 5)[:3]
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts]
    job = begin(ctx, key, key_s, insts, tables)
    with pytest.raises(hip.SpartanHipError, match="a batch opened ahead is pending") as e:
        begin(ctx, key, key_s, insts, tables)
    assert INVALID_INPUT_LENGTH in str(e.value)
    with pytest.raises(hip.SpartanHipError, match="a batch opened ahead is pending") as e:
        call(ctx, key, key_s, insts, tables=tables)
    assert INVALID_INPUT_LENGTH in str(e.value)
    job.rows(row_points(insts))
    trs = [i.transcript(ctx) for i in insts]
    check(insts, finish(job, key, key_s, insts, tables, trs), trs)


def test_begin_refuses_what_the_batched_call_refuses(ctx, key, key_s):
    insts = [Instance(12, 20 + k, pre_squeeze=True) for k in range(2)]
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts]
    short = hip.Table.from_host(ctx, insts[0].poly[: insts[0].n // 2])
    comms, blinds, tapes = [i.comm for i in insts], [i.blinds for i in insts], [i.tape for i in insts]
    n = insts[0].n

    def good():
        trs = [i.transcript(ctx) for i in insts]
        for t in trs:
            t.squeeze(b"n")
        check(insts, *ahead(ctx, key, key_s, insts, "rows", tables=tables, trs=trs))

    def refused(why, key_eval=key_s, **kw):
        a = dict(comm_rows=comms, polys=tables, n=n, blinds=blinds, rngs=tapes)
        a.update(kw)
        with pytest.raises(hip.SpartanHipError, match=why) as e:
            hip.OpeningJob(ctx, key, key_eval, a["comm_rows"], a["polys"], a["n"], a["blinds"], a["rngs"])
        assert INVALID_INPUT_LENGTH in str(e.value)
        good()

    many = [k % 2 for k in range(hip.LOCKSTEP_MAX + 1)]
    pick = lambda xs: [xs[k] for k in many]
    refused("count must be", comm_rows=[], polys=[], blinds=[], rngs=[])
    refused("count must be", comm_rows=pick(comms), polys=pick(tables), blinds=pick(blinds), rngs=pick(tapes))
    refused("null table, instance 0", polys=[None, tables[1]])
    refused("null commitment, instance 1", comm_rows=[comms[0], None])
    refused("null blinds, instance 0", blinds=[None, blinds[1]])
    refused("null randomness stream, instance 1", rngs=[tapes[0], None])
    refused("Expected 2\\^point.len\\(\\) elements", n=n - 1)
    refused("Expected 2\\^point.len\\(\\) elements in poly, instance 0", polys=[short, tables[1]])
    refused("one commitment row and one blind per matrix row", comm_rows=[np.concatenate([c, c[:1]]) for c in comms])
    refused("fewer than cols \\+ 2 blocks, instance 1", rngs=[tapes[0], tapes[1][: insts[1].cols + 1]])
    refused("ck_eval must be a narrow key with tables", key_eval=key)


def test_begin_retracts_a_single_proof_announcement(ctx, key, key_s):
    insts = instances(13, 5)[:3]
    tables = [hip.Table.from_host(ctx, i.poly) for i in insts]
    a = insts[0]
    key.prove_announce(a.comm, tables[0], a.n, a.blinds, a.tape)
    check(insts, *ahead(ctx, key, key_s, insts, "rows", tables=tables))
    single(ctx, key, key_s, a, tables[0])
