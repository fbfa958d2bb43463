// sp_hyrax_prove (include/spartan_hip.h): HyraxPCS::prove (src/provider/pcs/hyrax_pc.rs:387-478) + InnerProductArgumentLinear::prove
// (src/provider/pcs/ipa.rs:125-170), the lone opening that closes every prove, and its announcement (sp_hyrax_prove_announce / _announce_tables / _retract).
// ONE call in the place where the reference's trait method sits, so that a caller that follows src/spartan.rs:423-437 statement by statement gets the
// overlap below the ABI that the C++ driver used to arrange above it:
//   * the 64-byte-per-row transcript encoding of `comm` and the Keccak blocks of absorb(b"poly_com", comm) run on the context's helper thread,
//   * delta = <d, ck> + r_delta h (ipa.rs:147) and comm_LZ = <LZ, ck> + r_LZ h (hyrax_pc.rs:454-455) are table walks over the window tables of the
//     whole key (ck_key_tables: one launch each, no digits / sort / buckets / host Horner) on two streams side by side; LZ = L^T poly
//     (bind_with_delayed, :38-54) stays in device memory in front of its walk and travels to the host only for z_vec,
//   * the host meanwhile draws d_vec from the randomness stream (the wide reductions of E::Scalar::random), forms r_LZ = <L, blind>, <R, d> (tensor
//     form: n + sqrt(n) products) and beta.
// Transcript order and every value are the reference's. out = delta (8) | beta (8) | z_vec (4 * cols) | z_delta (4) | z_beta (4) words.
//
// Written like the batched opening beside it (capi_opening_batch.hip): one Shape, one state (Opening), the stages in the reference's order, each
// stated once; sp_hyrax_prove only says which stage runs when. This file defines no kernel and launches none itself: everything goes through the
// launchers of group_common.hpp. The host arithmetic (eq tables, folds, the tensor form of <R, d>) is opening_host.hpp.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "group_common.hpp"
#include "opening_host.hpp"

using sp::fail;
typedef FqP SF;
namespace oh = sp::host;

// ---- PCS::prove announced ahead ----------------------------------------------------------------------------------------------------------------
// src/spartan.rs calls PCS::prove last (:425-435), but three of its inputs exist long before: the commitment and its blinds when
// r1cs_instance_and_witness returns (:238-245), the IPA's randomness whenever the caller draws it (the reference draws inside
// InnerProductArgumentLinear::prove, ipa.rs:139-149: independent of everything), and the ROW half of the evaluation point when the inner sum-check has
// drawn it — rounds before its end. A caller (the shim's r1cs_instance_and_witness wrapper; prove_reference_order here) that announces the opening
// lets the library start under the sum-checks what sp_hyrax_prove would otherwise start behind them: the commitment's transcript encoding and its
// Keccak blocks + the mask vector's wide reductions (helper thread), delta's table walk (auxiliary stream, at once), and — when sp_sumcheck_quad on the
// same context reports the row challenges — L^T W and comm_LZ's walk. sp_hyrax_prove checks that what it is given is what was announced and then only
// collects; anything that does not match is dropped and computed as before. No protocol value changes: same group elements, same transcript bytes.
struct sp_pcs_ahead {
  // -- written by the CALLER's thread (the announcement, the sum-check's challenge hook, sp_hyrax_prove). The helper's jobs read them: a field is not
  //    written again once a job that reads it has been submitted (submit() publishes), until that job has been waited for.
  const sp_ck* ck = nullptr;
  const sp_table* poly = nullptr;
  size_t n = 0, npt = 0, nvr = 0, cols = 0, num_rows = 0;
  std::vector<aff_t> comm;
  std::vector<fe_t> blind, row_pt;
  std::vector<uint8_t> rng;
  fe_t r_delta;
  bool worker_busy = false;  // a job of this announcement may be running: wait() before the helper's fields below are read
  // <R, d> (ipa.rs:148) with R = eq(point[nvr..]) = left (x) right: T[b] = sum_a left[a] d[a * nright + b] once the first half of R's variables is drawn
  // col_pt collects the column challenges as they arrive; col_pt_T is the snapshot T was built from (frozen when the job is submitted): sp_hyrax_prove
  // compares ITS point with col_pt_T, so a later sum-check of the same length on this context — which overwrites col_pt — cannot make a stale T pass
  std::vector<fe_t> col_pt, col_pt_T;
  size_t hb = 0;
  bool T_submitted = false;
  // r_LZ = <eq(r_rows, .), blinds> is the blinds' multilinear extension at r_rows: the vector is folded by its top variable with every row challenge
  // (2^(nvr-k) products behind challenge k, under the device's next round), so that the last challenge leaves one product (hyrax_pc.rs:446-455)
  std::vector<fe_t> bfold;
  size_t rows_folded = 0;
  fe_t r_LZ;
  // With FixedBaseMul tables of the first `nfixed` commitment rows and of h (sp_hyrax_prove_announce_tables; the other rows are blind_i h by the caller's
  // word) comm_LZ = sum_{i < nfixed} L_i comm[i] + (sum_{i >= nfixed} L_i blind_i) h is ONE walk over those tables that needs L alone, not L^T W: it goes
  // out right behind the last row challenge instead of behind the 17-50 us matrix-vector product. eq(r_rows, .) is expanded a level per challenge
  // (P, new variable = index LSB, eq.rs:66-76); zfold = the zero rows' blinds folded like bfold gives h's scalar.
  const aff_t* row_tables = nullptr;
  size_t nfixed = 0;
  std::vector<fe_t> P, zfold, zfold_prev;
  bool lz_submitted = false;  // the launches behind the last row challenge are a job of the helper thread (the sum-check's thread goes on with its rounds)
  // z_vec = r LZ + d on the device (ipa.rs:160-163): the mask vector is uploaded behind delta's walk, the scaled sum lands in mapped memory
  fe_t* d_out = nullptr;  // [LZ (num_cols) | - | d (cols)] in the auxiliary lane's WS_ROWMAT_OUT
  bool z_fired = false;
  // -- written by the HELPER thread's jobs (job_announced: hashed .. seq_delta; job_partial_sums: T, T_ready; job_launch_lz: delta_j .. seq_lz). Plain
  //    fields: the caller's thread reads them only behind pcs_worker->wait() - the one at the top of pcs_ahead_drain, the one in front of the last row
  //    challenge's job, the one sp_hyrax_prove adopts the announcement with. (delta_collected is also set by sp_hyrax_prove, behind its wait.)
  sp::Keccak256State hashed;  // "poly_com" || commitment bytes hashed into a fresh sponge (valid when the transcript is fresh at the absorb: checked)
  std::vector<fe_t> dvec, T;
  bool delta_launched = false, T_ready = false, delta_collected = false;
  unsigned seq_delta = 0, seq_lz = 0;
  jac_t delta_j;
  // -- written by the helper thread's jobs and read by the sum-check's thread between its rounds WITHOUT a wait(): atomics, sequentially
  //    consistent - these are a handful of accesses per prove. What they announce (seq_lz behind lz_launched) is still read behind a wait() only.
  std::atomic<bool> lz_launched{false}, failed{false}, dvec_uploaded{false};
  std::atomic<unsigned> z_armed{0};  // sequence number of the k_scale_add_wait queued behind L^T W (0: none), released by sp_hyrax_prove's challenge or aborted
};

namespace {
const char* const MSG_LEN = "Hyrax prove: Expected 2^point.len() elements in poly";  // hyrax_pc.rs:400-408
// the polynomial as a num_rows x cols matrix over a key of num_cols columns, point = (nvr row variables | npt - nvr column variables)
struct Shape {
  size_t n, npt, nvr, cols, num_rows, num_cols;
};
// nullptr, or what sp_hyrax_prove says of a polynomial it cannot open (an announcement of one starts nothing ahead)
const char* shape_of(const sp_ck* ck, const sp_table* poly, size_t n, size_t rows, Shape* s) {
  s->n = n, s->num_cols = ck->num_cols, s->num_rows = (n + ck->num_cols - 1) / ck->num_cols;
  for (s->npt = 0; s->npt < 41 && ((size_t)1 << s->npt) < n;) ++s->npt;
  if (n != ((size_t)1 << s->npt) || n > poly->cap) return MSG_LEN;
  if (s->num_rows & (s->num_rows - 1)) return "Hyrax prove: the row count must be a power of two";
  if (rows != s->num_rows) return "Hyrax prove: one commitment row and one blind per matrix row";
  for (s->nvr = 0; ((size_t)1 << s->nvr) < s->num_rows;) ++s->nvr;
  s->cols = n / s->num_rows;  // |R| = |LZ| = |d|
  return nullptr;
}
// delta's walk reduces the randomness blocks itself (the wide kernel, the blocks within its scalar buffer): wide keys with window tables only
bool delta_takes_raw_blocks(const Shape& s) { return s.num_cols + 1 >= sp::multi_mul_wide_min() && 64 * s.num_cols <= sp::multi_mul_max_scalars() * sizeof(fe_t); }
// the event behind comm_LZ's walk and the pinned landing buffer of LZ
int landing_reserve(sp_ctx* c, size_t cols) {
  if (!c->pcs_ev) SP_HIP(hipEventCreateWithFlags(&c->pcs_ev, hipEventDisableTiming));
  if (c->h_pcs_bytes < cols * sizeof(fe_t)) {
    if (c->h_pcs) hipHostFree(c->h_pcs);
    c->h_pcs = nullptr;
    c->h_pcs_bytes = 0;
    SP_HIP(hipHostMalloc(&c->h_pcs, cols * sizeof(fe_t)));
    c->h_pcs_bytes = cols * sizeof(fe_t);
  }
  return SP_OK;
}
// L^T W: L | the partial products | LZ (num_cols scalars of the walk, its blind's slot, then - announced - the mask) on a lane's WS_ROWMAT_*
struct LzBufs {
  fe_t *dL, *part, *dout;
  size_t splits;  // row blocks of the partial products
  bool ok() const { return dL && part && dout; }
};
LzBufs lz_bufs(sp_ctx* c, const Shape& s, size_t out_elems, int lane) {
  LzBufs b;
  b.splits = s.num_rows < 64 ? s.num_rows : 64;
  b.dL = (fe_t*)c->workspace(sp_ctx::WS_ROWMAT_L, s.num_rows * sizeof(fe_t), lane);
  b.part = (fe_t*)c->workspace(sp_ctx::WS_ROWMAT_PART, b.splits * s.cols * sizeof(fe_t), lane);
  b.dout = (fe_t*)c->workspace(sp_ctx::WS_ROWMAT_OUT, out_elems * sizeof(fe_t), lane);
  return b;
}
// LZ = L^T W (hyrax_pc.rs:446-453) and comm_LZ's walk over the key's tables behind it (:454-455) on `st`, the stream of `lane`: eq(row point) -> dL,
// the tail of the walk's scalars zeroed, the product, the walk. key_tables == nullptr: comm_LZ's walk is out already (over the rows' own tables).
// More than 10 row variables do not fit the eq kernel's argument block, and the two callers differ there: the plain path hands over the table it has
// built on the host (L_host, which must outlive the stream's work) and it is uploaded; the helper's job has none and is refused.
// A failure means what the caller says it means: S->failed on the helper, sp_hyrax_prove's return value on the caller's thread.
int launch_lz(sp_ctx* c, int lane, hipStream_t st, const Shape& s, const fe_t* poly_d, const fe_t* row_pt, const fe_t* L_host, const LzBufs& b, const aff_t* key_tables,
              const fe_t* r_LZ, unsigned* seq) {
  if (s.nvr <= 10) sp::launch_eq_rows(st, row_pt, s.nvr, s.num_rows, b.dL);
  else if (!L_host) return SP_ERR_INTERNAL;
  else SP_HIP(hipMemcpyAsync(b.dL, L_host, s.num_rows * sizeof(fe_t), hipMemcpyHostToDevice, st));
  if (s.cols < s.num_cols) SP_HIP(hipMemsetAsync(b.dout + s.cols, 0, (s.num_cols - s.cols) * sizeof(fe_t), st));
  c->timed_on(st, "rowmat_vec", 32ull * (s.num_rows * s.cols + s.num_rows + s.cols), [&] { sp::launch_rowmat_vec(st, poly_d, s.num_rows, s.cols, b.dL, b.part, b.splits, b.dout); });
  return key_tables ? sp::multi_mul_launch(c, lane, key_tables, nullptr, s.num_cols + 1, seq, b.dout, r_LZ, 0) : SP_OK;
}
template <class T>
void wipe_vec(std::vector<T>& v) {
  if (!v.empty()) explicit_bzero(v.data(), v.size() * sizeof(T));
}
void abort_z(sp_ctx* c, sp_pcs_ahead* S) {  // a z_vec kernel that waits for a challenge which will not come leaves
  if (S->z_armed && !S->z_fired) {
    sp::scale_add_abort(c, S->z_armed);
    S->z_fired = true;
  }
}
// a launched L^T W + comm_LZ walk whose result nobody takes: its lane and its event are needed again
void drain_walk(sp_ctx* c, sp_pcs_ahead* S) {
  abort_z(c, S);
  jac_t sink;
  (void)sp::multi_mul_collect(c, 1, S->seq_lz, &sink, false);
  if (c->pcs_ev) (void)sp::event_sync(c->pcs_ev);
}
void pcs_ahead_drain(sp_ctx* c) {  // no device job of a dropped announcement may outlive it (its mapped result slot is reused)
  sp_pcs_ahead* S = c->pcs_ahead;
  if (!S) return;
  if (S->worker_busy && c->pcs_worker) c->pcs_worker->wait();
  abort_z(c, S);
  jac_t sink;
  if (S->delta_launched && !S->delta_collected) (void)sp::multi_mul_collect(c, 1, S->seq_delta, &sink, false);
  if (S->lz_launched) drain_walk(c, S);
}

// ---- the helper thread's jobs ---------------------------------------------------------------------------------------------------------------------
// the announcement's own: delta = <d, ck> + r_delta h first - its walk (auxiliary stream) reduces the randomness blocks itself -, then the commitment's
// transcript bytes into a fresh sponge, the mask vector's wide reductions, and the mask to the device behind delta's walk (needed when the IPA's
// challenge is drawn: z_vec = r LZ + d)
void job_announced(sp_ctx* c, sp_pcs_ahead* S) {
  const size_t num_cols = S->ck->num_cols;
  if (hipSetDevice(c->device) != hipSuccess ||
      sp::multi_mul_launch(c, 1, S->ck->d_keytables, reinterpret_cast<const uint64_t*>(S->rng.data()), num_cols + 1, &S->seq_delta, nullptr, &S->r_delta, S->cols))
    S->failed = true;
  else
    S->delta_launched = true;
  S->hashed.init();
  sp::absorb_commitment(S->hashed, S->comm.data(), S->comm.size());
  for (size_t i = 0; i < S->cols; ++i) S->dvec[i] = fe_from_uniform<SF>(S->rng.data() + 64 * i);
  fe_t* stage = reinterpret_cast<fe_t*>(c->h_pinned_vec) + c->h_pinned_vec_cols;
  memcpy(stage, S->dvec.data(), S->cols * sizeof(fe_t));
  if (!S->failed && hipMemcpyAsync(S->d_out + num_cols + 1, stage, S->cols * sizeof(fe_t), hipMemcpyHostToDevice, c->stream2) == hipSuccess) S->dvec_uploaded = true;
}
void job_partial_sums(sp_pcs_ahead* S) {  // behind the first half of the column challenges
  oh::tensor_partial_sums<SF>(S->col_pt_T.data(), S->hb, S->dvec.data(), S->cols, S->T);
  S->T_ready = true;
}
// Behind the last row challenge: delta's walk has had the whole outer sum-check and is collected (its lane's result slot is needed again), then L^T W and
// comm_LZ's walk go out on the same lane - half a dozen runtime calls, ~20 us, on the helper thread: the sum-check's next round is not held up by them.
void job_launch_lz(sp_ctx* c, sp_pcs_ahead* S) {
  const bool collect = S->delta_launched && !S->delta_collected;
  if (hipSetDevice(c->device) != hipSuccess || (collect && sp::multi_mul_collect(c, 1, S->seq_delta, &S->delta_j, false))) {
    S->failed = true;
    return;
  }
  if (collect) S->delta_collected = true;
  const Shape s{S->n, S->npt, S->nvr, S->cols, S->num_rows, S->ck->num_cols};
  const LzBufs b = lz_bufs(c, s, s.num_cols + 1 + s.cols, 1);
  if (!b.ok() || b.dout != S->d_out) {  // (sized by the announcement: a buffer that moved since would have lost the uploaded mask)
    S->failed = true;
    return;
  }
  bool walk_out = false;
  if (S->row_tables) {  // comm_LZ from the rows' own tables: the walk first, L^T W (needed for z_vec only) behind it
    const fe_t rl = S->row_pt[s.nvr - 1];
    const bool expand = S->nfixed + 1 < sp::multi_mul_wide_min() && S->zfold_prev.size() == 2;  // the last level of eq(r_rows, .) on the device (k_multi_mul_coop EXPAND)
    std::vector<fe_t> sc(expand ? (S->nfixed + 1) / 2 + 2 : S->nfixed + 1);
    if (expand) {
      memcpy(sc.data(), S->P.data(), (sc.size() - 2) * sizeof(fe_t));
      sc[sc.size() - 2] = S->zfold_prev[0];
      sc[sc.size() - 1] = S->zfold_prev[1];
    } else {
      oh::eq_expand<SF>(S->P.data(), S->P.size(), rl, sc.data(), S->nfixed);
      sc[S->nfixed] = S->zfold[0];
    }
    const int mrc = sp::multi_mul_launch(c, 1, S->row_tables, reinterpret_cast<const uint64_t*>(sc.data()), S->nfixed + 1, &S->seq_lz, nullptr, expand ? &rl : nullptr, 0, expand);
    wipe_vec(sc);
    if (mrc) {
      S->failed = true;
      return;
    }
    walk_out = true;
  }
  if (launch_lz(c, 1, c->stream2, s, S->poly->d, S->row_pt.data(), nullptr, b, walk_out ? nullptr : S->ck->d_keytables, &S->r_LZ, &S->seq_lz) ||
      hipEventRecord(c->pcs_ev, c->stream2) != hipSuccess) {
    S->failed = true;  // (a launched walk is still drained by pcs_ahead_drain: lz_launched stays false only if the launch itself failed)
    S->lz_launched = walk_out;
    return;
  }
  // z_vec's kernel waits for the IPA's challenge on the second auxiliary stream, behind this one's work so far. That stream is non-blocking: a waiting
  // kernel on a blocking stream would hold up every legacy default-stream operation of the process (a synchronous hipMemcpy between the sum-check and
  // the opening) until its watchdog.
  if (S->dvec_uploaded && c->stream3 && hipStreamWaitEvent(c->stream3, c->pcs_ev, 0) == hipSuccess)
    S->z_armed = sp::scale_add_arm(c, c->stream3, b.dout, b.dout + s.num_cols + 1, s.cols);
  S->lz_launched = true;
}

// ---- the inner sum-check's challenges: round 0 binds the variable that separates W from (1, X); rounds 1 .. nvr are the opening's row variables ------
// a column variable: after the first half of them the helper thread forms the partial sums of <R, d>
void on_column_challenge(sp_ctx* c, sp_pcs_ahead* S, size_t k, const uint64_t r[4]) {
  if (k < S->hb) memcpy(&S->col_pt[k], r, 32);
  if (k + 1 != S->hb || S->T_submitted) return;
  if (S->worker_busy) c->pcs_worker->wait();
  S->worker_busy = true;
  S->T_submitted = true;
  S->col_pt_T = S->col_pt;
  c->pcs_worker->submit([S] { job_partial_sums(S); });
}
// a row variable: the blinds (and, with tables, the zero rows' blinds) folded by it, eq(r_rows, .) a level further
void fold_row_challenge(sp_pcs_ahead* S, size_t round) {
  const fe_t rk = S->row_pt[round - 1];
  oh::fold_top<SF>(S->bfold, rk);
  S->rows_folded = round;
  if (!S->row_tables) return;
  if (S->zfold.size() == 2) S->zfold_prev = S->zfold;  // (S0, S1): h's scalar is S0 + r (S1 - S0), which the walk's kernel can form itself
  oh::fold_top<SF>(S->zfold, rk);
  if (round < S->nvr) {  // (the last level is the helper job's: 2^(nvr-1) products)
    std::vector<fe_t> Q(2 * S->P.size());
    oh::eq_expand<SF>(S->P.data(), S->P.size(), rk, Q.data());
    S->P.swap(Q);
  }
}
}  // namespace

namespace sp {
bool pcs_ahead_wants(const sp_ctx* c, size_t rounds) { return c->pcs_ahead && !c->pcs_ahead->failed && rounds == c->pcs_ahead->npt + 1; }
// The announcement holds zero-knowledge material for the span of both sum-checks (the commitment's blinds, the IPA's randomness blocks and the mask
// vector drawn from them, the partial sums of <R, d>, r_delta, r_LZ): wiped before the memory goes back to the allocator.
void pcs_ahead_free(sp_ctx* c) {
  if (!c || !c->pcs_ahead) return;
  pcs_ahead_drain(c);
  sp_pcs_ahead* S = c->pcs_ahead;
  c->pcs_ahead = nullptr;
  if (S->dvec_uploaded && S->d_out && c->h_pinned_vec) {
    // a dropped or retracted announcement had staged the mask vector (pinned block) and uploaded it (auxiliary stream): neither copy outlives it.
    // (a consumed one has wiped both already - sp_hyrax_prove - and wiping zeros again costs a 64 KiB memset off everybody's path)
    (void)sp::stream_sync(c->stream2);
    sp::addend_wipe(c, S->d_out + S->ck->num_cols + 1, S->cols, c->stream2);
  }
  auto wipe = [S] {
    for (std::vector<fe_t>* v : {&S->blind, &S->dvec, &S->T, &S->bfold, &S->zfold, &S->zfold_prev}) wipe_vec(*v);
    wipe_vec(S->rng);
    explicit_bzero(&S->r_delta, sizeof(fe_t));
    explicit_bzero(&S->r_LZ, sizeof(fe_t));
    delete S;
  };
  // ~250 KB at config 2: 15-20 us of stores, on the context's helper thread when there is one (nothing else of the announcement is alive: drained above)
  if (c->pcs_worker) c->pcs_worker->submit(wipe);
  else wipe();
}
void pcs_ahead_on_challenge(void* ctx, size_t round, const uint64_t r[4]) {
  sp_ctx* c = (sp_ctx*)ctx;
  sp_pcs_ahead* S = c->pcs_ahead;
  if (!S || S->failed || S->nvr == 0 || round == 0) return;
  if (round > S->nvr) return on_column_challenge(c, S, round - S->nvr - 1, r);
  if (S->lz_submitted || S->lz_launched) return;  // (lz_submitted first: while it is false no helper job is writing lz_launched)
  if (round != S->rows_folded + 1) {  // (challenges arrive in order, once each; anything else and the plain call computes everything itself)
    S->failed = true;
    return;
  }
  memcpy(&S->row_pt[round - 1], r, 32);
  if (round == 1 && c->pcs_worker) c->pcs_worker->keep_hot(700);  // the jobs below and the opening's own are claimed without a wake-up
  fold_row_challenge(S, round);
  if (round != S->nvr) return;
  S->r_LZ = S->bfold[0];
  if (S->worker_busy) {  // the announcement's helper job (it launched delta's walk on this lane)
    c->pcs_worker->wait();
    S->worker_busy = false;
  }
  if (S->failed || S->nvr > 10) {  // (launch_lz would refuse a helper's job of more than 10 row variables: not submitted)
    S->failed = true;
    return;
  }
  S->lz_submitted = true;
  S->worker_busy = true;
  c->pcs_worker->submit([S, c] { job_launch_lz(c, S); });
}
}  // namespace sp

extern "C" int sp_hyrax_prove_retract(sp_ctx* c) {
  if (!c) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_hyrax_prove_retract: null context");
  sp::pcs_ahead_free(c);
  return SP_OK;
}
static int announce_impl(sp_ctx* c, const sp_ck* ck, const uint64_t* comm_rows_aff, size_t rows, const sp_table* poly, size_t n, const uint64_t* blinds, const uint8_t* rng,
                         size_t rng_blocks, const sp_fbtables* row_tables, size_t nfixed) {
  if (!c || !ck || !comm_rows_aff || !poly || !blinds || !rng) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_hyrax_prove_announce: null argument");
  sp::pcs_ahead_free(c);  // at most one announcement per context; an unconsumed one is dropped
  Shape s;
  if (shape_of(ck, poly, n, rows, &s) || s.num_rows < 2) return SP_OK;  // nothing to start ahead: the plain call decides
  if (rng_blocks < s.cols + 2 || s.nvr > 10) return SP_OK;
  SP_HIP(hipSetDevice(c->device));
  if (sp::ck_key_tables(c, ck) != 0) return SP_OK;  // no window tables of the key: the bucket MSMs have nothing to gain from an early start of this kind
  if (!delta_takes_raw_blocks(s)) return SP_OK;
  if (int rc = landing_reserve(c, s.cols)) return rc;
  sp_pcs_ahead* S = new sp_pcs_ahead();
  S->ck = ck;
  S->poly = poly;
  S->n = n, S->npt = s.npt, S->nvr = s.nvr, S->cols = s.cols, S->num_rows = s.num_rows;
  S->comm.assign(reinterpret_cast<const aff_t*>(comm_rows_aff), reinterpret_cast<const aff_t*>(comm_rows_aff) + rows);
  S->blind.assign(reinterpret_cast<const fe_t*>(blinds), reinterpret_cast<const fe_t*>(blinds) + rows);
  S->rng.assign(rng, rng + 64 * (s.cols + 2));
  S->row_pt.resize(s.nvr);
  S->hb = (s.npt - s.nvr) / 2;
  S->col_pt.resize(S->hb ? S->hb : 1);
  S->dvec.resize(s.cols);
  S->r_delta = fe_from_uniform<SF>(S->rng.data() + 64 * s.cols);
  S->bfold = S->blind;
  // (tables still being built - sp_fbtables_create_async a moment ago - are not waited for: this opening takes the walk over the key instead)
  if (row_tables && nfixed >= 1 && nfixed + 1 <= sp::multi_mul_max_scalars() && sp_fbtables_ready(row_tables, 0) == 1) {
    S->row_tables = row_tables->d_tables;
    S->nfixed = nfixed;
    S->zfold = S->blind;
    for (size_t i = 0; i < nfixed; ++i) S->zfold[i] = fe_zero();
    S->P.assign(1, fe_one<SF>());
  }
  // the buffers of the launches behind the last row challenge and of z_vec, sized here: the helper thread's workspace() calls are then plain look-ups
  const int rc_pin = sp::ensure_pinned_vec(c, s.cols);
  const LzBufs b = lz_bufs(c, s, s.num_cols + 1 + s.cols, 1);
  if (rc_pin || !b.ok()) {
    delete S;
    return SP_OK;  // the plain call will report what is wrong
  }
  S->d_out = b.dout;
  c->pcs_ahead = S;
  if (!c->pcs_worker) c->pcs_worker = new sp::Worker();
  S->worker_busy = true;
  c->pcs_worker->submit([S, c] { job_announced(c, S); });
  return SP_OK;
}
extern "C" int sp_hyrax_prove_announce(sp_ctx* c, const sp_ck* ck, const uint64_t* comm_rows_aff, size_t rows, const sp_table* poly, size_t n, const uint64_t* blinds,
                                       const uint8_t* rng, size_t rng_blocks) {
  return announce_impl(c, ck, comm_rows_aff, rows, poly, n, blinds, rng, rng_blocks, nullptr, 0);
}
extern "C" int sp_hyrax_prove_announce_tables(sp_ctx* c, const sp_ck* ck, const uint64_t* comm_rows_aff, size_t rows, const sp_table* poly, size_t n, const uint64_t* blinds,
                                              const uint8_t* rng, size_t rng_blocks, const sp_fbtables* row_tables, size_t nfixed) {
  if (!row_tables || row_tables->n != nfixed + 1 || nfixed > rows)
    return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_hyrax_prove_announce_tables: one table per fixed row and one of h");
  return announce_impl(c, ck, comm_rows_aff, rows, poly, n, blinds, rng, rng_blocks, row_tables, nfixed);
}

// ---- sp_hyrax_prove: one state, the stages in the order of hyrax_pc.rs:387-478 and ipa.rs:125-170 -----------------------------------------------------
namespace {
struct Opening {
  // inputs
  sp_ctx* c;
  const sp_ck *ck, *ck_eval;
  sp_transcript* tr;
  const aff_t* comm;
  size_t rows;
  const sp_table* poly;
  const fe_t *blind, *pt;
  const uint8_t* rng;
  Shape s;
  aff_t comm_eval;
  // E::Scalar::random draws (ipa.rs:139-149): d_vec, then the blinds of delta and beta, each the wide reduction of 64 uniform bytes. The two blinds at
  // once, the mask vector (draw_mask) while the device already works on LZ.
  fe_t b_eval, r_delta, r_beta;
  // decisions. S != nullptr ("ahead"): the announcement is this opening's - hashing, mask and delta are done or under way; lz_ahead: so are L^T W and
  // comm_LZ; hashed_ahead: its sponge is installed; walk: the key has window tables; beta_beside: beta's two walks run on the helper thread
  sp_pcs_ahead* S = nullptr;
  bool walk = false, lz_ahead = false, hashed_ahead = false, beta_beside = false;
  unsigned seq_delta = 0, seq_lz = 0;
  sp_msm_job* delta_job = nullptr;  // (the bucket MSM of a key without tables)
  sp::Keccak256State hashed;
  std::vector<fe_t> L, LZ, dvec_own;
  const std::vector<fe_t>* dvec = nullptr;  // the announcement's or dvec_own
  // results
  fe_t r_LZ, ip, rr;
  jac_t beta_h = jac_identity(), beta_c = jac_identity();
  aff_t comm_LZ, delta, beta;
  // SPARTAN_HOST_LAPS: the host time of every stage on stderr
  bool laps = false;
  double t_lap = 0;
  static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void lap(const char* what) {
    if (!laps) return;
    const double t = now_us();
    fprintf(stderr, "  hyrax_prove lap %-24s %8.1f us\n", what, t - t_lap);
    t_lap = t;
  }
  bool z_on_device() const { return lz_ahead && S->dvec_uploaded; }  // (an announced opening forms z_vec on the device: LZ never comes to the host)
  void drop_announcement() {
    sp::pcs_ahead_free(c);
    S = nullptr;
  }
  void adopt_or_drop_announcement();
  void start_hashing();
  int start_delta();
  int start_lz();
  int draw_mask();
  void inner_product();
  int start_beta();
  int collect_walks();
  int z_vec(uint64_t* out_z);
};
// (0) was this opening announced (sp_hyrax_prove_announce)? Then its commitment hashing, mask vector, delta and — if the inner sum-check reported the row
// challenges — L^T W and comm_LZ are done or under way; anything that differs from what was announced drops the announcement.
void Opening::adopt_or_drop_announcement() {
  sp_pcs_ahead* A = c->pcs_ahead;
  const bool ahead = A && !A->failed && A->ck == ck && A->poly == poly && A->n == s.n && A->comm.size() == rows && memcmp(A->comm.data(), comm, rows * sizeof(aff_t)) == 0 &&
                     memcmp(A->blind.data(), blind, rows * sizeof(fe_t)) == 0 && memcmp(A->rng.data(), rng, 64 * (s.cols + 2)) == 0;
  if (A && !ahead) sp::pcs_ahead_free(c);
  tr->join();
  if (!c->pcs_worker) c->pcs_worker = new sp::Worker();
  if (!ahead) return;
  S = A;
  c->pcs_worker->wait();
  S->worker_busy = false;
  if (S->failed || !S->delta_launched) drop_announcement();  // the helper could not launch delta's walk: as if nothing had been announced
}
// (1) helper thread: transcript.absorb(b"poly_com", comm) (hyrax_pc.rs:410) into a copy of the running hasher, installed at the join; then h's half of beta
void Opening::start_hashing() {
  hashed = tr->t.h;
  if (S) {  // the announced hashing started from a fresh sponge: usable exactly when nothing has been absorbed since the last squeeze
    bool fresh = tr->t.h.fill == 0;
    for (int i = 0; i < 25 && fresh; ++i) fresh = tr->t.h.a[i] == 0;
    if (fresh) hashed = S->hashed;
    hashed_ahead = fresh;
  }
  if (!hashed_ahead) c->pcs_worker->submit([hp = &hashed, comm = comm, rows = rows] { sp::absorb_commitment(*hp, comm, rows); });
  // beta = ck_c <R, d> + h r_beta (ipa.rs:149) is two table walks on the host, ~11 us each. With the helper thread polling (an announced opening keeps it
  // so) and not busy with the commitment's hashing, h's walk runs beside this thread's compare / <R, d> and ck_c's beside its collection of the two device
  // walks; otherwise both are this thread's (sp_hyrax_commit_small). The jobs write into the state, which outlives the join on every exit path.
  beta_beside = hashed_ahead && ck_eval->n_tables >= 2 && ck_eval->num_cols >= 1 && c->pcs_worker->hot();
  if (beta_beside) c->pcs_worker->submit([ck_eval = ck_eval, dst = &beta_h, rb = r_beta] { *dst = sp::ck_table_mul_host(ck_eval, ck_eval->n_tables - 1, rb); });
  lap("submit hashing");
}
// (2) device: delta = <d, ck> + r_delta h (ipa.rs:147) on the auxiliary stream first: it needs nothing but the randomness stream, whose blocks the walk
// reduces itself. Keys it cannot (no tables, narrow) start delta from the drawn mask (draw_mask).
int Opening::start_delta() {
  const int kt = (s.nvr == 0 && s.cols > s.num_cols) ? 1 : sp::ck_key_tables(c, ck);
  if (kt < 0) return kt;
  walk = kt == 0;
  if (S && !walk) drop_announcement();  // (cannot happen: the announcement needs the key's window tables)
  int rc;
  if (S) seq_delta = S->seq_delta;
  else if (walk && delta_takes_raw_blocks(s) &&
           (rc = sp::multi_mul_launch(c, 1, ck->d_keytables, reinterpret_cast<const uint64_t*>(rng), s.num_cols + 1, &seq_delta, nullptr, &r_delta, s.cols)))
    return rc;
  lap("delta launch");
  return SP_OK;
}
// LZ = L^T W, r_LZ = <L, blind>, comm_LZ = <LZ, ck> + r_LZ h (hyrax_pc.rs:417-455): the row itself / what the announcement launched / this call's own
int Opening::start_lz() {
  int rc;
  if (s.nvr == 0) {  // a single row: the commitment is the row itself (hyrax_pc.rs:417-423)
    comm_LZ = comm[0];
    LZ.resize(s.cols);
    if ((rc = sp_table_read(c, poly, 0, s.n, reinterpret_cast<uint64_t*>(LZ.data())))) return rc;
    r_LZ = blind[0];
  } else if (S && S->lz_launched && memcmp(S->row_pt.data(), pt, s.nvr * sizeof(fe_t)) == 0) {
    lz_ahead = true;  // L^T W and comm_LZ's walk have been running on the auxiliary stream since the inner sum-check drew the row challenges
    r_LZ = S->r_LZ;
    seq_lz = S->seq_lz;
  } else {
    L.resize((size_t)1 << s.nvr);
    oh::eq_table<SF>(pt, s.nvr, L.data());
    LZ.resize(s.cols);
    if (S && S->lz_launched) {  // started for other row challenges than the point given now: drain it, its lane is needed
      drain_walk(c, S);
      S->lz_launched = false;
    }
    r_LZ = fe_zero();
    for (size_t i = 0; i < s.num_rows; ++i) r_LZ = fe_add<SF>(r_LZ, fe_mul<SF>(L[i], blind[i]));
    if (walk) {
      if ((rc = landing_reserve(c, s.cols))) return rc;
      const LzBufs b = lz_bufs(c, s, s.num_cols + 1, 0);
      if (!b.ok()) return SP_ERR_NO_DEVICE;
      // (L outlives the stream's work: collect_walks joins it)
      if ((rc = launch_lz(c, 0, c->stream, s, poly->d, pt, L.data(), b, ck->d_keytables, &r_LZ, &seq_lz))) return rc;
      SP_HIP(hipMemcpyAsync(c->h_pcs, b.dout, s.cols * sizeof(fe_t), hipMemcpyDeviceToHost, c->stream));  // behind the walk: LZ is needed on the host only for z_vec
      SP_HIP(hipEventRecord(c->pcs_ev, c->stream));
    } else if ((rc = sp_rowmat_vec(c, poly, s.num_rows, s.cols, reinterpret_cast<const uint64_t*>(L.data()), reinterpret_cast<uint64_t*>(LZ.data())))) {
      return rc;
    }
  }
  lap("LZ + comm_LZ launch");
  return SP_OK;
}
// d_vec: 2048 wide reductions at config 2, ~65 us of host work beside the device's (delta's walk reduces its own copy of the blocks); then the delta
// that starts from the drawn scalars
int Opening::draw_mask() {
  if (!S) {  // (an announcement's helper job has drawn it)
    dvec_own.resize(s.cols);
    for (size_t i = 0; i < s.cols; ++i) dvec_own[i] = fe_from_uniform<SF>(rng + 64 * i);
  }
  dvec = S ? &S->dvec : &dvec_own;
  lap("d_vec draw");
  if (!walk) return sp_msm_ck_begin(c, ck, reinterpret_cast<const uint64_t*>(dvec->data()), s.cols, &delta_job);
  if (delta_takes_raw_blocks(s) || S) return SP_OK;
  std::vector<fe_t> sc(s.num_cols + 1, fe_zero());  // narrow keys: the walk from the drawn scalars
  memcpy(sc.data(), dvec->data(), s.cols * sizeof(fe_t));
  sc[s.num_cols] = r_delta;
  return sp::multi_mul_launch(c, 1, ck->d_keytables, reinterpret_cast<const uint64_t*>(sc.data()), s.num_cols + 1, &seq_delta, nullptr, nullptr, 0);
}
// (3) host work under the device's: <R, d> with R = eq(point[nvr..]) = left (x) right (ipa.rs:148): closed over the announcement's partial sums when
// it formed them from this point's first half, row by row otherwise (through the partial sums the unannounced openings of a batch measured slower:
// profiles/opening_refactor.md)
void Opening::inner_product() {
  const size_t k = s.npt - s.nvr, hb = k / 2;
  if (S && S->T_ready && S->hb == hb && S->col_pt_T.size() >= hb && memcmp(S->col_pt_T.data(), pt + s.nvr, hb * sizeof(fe_t)) == 0)
    ip = oh::tensor_close<SF>(pt + s.nvr + hb, k - hb, S->T.data());
  else
    ip = oh::tensor_inner_product<SF>(pt + s.nvr, k, dvec->data());
  lap("<R, d>");
}
// beta = ck_c * <R, d> + h_c * r_beta (ipa.rs:149)
int Opening::start_beta() {
  if (beta_beside) {
    c->pcs_worker->wait(1);  // h's walk (an unclaimed job is taken back and run here)
    c->pcs_worker->submit([ck_eval = ck_eval, dst = &beta_c, ipv = ip] { *dst = sp::ck_table_mul_host(ck_eval, 0, ipv); });
  } else if (int rc = sp_hyrax_commit_small(c, ck_eval, reinterpret_cast<const uint64_t*>(&ip), 1, reinterpret_cast<const uint64_t*>(&r_beta), reinterpret_cast<uint64_t*>(&beta))) {
    return rc;
  }
  lap("beta");
  return SP_OK;
}
// (4) joins: delta, comm_LZ, LZ (for a z_vec formed on the host), beta
int Opening::collect_walks() {
  int rc;
  if (walk) {
    jac_t dj;
    if (S && S->delta_collected) {
      dj = S->delta_j;
    } else {
      if ((rc = sp::multi_mul_collect(c, 1, seq_delta, &dj, false))) return rc;
      if (S) S->delta_collected = true;
    }
    delta = jac_to_affine(dj);
    if (s.nvr != 0) {
      jac_t lj;
      if ((rc = sp::multi_mul_collect(c, lz_ahead ? 1 : 0, seq_lz, &lj, false))) return rc;
      if (lz_ahead) S->lz_launched = false;
      comm_LZ = jac_to_affine(lj);
      if (!z_on_device()) {
        if (lz_ahead) {
          LZ.resize(s.cols);
          SP_HIP(hipMemcpyAsync(c->h_pcs, S->d_out, s.cols * sizeof(fe_t), hipMemcpyDeviceToHost, c->stream2));
          SP_HIP(hipEventRecord(c->pcs_ev, c->stream2));
        }
        SP_HIP(sp::event_sync(c->pcs_ev));
        memcpy(LZ.data(), c->h_pcs, s.cols * sizeof(fe_t));
      }
    }
  } else {
    if (s.nvr != 0 && (rc = sp_msm_ck(c, ck, reinterpret_cast<const uint64_t*>(LZ.data()), s.cols, reinterpret_cast<const uint64_t*>(&r_LZ), reinterpret_cast<uint64_t*>(&comm_LZ))))
      return rc;
    sp_msm_job* j = delta_job;
    delta_job = nullptr;
    if ((rc = sp_msm_ck_finish(c, ck, j, reinterpret_cast<const uint64_t*>(&r_delta), reinterpret_cast<uint64_t*>(&delta)))) return rc;
  }
  if (beta_beside) {
    c->pcs_worker->wait(1);
    beta = jac_to_affine(jac_add(beta_c, beta_h));
  }
  lap("join walks");
  return SP_OK;
}
// (6) z_vec = r * LZ + d (ipa.rs:160-163)
int Opening::z_vec(uint64_t* out_z) {
  if (z_on_device()) {
    // behind comm_LZ's walk on the auxiliary stream (collected): one launch, armed ahead or not, the sum lands in mapped memory (2048 products on this
    // thread and its helper were ~32 us); then the consumed mask's two copies go
    fe_t* d_mask = S->d_out + s.num_cols + 1;
    const bool armed = S->z_armed && !S->z_fired;
    if (armed) S->z_fired = true;
    const int rc = armed ? sp::scale_add_fire(c, c->stream3, S->z_armed, S->d_out, d_mask, rr, s.cols, out_z, "hyrax_prove z_vec")
                         : sp::scale_add_to_host(c, c->stream2, S->d_out, d_mask, rr, s.cols, out_z, "hyrax_prove z_vec");
    if (rc) return rc;
    sp::addend_wipe(c, d_mask, s.cols, c->stream2);
    S->dvec_uploaded = false;  // (both copies are gone: pcs_ahead_free has nothing left to wipe)
    return SP_OK;
  }
  // on the host, shared with the helper thread chunk by chunk: whoever is awake takes the next 128 elements. The owner never waits for the helper to WAKE
  // (a sleeping thread can take milliseconds when the process is at its CPU quota), only for chunks the helper has actually claimed.
  struct Share {
    std::atomic<size_t> next{0}, done{0};
  };
  auto sh = std::make_shared<Share>();
  constexpr size_t CH = 128;
  const size_t cols = s.cols, nch = (cols + CH - 1) / CH;
  auto work = [sh, zv = reinterpret_cast<fe_t*>(out_z), lz = LZ.data(), dv = dvec->data(), rr = rr, cols, nch] {
    for (;;) {
      const size_t ci = sh->next.fetch_add(1, std::memory_order_acq_rel);
      if (ci >= nch) return;
      const size_t hi = (ci + 1) * CH < cols ? (ci + 1) * CH : cols;
      for (size_t i = ci * CH; i < hi; ++i) zv[i] = fe_add<SF>(fe_mul<SF>(rr, lz[i]), dv[i]);
      sh->done.fetch_add(1, std::memory_order_acq_rel);
    }
  };
  if (nch > 2) c->pcs_worker->submit(work);
  work();
  while (sh->done.load(std::memory_order_acquire) < nch) sp::relax();
  return SP_OK;
}
}  // namespace

extern "C" int sp_hyrax_prove(sp_ctx* c, const sp_ck* ck, const sp_ck* ck_eval, sp_transcript* tr, const uint64_t* comm_rows_aff, size_t rows, const sp_table* poly, size_t n,
                              const uint64_t* blinds, const uint64_t* point, size_t npt, const uint64_t comm_eval_aff[8], const uint64_t blind_eval[4], const uint8_t* rng,
                              size_t rng_blocks, uint64_t* out) {
  if (!c || !ck || !ck_eval || !tr || !comm_rows_aff || !poly || !blinds || (!point && npt) || !comm_eval_aff || !blind_eval || !rng || !out)
    return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_hyrax_prove: null argument");
  if (npt > 40 || n != ((size_t)1 << npt)) return fail(SP_ERR_INVALID_INPUT_LENGTH, MSG_LEN);
  Opening o{c, ck, ck_eval, tr, reinterpret_cast<const aff_t*>(comm_rows_aff), rows, poly, reinterpret_cast<const fe_t*>(blinds), reinterpret_cast<const fe_t*>(point), rng};
  if (const char* why = shape_of(ck, poly, n, rows, &o.s)) return fail(SP_ERR_INVALID_INPUT_LENGTH, why);
  if (!ck_eval->d_cktables || ck_eval->num_cols < 1) return fail(SP_ERR_INVALID_INPUT_LENGTH, "Hyrax prove: ck_eval must be a narrow key with tables");
  SP_HIP(hipSetDevice(c->device));
  static const bool laps = getenv("SPARTAN_HOST_LAPS") != nullptr;
  o.laps = laps;
  if (laps) o.t_lap = Opening::now_us();
  const size_t cols = o.s.cols;
  if (rng_blocks < cols + 2) return fail(SP_ERR_INVALID_INPUT_LENGTH, "Hyrax prove: the randomness stream holds fewer than cols + 2 blocks");
  o.r_delta = fe_from_uniform<SF>(rng + 64 * cols), o.r_beta = fe_from_uniform<SF>(rng + 64 * (cols + 1));
  memcpy(&o.b_eval, blind_eval, 32);
  memcpy(&o.comm_eval, comm_eval_aff, sizeof(aff_t));

  struct AheadDone {  // consumed or not, the announcement ends with this call
    sp_ctx* c;
    ~AheadDone() { sp::pcs_ahead_free(c); }
  } ahead_done{c};
  o.adopt_or_drop_announcement();
  struct Join {  // the hashing job reads `comm` and writes `hashed`: it must have finished on every exit path (not so the z_vec helper job at the end)
    sp::Worker* w;
    bool joined = false;
    ~Join() {
      if (!joined) w->wait();
    }
  } join{c->pcs_worker};
  struct JobGuard {  // an error exit must not leave the asynchronous MSM of the fallback path outstanding
    sp_ctx* c;
    sp_msm_job*& j;
    ~JobGuard() {
      uint64_t sink[8];
      if (j) sp_msm_job_finish(c, j, sink);
      j = nullptr;
    }
  } job_guard{c, o.delta_job};
  int rc;
  o.start_hashing();
  if ((rc = o.start_delta()) || (rc = o.start_lz()) || (rc = o.draw_mask())) return rc;
  o.inner_product();
  if ((rc = o.start_beta()) || (rc = o.collect_walks())) return rc;
  if (!o.hashed_ahead) c->pcs_worker->wait();
  join.joined = true;
  o.lap("join hashing");
  tr->t.h = o.hashed;
  // (5) InnerProductArgumentLinear::prove, transcript part (ipa.rs:132-158)
  if (!sp::ipa_transcript(tr->t, o.comm_LZ, o.comm_eval, o.delta, o.beta, &o.rr)) return fail(SP_ERR_INTERNAL_TRANSCRIPT, "transcript round counter overflow");
  // (6) z_vec = r * LZ + d, z_delta = r * r_LZ + r_delta, z_beta = r * blind_eval + r_beta (ipa.rs:160-168)
  memcpy(out, &o.delta, sizeof(aff_t));
  memcpy(out + 8, &o.beta, sizeof(aff_t));
  if ((rc = o.z_vec(out + 16))) return rc;
  fe_t* zv = reinterpret_cast<fe_t*>(out + 16);
  zv[cols] = fe_add<SF>(fe_mul<SF>(o.rr, o.r_LZ), o.r_delta);
  zv[cols + 1] = fe_add<SF>(fe_mul<SF>(o.rr, o.b_eval), o.r_beta);
  o.lap("transcript + z_vec");
  return SP_OK;
}
