// sp_hyrax_prove_batch (include/spartan_hip.h): `count` instances of HyraxPCS::prove (hyrax_pc.rs:387-478) + InnerProductArgumentLinear::prove
// (ipa.rs:125-170) on one commitment key, opened in one pass. sp_hyrax_prove (capi_opening.hip) is latency-shaped: two 65-block table walks, one L^T W,
// ~65 us of host mask draws and a 32 KiB Keccak per opening, hidden under the sum-checks by an announcement that exists once per context. A batch has
// no sum-check to hide under, so here every device stage is ONE plain launch for all instances (kernels_opening_batch.hpp) on the main stream:
//   upload (blocks, instances, points) -> k_ob_mask -> copy of the <R, d> block sums, event
//                                      -> k_ob_rowmat -> k_ob_walk -> copy of the 2 count Jacobian sums
//   host, per instance, on the polling host threads (sp_host_parallel_for; woken for the length of the call by sp_walkers_keep_hot before the uploads,
//   since a region posted to sleeping walkers is run by its owner alone; the calling thread alone with SPARTAN_WALKERS=0):
//     before the uploads         r_LZ = <eq(row point), blinds>
//     while the device works     the commitment's transcript bytes + Keccak blocks into a copy of the hasher
//     behind the event           beta = ck_c <R, d> + h r_beta over the host tables
//     behind the walks           the IPA's absorbs and the squeeze of r, z_delta, z_beta
//   k_ob_z -> copy of z_vec, wait, wipe.
// No resident kernel, no mailbox, no polled slot, no announcement. Every value is the one sp_hyrax_prove computes (group sums as canonical affine
// points, exact field arithmetic), so the words, the blocks consumed and the transcripts are those of `count` lone calls. gfx950 only; no CPU fallback.
//
// sp_hyrax_prove_batch_begin / _rows / _finish: the same opening for a caller that HAS sum-checks to hide it under (prove_batch). Most of it needs
// nothing from them, so it is cut where its inputs become known, and everything the job queues goes to the context's auxiliary stream:
//   _begin   (commitments, blinds, randomness)   upload -> k_ob_dvec -> k_ob_walk over the delta vectors (ipa.rs:139-147); the commitments'
//                                                transcript bytes + Keccak blocks into FRESH sponges on the context's helper thread (hyrax_pc.rs:410)
//   _rows    (row half of every point)           r_LZ on the host, upload -> k_ob_rowmat -> k_ob_walk over the comm_LZ vectors (hyrax_pc.rs:446-455)
//   _finish  (everything)                        compare; k_ob_ip -> <R, d>, beta, the IPA's transcript part per instance, k_ob_z (ipa.rs:148-168)
// _finish uses what the job holds only if it was made from what _finish is given (key, tables, commitment words, blinds, randomness blocks, row
// challenges - compared by value) and runs sp_hyrax_prove_batch otherwise; a sponge hashed ahead is installed only into a transcript that has absorbed
// nothing since its last squeeze. One job per context: it owns the WS_OPENING_* workspaces and the pinned buffer until _finish or _drop.
//
// Both forms are written over the same pieces, each stated once below: the buffers (Plan), where an instance's inputs live (Inputs: the caller's
// arguments, or the job's own copies), the host stages per instance, the uploads, one launcher per kernel that both forms launch, the tail and the
// wipe, each taking the stream through the Run it is given. What differs stays in the entry points: which kernels, on which stream, in what order.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "group_common.hpp"
#include "kernels_opening_batch.hpp"

using sp::fail;
typedef spk::SF SF;
static_assert(SP_LOCKSTEP_MAX == spk::OB_MAX, "the challenge argument holds SP_LOCKSTEP_MAX instances");

namespace {
const char* const WHO = "sp_hyrax_prove_batch";

struct Shape {
  size_t count, rows, n, npt, nvr, cols, num_cols;
};
// one instance's host-side state between the stages
struct Item {
  sp::Keccak256State hashed;
  fe_t r_delta, r_beta, r_LZ, ip, r;
  aff_t beta;
  int rc = SP_OK;
};
// where an instance's inputs are read from: the caller's arguments, or the copies a job opened ahead owns
struct Inputs {
  const aff_t* comm[spk::OB_MAX];    // rows commitment rows
  const fe_t* blinds[spk::OB_MAX];   // rows blinds
  const uint8_t* rng[spk::OB_MAX];   // cols + 2 uniform blocks
  const fe_t* poly_d[spk::OB_MAX];   // poly->d
};
// the buffers of one opening. Device: WS_OPENING_BLOCKS | WS_OPENING_VECS (d, LZ, z) | WS_OPENING_PARAMS (instances, points) | WS_OPENING_WALK
// (tickets, block sums, sums, ip block sums). Pinned: [blocks | one params slot per upload | ip block sums | walk sums | z] - with a slot of its own,
// a stage never rewrites what an earlier stage's copy may still read
struct Plan {
  char *d_blocks = nullptr, *d_params = nullptr;
  fe_t *d_d = nullptr, *d_lz = nullptr, *d_z = nullptr, *d_ip = nullptr;
  unsigned* d_ticket = nullptr;
  xyzz_t* d_part = nullptr;
  jac_t* d_sums = nullptr;  // delta_0 .. delta_(count-1), then comm_LZ_0 .. (two or more rows)
  size_t blocks_bytes = 0, vec_bytes = 0, inst_bytes = 0, params_bytes = 0, ip_bytes = 0, sums_bytes = 0, tick_bytes = 0, nb_ip = 0;
  size_t off_params[3] = {0, 0, 0}, off_ip = 0, off_sums = 0, off_z = 0, pinned_bytes = 0;
  unsigned nb_walk = 0;
};
// one opening under way, as its stages see it; everything they queue goes to `st`
struct Run {
  sp_ctx* c;
  hipStream_t st;
  const Shape& s;
  const Plan& P;
  const Inputs& in;
  Item* items;
  char* pinned() const { return static_cast<char*>(c->h_opening); }
};
// what only the closing stages need: the transcripts, the points, the evaluations' commitments and blinds, the proofs
struct Job {
  const Run& R;
  const sp_ck* ck_eval;
  sp_transcript* const* tr;
  const uint64_t* comm_eval;
  const uint64_t* blind_eval;
  uint64_t* out;
};
inline size_t out_words(const Shape& s) { return 16 + 4 * s.cols + 8; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// sizes for both halves of the walk and `slots` params slots; grows the workspaces and the pinned buffer, makes the context's event
int make_plan(sp_ctx* c, const Shape& s, int slots, Plan* plan) {
  Plan P;
  const size_t nsc = s.num_cols + 1, nvec = 2 * s.count;
  P.nb_ip = (s.cols + spk::OB_STREAM_THREADS - 1) / spk::OB_STREAM_THREADS;
  P.nb_walk = (unsigned)((nsc * 32 + spk::OB_WALK_ITEMS - 1) / spk::OB_WALK_ITEMS);
  P.blocks_bytes = s.count * s.cols * 64;
  P.vec_bytes = s.count * s.cols * sizeof(fe_t);
  P.inst_bytes = align256(s.count * sizeof(spk::ObInst));
  P.params_bytes = align256(P.inst_bytes + s.count * (s.npt ? s.npt : 1) * sizeof(fe_t));
  P.ip_bytes = align256(s.count * P.nb_ip * sizeof(fe_t));
  P.sums_bytes = align256(nvec * sizeof(jac_t));
  P.tick_bytes = align256(nvec * sizeof(unsigned));
  const size_t part_bytes = nvec * (size_t)spk::OB_WALK_MAX_BLOCKS * sizeof(xyzz_t);
  P.d_blocks = (char*)c->workspace(sp_ctx::WS_OPENING_BLOCKS, P.blocks_bytes);
  fe_t* d_vecs = (fe_t*)c->workspace(sp_ctx::WS_OPENING_VECS, 3 * P.vec_bytes);
  P.d_params = (char*)c->workspace(sp_ctx::WS_OPENING_PARAMS, P.params_bytes);
  char* d_walk = (char*)c->workspace(sp_ctx::WS_OPENING_WALK, P.tick_bytes + part_bytes + P.sums_bytes + P.ip_bytes);
  if (!P.d_blocks || !d_vecs || !P.d_params || !d_walk) return SP_ERR_NO_DEVICE;
  P.d_d = d_vecs, P.d_lz = d_vecs + s.count * s.cols, P.d_z = d_vecs + 2 * s.count * s.cols;
  P.d_ticket = reinterpret_cast<unsigned*>(d_walk);
  P.d_part = reinterpret_cast<xyzz_t*>(d_walk + P.tick_bytes);
  P.d_sums = reinterpret_cast<jac_t*>(d_walk + P.tick_bytes + part_bytes);
  P.d_ip = reinterpret_cast<fe_t*>(d_walk + P.tick_bytes + part_bytes + P.sums_bytes);
  for (int i = 0; i < slots; ++i) P.off_params[i] = align256(P.blocks_bytes) + i * P.params_bytes;
  P.off_ip = P.off_params[slots - 1] + P.params_bytes;
  P.off_sums = P.off_ip + P.ip_bytes;
  P.off_z = P.off_sums + P.sums_bytes;
  P.pinned_bytes = P.off_z + P.vec_bytes;
  const int rc = sp::opening_pinned_reserve(c, P.pinned_bytes);
  if (rc) return rc;
  if (!c->opening_ev) SP_HIP(hipEventCreateWithFlags(&c->opening_ev, hipEventDisableTiming));
  *plan = P;
  return SP_OK;
}

template <class F>
void for_instances(size_t count, F f) {  // f(k) for every instance, the instances dealt over the polling host threads
  struct Ctx {
    size_t count;
    F* f;
  } cx{count, &f};
  sp_host_parallel_for((unsigned)(count < 32 ? count : 32), [](void* a, unsigned part, unsigned np) {
    Ctx& c = *static_cast<Ctx*>(a);
    for (size_t k = part; k < c.count; k += np) (*c.f)(k);
  }, &cx);
}

// E::Scalar::random draws behind the mask vector (ipa.rs:146-149): the blinds of delta and beta
void draw_blinds(const Shape& s, const Inputs& in, Item* items) {
  for (size_t k = 0; k < s.count; ++k) {
    items[k].r_delta = fe_from_uniform<SF>(in.rng[k] + 64 * s.cols);
    items[k].r_beta = fe_from_uniform<SF>(in.rng[k] + 64 * (s.cols + 1));
  }
}
// r_LZ = <L, blinds> with L = eq(row point) (hyrax_pc.rs:446-455), h's scalar in comm_LZ's walk - 2 rows products an instance; a single row's
// commitment is the row itself and r_LZ its blind (:417-423). pts: instance k's row challenges at element pts_stride * k
void stage_r_lz(const Run& R, const uint64_t* pts, size_t pts_stride, size_t k) {
  const Shape& s = R.s;
  const fe_t* blind = R.in.blinds[k];
  fe_t r_lz = blind[0];
  if (s.nvr) {
    std::vector<fe_t> L(s.rows);
    sp::eq_evals_host(reinterpret_cast<const fe_t*>(pts) + k * pts_stride, s.nvr, L.data());
    r_lz = fe_zero();
    for (size_t i = 0; i < s.rows; ++i) r_lz = fe_add<SF>(r_lz, fe_mul<SF>(L[i], blind[i]));
  }
  R.items[k].r_LZ = r_lz;
}
// while the device works: transcript.absorb(b"poly_com", comm) (hyrax_pc.rs:410) into a copy of the running hasher
void stage_hash(const Job& J, size_t k) {
  Item& it = J.R.items[k];
  it.hashed = J.tr[k]->t.h;
  sp::absorb_commitment(it.hashed, J.R.in.comm[k], J.R.s.rows);
}
// behind the copy of the block sums: beta = ck_c <R, d> + h_c r_beta (ipa.rs:148-149), two walks over the host tables
void stage_beta(const Job& J, size_t k) {
  Item& it = J.R.items[k];
  const size_t nb_ip = J.R.P.nb_ip;
  const fe_t* ip_part = reinterpret_cast<const fe_t*>(J.R.pinned() + J.R.P.off_ip) + k * nb_ip;
  fe_t ip = fe_zero();
  for (size_t b = 0; b < nb_ip; ++b) ip = fe_add<SF>(ip, ip_part[b]);
  it.ip = ip;
  const jac_t c = sp::ck_table_mul_host(J.ck_eval, 0, ip), h = sp::ck_table_mul_host(J.ck_eval, J.ck_eval->n_tables - 1, it.r_beta);
  it.beta = jac_to_affine(jac_add(c, h));
}
// behind the walks: InnerProductArgumentLinear::prove's transcript part (ipa.rs:132-158) and the two scalars of its answer (:164-168)
void stage_ipa(const Job& J, size_t k) {
  const Shape& s = J.R.s;
  Item& it = J.R.items[k];
  const jac_t* sums = reinterpret_cast<const jac_t*>(J.R.pinned() + J.R.P.off_sums);
  const aff_t delta = jac_to_affine(sums[k]);
  const aff_t comm_LZ = s.nvr == 0 ? J.R.in.comm[k][0] : jac_to_affine(sums[s.count + k]);
  aff_t comm_eval;
  memcpy(&comm_eval, J.comm_eval + 8 * k, sizeof(aff_t));
  sp::Transcript& t = J.tr[k]->t;
  t.h = it.hashed;
  if (!sp::ipa_transcript(t, comm_LZ, comm_eval, delta, it.beta, &it.r)) {
    it.rc = SP_ERR_INTERNAL_TRANSCRIPT;
    return;
  }
  uint64_t* o = J.out + k * out_words(s);
  memcpy(o, &delta, sizeof(aff_t));
  memcpy(o + 8, &it.beta, sizeof(aff_t));
  fe_t b_eval;
  memcpy(&b_eval, J.blind_eval + 4 * k, 32);
  fe_t* zv = reinterpret_cast<fe_t*>(o + 16);
  zv[s.cols] = fe_add<SF>(fe_mul<SF>(it.r, it.r_LZ), it.r_delta);   // z_delta = r r_LZ + r_delta
  zv[s.cols + 1] = fe_add<SF>(fe_mul<SF>(it.r, b_eval), it.r_beta);  // z_beta = r blind_eval + r_beta
}

// the mask vectors' uniform blocks through the pinned buffer to the device
int upload_blocks(const Run& R) {
  const size_t row = R.s.cols * 64;
  for (size_t k = 0; k < R.s.count; ++k) memcpy(R.pinned() + k * row, R.in.rng[k], row);
  SP_HIP(hipMemcpyAsync(R.P.d_blocks, R.pinned(), R.P.blocks_bytes, hipMemcpyHostToDevice, R.st));
  return SP_OK;
}
// the instance records and the first pts_take elements of every point (instance k's at element pts_stride * k) into pinned slot `slot`, then to the device
int upload_params(const Run& R, int slot, const uint64_t* pts, size_t pts_stride, size_t pts_take) {
  const Shape& s = R.s;
  const Plan& P = R.P;
  char* hp = R.pinned() + P.off_params[slot];
  memset(hp, 0, P.params_bytes);
  spk::ObInst* hi = reinterpret_cast<spk::ObInst*>(hp);
  fe_t* hpts = reinterpret_cast<fe_t*>(hp + P.inst_bytes);
  const fe_t* d_points = reinterpret_cast<const fe_t*>(P.d_params + P.inst_bytes);
  for (size_t k = 0; k < s.count; ++k) {
    hi[k].blocks = reinterpret_cast<const uint8_t*>(P.d_blocks + k * s.cols * 64);
    hi[k].poly = R.in.poly_d[k];
    hi[k].lz = s.nvr ? P.d_lz + k * s.cols : R.in.poly_d[k];
    hi[k].point = d_points + k * s.npt;
    hi[k].r_delta = R.items[k].r_delta;
    hi[k].r_lz = R.items[k].r_LZ;
    if (pts_take) memcpy(hpts + k * s.npt, pts + 4 * pts_stride * k, pts_take * sizeof(fe_t));
  }
  SP_HIP(hipMemcpyAsync(P.d_params, hp, P.params_bytes, hipMemcpyHostToDevice, R.st));
  return SP_OK;
}
inline const spk::ObInst* d_inst(const Run& R) { return reinterpret_cast<const spk::ObInst*>(R.P.d_params); }
inline dim3 stream_grid(const Run& R) { return dim3((unsigned)R.P.nb_ip, (unsigned)R.s.count); }  // k_ob_mask / _dvec / _ip / _z: one element a thread

// LZ = L^T W for every polynomial
void launch_rowmat(const Run& R) {
  const Shape& s = R.s;
  R.c->timed_on(R.st, "opening_batch_rowmat", 32ull * s.count * (s.rows * s.cols + s.cols), [&] {
    hipLaunchKernelGGL(spk::k_ob_rowmat, dim3((unsigned)((s.cols + spk::OB_RMV_COLS - 1) / spk::OB_RMV_COLS), (unsigned)s.count), dim3(spk::OB_RMV_THREADS), 0, R.st, d_inst(R),
                       (unsigned)s.rows, (unsigned)s.cols, (int)s.nvr, R.P.d_lz);
  });
}
// the walk of vectors vbase .. vbase + nvec - 1 (the deltas from 0, the comm_LZ from count) over the key's window tables
void launch_walk(const Run& R, const sp_ck* ck, size_t vbase, size_t nvec) {
  const size_t nsc = R.s.num_cols + 1;
  R.c->timed_on(R.st, "opening_batch_walk", 32ull * nvec * nsc, [&] {
    hipLaunchKernelGGL(spk::k_ob_walk, dim3(R.P.nb_walk, (unsigned)nvec), dim3(512), 0, R.st, d_inst(R), (unsigned)R.s.count, (unsigned)vbase, nsc, R.s.cols,
                       (const aff_t*)ck->d_keytables, R.P.d_part, R.P.d_ticket, R.P.d_sums);
  });
}
// the tail: every instance's challenge, z_vec = r LZ + d for all of them in one launch, and its words into the proofs
int finish_z(const Run& R, uint64_t* out) {
  const Shape& s = R.s;
  const Plan& P = R.P;
  spk::ObChallenges ch;
  memset(&ch, 0, sizeof ch);
  for (size_t k = 0; k < s.count; ++k) {
    if (R.items[k].rc) return fail(R.items[k].rc, "transcript round counter overflow");
    ch.r[k] = R.items[k].r;
  }
  R.c->timed_on(R.st, "opening_batch_z", 96ull * s.count * s.cols, [&] {
    hipLaunchKernelGGL(spk::k_ob_z, stream_grid(R), dim3(spk::OB_STREAM_THREADS), 0, R.st, d_inst(R), ch, (unsigned)s.cols, (const fe_t*)P.d_d, P.d_z);
  });
  SP_HIP(hipMemcpyAsync(R.pinned() + P.off_z, P.d_z, P.vec_bytes, hipMemcpyDeviceToHost, R.st));
  SP_HIP(sp::stream_sync(R.st));
  for (size_t k = 0; k < s.count; ++k) memcpy(out + k * out_words(s) + 16, R.pinned() + P.off_z + k * s.cols * sizeof(fe_t), s.cols * sizeof(fe_t));
  return SP_OK;
}

// every copy an opening made of mask material - the uniform blocks, d, the instances' blinds, <R, d> - on every exit path: the device buffers and the
// pinned buffer of a plan that was made, and the Items. (A job opened ahead wipes its own copies of the inputs beside this.)
// Deliberately NOT wiped: z = r LZ + d, which is the proof's z_vec, and LZ = L^T W in WS_OPENING_VECS, which is no mask material and which
// sp_hyrax_prove leaves behind in WS_ROWMAT_OUT the same way.
void wipe(const Run& R, bool tickets) {
  const Plan& P = R.P;
  if (P.d_blocks) {
    (void)hipMemsetAsync(P.d_blocks, 0, P.blocks_bytes, R.st);
    (void)hipMemsetAsync(P.d_d, 0, P.vec_bytes, R.st);
    (void)hipMemsetAsync(P.d_params, 0, P.params_bytes, R.st);
    (void)hipMemsetAsync(P.d_ip, 0, P.ip_bytes, R.st);
    if (tickets) (void)hipMemsetAsync(P.d_ticket, 0, P.tick_bytes, R.st);  // (a walk that was never joined leaves no count behind)
    (void)sp::stream_sync(R.st);  // (also: nothing of this opening still reads the pinned buffer)
    if (R.c->h_opening && R.c->h_opening_bytes >= P.pinned_bytes) explicit_bzero(R.c->h_opening, P.pinned_bytes);
  }
  explicit_bzero(R.items, R.s.count * sizeof(Item));
}

// the refusals of sp_hyrax_prove_batch: nothing is launched, absorbed or written before the last of them. full = 0: those that concern the arguments
// sp_hyrax_prove_batch_begin is given (no transcripts, points, eval commitments or output; npt is the logarithm of n)
int check_args(const char* who, sp_ctx* c, const sp_ck* ck, const sp_ck* ck_eval, size_t count, bool full, sp_transcript* const* tr, const uint64_t* const* comm_rows_aff,
               size_t rows, const sp_table* const* poly, size_t n, const uint64_t* const* blinds, const uint64_t* points, size_t npt, const uint64_t* comm_eval_aff,
               const uint64_t* blind_eval, const uint8_t* const* rng, const size_t* rng_blocks, const uint64_t* out, Shape* shape) {
  const std::string w(who);
  if (count == 0 || count > SP_LOCKSTEP_MAX) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": count must be 1 .. SP_LOCKSTEP_MAX");
  if (!c || !ck || !ck_eval || !comm_rows_aff || !poly || !blinds || !rng || !rng_blocks || (full && (!tr || (!points && npt) || !comm_eval_aff || !blind_eval || !out)))
    return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null argument");
  if (c->opening_job) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": a batch opened ahead is pending on this context (sp_hyrax_prove_batch_finish or _drop first)");
  for (size_t k = 0; k < count; ++k) {
    const char* what = (full && !tr[k]) ? "transcript" : !comm_rows_aff[k] ? "commitment" : (!poly[k] || !poly[k]->d) ? "table" : !blinds[k] ? "blinds" : !rng[k] ? "randomness stream" : nullptr;
    if (what) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null " + what + ", instance " + std::to_string(k));
  }
  if (!full)
    for (npt = 0; npt < 40 && ((size_t)1 << npt) < n; ++npt) {}
  if (npt > 40 || n != ((size_t)1 << npt)) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": Expected 2^point.len() elements in poly");  // hyrax_pc.rs:400-408
  for (size_t k = 0; k < count; ++k)
    if (n > poly[k]->cap) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": Expected 2^point.len() elements in poly, instance " + std::to_string(k));
  const size_t num_cols = ck->num_cols, num_rows = (n + num_cols - 1) / num_cols;
  if (num_rows & (num_rows - 1)) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": the row count must be a power of two");
  if (rows != num_rows) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": one commitment row and one blind per matrix row");
  size_t nvr = 0;
  while (((size_t)1 << nvr) < num_rows) ++nvr;
  const size_t cols = n / num_rows;  // |R| = |LZ| = |d|
  for (size_t k = 0; k < count; ++k)
    if (rng_blocks[k] < cols + 2)
      return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": the randomness stream holds fewer than cols + 2 blocks, instance " + std::to_string(k));
  if (full)
    for (size_t k = 0; k < count; ++k)
      for (size_t j = 0; j < k; ++j)
        if (tr[j] == tr[k]) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": the same transcript twice, instances " + std::to_string(j) + " and " + std::to_string(k));
  if (!ck_eval->d_cktables || ck_eval->num_cols < 1) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": ck_eval must be a narrow key with tables");
  *shape = Shape{count, rows, n, npt, nvr, cols, num_cols};
  return SP_OK;
}
// the batched stages walk the window tables of a key of 1023 .. 4095 columns (k_ob_walk is k_multi_mul_wide's shape) and keep the row weights in LDS
bool batched_shape(const Shape& s) {
  const size_t nsc = s.num_cols + 1;
  return nsc >= sp::multi_mul_wide_min() && nsc * 32 <= (size_t)spk::OB_WALK_MAX_BLOCKS * spk::OB_WALK_ITEMS && s.cols <= s.num_cols && s.nvr <= (size_t)spk::OB_ROW_BITS_MAX;
}
}  // namespace

extern "C" int sp_hyrax_prove_batch(sp_ctx* c, const sp_ck* ck, const sp_ck* ck_eval, size_t count, sp_transcript* const* tr, const uint64_t* const* comm_rows_aff,
                                    size_t rows, const sp_table* const* poly, size_t n, const uint64_t* const* blinds, const uint64_t* points, size_t npt,
                                    const uint64_t* comm_eval_aff, const uint64_t* blind_eval, const uint8_t* const* rng, const size_t* rng_blocks, uint64_t* out) {
  Shape sh;
  int rc = check_args(WHO, c, ck, ck_eval, count, true, tr, comm_rows_aff, rows, poly, n, blinds, points, npt, comm_eval_aff, blind_eval, rng, rng_blocks, out, &sh);
  if (rc) return rc;
  const size_t nvr = sh.nvr, cols = sh.cols;

  SP_HIP(hipSetDevice(c->device));
  rc = sp_hyrax_prove_retract(c);  // an announced opening is not this call's: withdrawn, never consumed
  if (rc) return rc;
  auto per_instance = [&]() -> int {
    for (size_t k = 0; k < count; ++k) {
      const int r = sp_hyrax_prove(c, ck, ck_eval, tr[k], comm_rows_aff[k], rows, poly[k], n, blinds[k], points + 4 * npt * k, npt, comm_eval_aff + 8 * k, blind_eval + 4 * k,
                                   rng[k], rng_blocks[k], out + k * out_words(sh));
      if (r) return r;
    }
    return SP_OK;
  };
  if (count == 1 || !batched_shape(sh)) return per_instance();
  const int kt = sp::ck_key_tables(c, ck);
  if (kt < 0) return kt;
  if (kt != 0) return per_instance();

  Plan P;
  if ((rc = make_plan(c, sh, 1, &P))) return rc;
  for (size_t k = 0; k < count; ++k) tr[k]->join();
  // The per-instance host stages below are spread over the polling threads, which only claim parts while they are awake: woken here, ahead of the
  // uploads (a wake-up is 5-50 us, the first one starts the threads), for the length of the call - profiles/prove_batch.md: ~0.13 ms an instance at
  // K = 16, ~0.17 at K = 4 - and again before each stage, which costs two loads while they are awake.
  const uint64_t hot_us = 400 + 150 * count;
  (void)sp_walkers_keep_hot(hot_us);

  Inputs in;
  for (size_t k = 0; k < count; ++k) {
    in.comm[k] = reinterpret_cast<const aff_t*>(comm_rows_aff[k]);
    in.blinds[k] = reinterpret_cast<const fe_t*>(blinds[k]);
    in.rng[k] = rng[k];
    in.poly_d[k] = poly[k]->d;
  }
  std::vector<Item> items(count);
  const Run R{c, c->stream, sh, P, in, items.data()};
  const Job J{R, ck_eval, tr, comm_eval_aff, blind_eval, out};
  struct Wipe {
    const Run& R;
    ~Wipe() { wipe(R, false); }
  } wipe_on_exit{R};

  // ---- uploads: the mask vectors' blocks, the instances, the points
  draw_blinds(sh, in, items.data());
  for_instances(count, [&](size_t k) { stage_r_lz(R, points, npt, k); });
  if ((rc = upload_blocks(R)) || (rc = upload_params(R, 0, points, npt, npt))) return rc;
  SP_HIP(hipMemsetAsync(P.d_ticket, 0, P.tick_bytes, c->stream));
  // ---- stage: the mask vectors and the block sums of <R, d>
  c->timed("opening_batch_mask", 96ull * count * cols, [&] {
    hipLaunchKernelGGL(spk::k_ob_mask, stream_grid(R), dim3(spk::OB_STREAM_THREADS), 0, c->stream, d_inst(R), (unsigned)cols, (int)nvr, (int)(npt - nvr), P.d_d, P.d_ip);
  });
  SP_HIP(hipMemcpyAsync(R.pinned() + P.off_ip, P.d_ip, count * P.nb_ip * sizeof(fe_t), hipMemcpyDeviceToHost, c->stream));
  SP_HIP(hipEventRecord(c->opening_ev, c->stream));
  // ---- stage: LZ = L^T W for every polynomial, then the walks of every delta and comm_LZ
  const size_t nvec = nvr ? 2 * count : count;
  if (nvr) launch_rowmat(R);
  launch_walk(R, ck, 0, nvec);
  SP_HIP(hipMemcpyAsync(R.pinned() + P.off_sums, P.d_sums, nvec * sizeof(jac_t), hipMemcpyDeviceToHost, c->stream));
  // host beside the device: the commitments' hashing, then - the block sums of <R, d> have landed - beta
  (void)sp_walkers_keep_hot(hot_us);
  for_instances(count, [&](size_t k) { stage_hash(J, k); });
  SP_HIP(sp::event_sync(c->opening_ev));
  for_instances(count, [&](size_t k) { stage_beta(J, k); });
  SP_HIP(sp::stream_sync(c->stream));
  // ---- the IPA's transcript part per instance, then z_vec = r LZ + d for all of them
  (void)sp_walkers_keep_hot(200);
  for_instances(count, [&](size_t k) { stage_ipa(J, k); });
  return finish_z(R, out);
}

// ---- the same opening, begun ahead of its point -------------------------------------------------------------------------------------------------
// What _begin was given, by value where _finish compares by value (the caller's buffers may be rewritten in between), and the state of its stages.
struct sp_opening_job {
  Shape sh{};
  const sp_ck *ck = nullptr, *ck_eval = nullptr;
  bool started = false;    // false: a shape sp_hyrax_prove_batch opens instance by instance - nothing is queued, _finish runs that loop
  bool rows_done = false;  // the row stage is queued (or the polynomial has one row: there is none)
  bool hash_posted = false;
  bool failed = false;     // a stage could not be queued: _finish computes everything as sp_hyrax_prove_batch does
  std::vector<const uint64_t*> comm_ptr;
  std::vector<const sp_table*> poly;
  std::vector<aff_t> comm;        // count x rows
  std::vector<fe_t> blinds;       // count x rows
  std::vector<uint8_t> rng;       // count x (cols + 2) blocks
  std::vector<fe_t> row_pts;      // count x nvr, as _rows saw them
  Inputs in;                      // the copies above, and poly->d as _begin saw it
  std::vector<Item> items;        // hashed: "poly_com" || commitment bytes in a FRESH sponge
  Plan P;                         // one params slot per stage
  Run run(sp_ctx* c) { return Run{c, c->stream2, sh, P, in, items.data()}; }
};

namespace {
template <class T>
void wipe_vec(std::vector<T>& v) {
  if (!v.empty()) explicit_bzero(v.data(), v.size() * sizeof(T));
}
// r_LZ per instance on the host, then k_ob_rowmat and the walk of the comm_LZ vectors behind the delta walk
int queue_rows(sp_ctx* c, sp_opening_job* j, const uint64_t* pts, size_t pts_stride) {
  const Shape& s = j->sh;
  const Run R = j->run(c);
  j->row_pts.resize(s.count * s.nvr);
  for (size_t k = 0; k < s.count; ++k) memcpy(&j->row_pts[k * s.nvr], pts + 4 * pts_stride * k, s.nvr * sizeof(fe_t));
  (void)sp_walkers_keep_hot(100);
  for_instances(s.count, [&](size_t k) { stage_r_lz(R, pts, pts_stride, k); });
  j->rows_done = true;  // (set before the launches: a failure below leaves `failed`, which is all _finish looks at then)
  j->failed = true;
  int rc = upload_params(R, 1, pts, pts_stride, s.nvr);
  if (rc) return rc;
  launch_rowmat(R);
  launch_walk(R, j->ck, s.count, s.count);
  SP_HIP(hipMemcpyAsync(R.pinned() + j->P.off_sums + s.count * sizeof(jac_t), j->P.d_sums + s.count, s.count * sizeof(jac_t), hipMemcpyDeviceToHost, c->stream2));
  j->failed = false;
  return SP_OK;
}
}  // namespace

namespace sp {
// waits for what the job queued, wipes every copy of the mask vectors, the randomness blocks and the blinds - pinned, device and the job's own - and
// frees the job (`wipe` above, with the tickets; z and LZ are no mask material)
void opening_job_free(sp_ctx* c) {
  if (!c || !c->opening_job) return;
  sp_opening_job* j = c->opening_job;
  c->opening_job = nullptr;
  if (j->hash_posted && c->pcs_worker) c->pcs_worker->wait();
  wipe(j->run(c), true);
  wipe_vec(j->blinds);
  wipe_vec(j->rng);
  delete j;
}
}  // namespace sp

extern "C" int sp_hyrax_prove_batch_begin(sp_ctx* c, const sp_ck* ck, const sp_ck* ck_eval, size_t count, const uint64_t* const* comm_rows_aff, size_t rows,
                                          const sp_table* const* poly, size_t n, const uint64_t* const* blinds, const uint8_t* const* rng, const size_t* rng_blocks,
                                          sp_opening_job** job) {
  static const char* who = "sp_hyrax_prove_batch_begin";
  if (!job) return fail(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": null argument");
  Shape sh;
  int rc = check_args(who, c, ck, ck_eval, count, false, nullptr, comm_rows_aff, rows, poly, n, blinds, nullptr, 0, nullptr, nullptr, rng, rng_blocks, nullptr, &sh);
  if (rc) return rc;
  SP_HIP(hipSetDevice(c->device));
  rc = sp_hyrax_prove_retract(c);  // an announced opening is not this batch's: withdrawn, never consumed
  if (rc) return rc;
  const size_t cols = sh.cols, nvr = sh.nvr;
  bool started = count > 1 && batched_shape(sh);
  if (started) {
    const int kt = sp::ck_key_tables(c, ck);
    if (kt < 0) return kt;
    started = kt == 0;
  }
  std::unique_ptr<sp_opening_job> owner(new sp_opening_job);
  sp_opening_job* j = owner.get();
  j->sh = sh;
  j->ck = ck;
  j->ck_eval = ck_eval;
  j->comm_ptr.assign(comm_rows_aff, comm_rows_aff + count);
  j->poly.assign(poly, poly + count);
  j->comm.resize(count * rows);
  j->blinds.resize(count * rows);
  j->rng.resize(count * 64 * (cols + 2));
  j->items.resize(count);
  for (size_t k = 0; k < count; ++k) {
    memcpy(&j->comm[k * rows], comm_rows_aff[k], rows * sizeof(aff_t));
    memcpy(&j->blinds[k * rows], blinds[k], rows * sizeof(fe_t));
    memcpy(&j->rng[k * 64 * (cols + 2)], rng[k], 64 * (cols + 2));
    j->in.comm[k] = &j->comm[k * rows];
    j->in.blinds[k] = &j->blinds[k * rows];
    j->in.rng[k] = &j->rng[k * 64 * (cols + 2)];
    j->in.poly_d[k] = poly[k]->d;
  }
  const Run R = j->run(c);  // (refers to the job's plan: made below)
  draw_blinds(sh, j->in, j->items.data());
  j->rows_done = nvr == 0;
  if (!nvr)
    for (size_t k = 0; k < count; ++k) stage_r_lz(R, nullptr, 0, k);
  if (!started) {
    c->opening_job = owner.release();
    *job = j;
    return SP_OK;
  }
  if ((rc = make_plan(c, sh, 3, &j->P))) return rc;
  if (!c->pcs_worker) c->pcs_worker = new sp::Worker();
  j->started = true;
  c->opening_job = owner.release();  // from here on every exit leaves the job to _finish / _drop, which wait and wipe
  *job = nullptr;
  auto queue = [&]() -> int {
    // ---- the auxiliary stream takes over behind what the main stream holds now (the tables' and the workspaces' last writers)
    SP_HIP(hipEventRecord(c->opening_ev, c->stream));
    SP_HIP(hipStreamWaitEvent(c->stream2, c->opening_ev, 0));
    if ((rc = upload_blocks(R)) || (rc = upload_params(R, 0, nullptr, 0, 0))) return rc;
    SP_HIP(hipMemsetAsync(j->P.d_ticket, 0, j->P.tick_bytes, c->stream2));
    c->timed_on(c->stream2, "opening_batch_dvec", 96ull * count * cols, [&] {
      hipLaunchKernelGGL(spk::k_ob_dvec, stream_grid(R), dim3(spk::OB_STREAM_THREADS), 0, c->stream2, d_inst(R), (unsigned)cols, j->P.d_d);
    });
    launch_walk(R, ck, 0, count);
    SP_HIP(hipMemcpyAsync(R.pinned() + j->P.off_sums, j->P.d_sums, count * sizeof(jac_t), hipMemcpyDeviceToHost, c->stream2));
    return SP_OK;
  };
  if ((rc = queue())) {  // nothing of a job that could not be queued stays behind
    sp::opening_job_free(c);
    return rc;
  }
  *job = j;
  // ---- the helper thread: transcript.absorb(b"poly_com", comm) (hyrax_pc.rs:410) of every instance into a fresh sponge
  j->hash_posted = true;
  c->pcs_worker->keep_hot(200);
  c->pcs_worker->submit([j] {
    for (size_t k = 0; k < j->sh.count; ++k) {
      j->items[k].hashed.init();
      sp::absorb_commitment(j->items[k].hashed, j->in.comm[k], j->sh.rows);
    }
  });
  return SP_OK;
}

extern "C" int sp_hyrax_prove_batch_rows(sp_ctx* c, sp_opening_job* job, const uint64_t* row_points) {
  if (!c || !job || c->opening_job != job) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_hyrax_prove_batch_rows: not this context's open job");
  if (!job->started || job->sh.nvr == 0 || job->rows_done || job->failed) return SP_OK;  // no row stage, or it is queued: nothing to do
  if (!row_points) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_hyrax_prove_batch_rows: null argument");
  SP_HIP(hipSetDevice(c->device));
  return queue_rows(c, job, row_points, job->sh.nvr);
}

extern "C" void sp_hyrax_prove_batch_drop(sp_ctx* c, sp_opening_job* job) {
  if (!c || !job || c->opening_job != job) return;
  (void)hipSetDevice(c->device);
  sp::opening_job_free(c);
}

extern "C" int sp_hyrax_prove_batch_finish(sp_ctx* c, sp_opening_job* job, const sp_ck* ck, const sp_ck* ck_eval, size_t count, sp_transcript* const* tr,
                                           const uint64_t* const* comm_rows_aff, size_t rows, const sp_table* const* poly, size_t n, const uint64_t* const* blinds,
                                           const uint64_t* points, size_t npt, const uint64_t* comm_eval_aff, const uint64_t* blind_eval, const uint8_t* const* rng,
                                           const size_t* rng_blocks, uint64_t* out) {
  if (!c) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_hyrax_prove_batch_finish: null argument");
  if (!job) return sp_hyrax_prove_batch(c, ck, ck_eval, count, tr, comm_rows_aff, rows, poly, n, blinds, points, npt, comm_eval_aff, blind_eval, rng, rng_blocks, out);
  if (c->opening_job != job) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_hyrax_prove_batch_finish: not this context's open job");
  (void)hipSetDevice(c->device);
  struct Done {  // the job ends with this call, whatever it returns
    sp_ctx* c;
    ~Done() { sp::opening_job_free(c); }
  } done{c};
  auto plain = [&]() -> int {  // drop what the job holds; compute as sp_hyrax_prove_batch does
    sp::opening_job_free(c);
    return sp_hyrax_prove_batch(c, ck, ck_eval, count, tr, comm_rows_aff, rows, poly, n, blinds, points, npt, comm_eval_aff, blind_eval, rng, rng_blocks, out);
  };
  if (!job->started || job->failed) return plain();
  sp_opening_job* j = job;
  c->opening_job = nullptr;  // (the refusals below are sp_hyrax_prove_batch's own; the open job is not one of them)
  Shape sh;
  int rc = check_args("sp_hyrax_prove_batch_finish", c, ck, ck_eval, count, true, tr, comm_rows_aff, rows, poly, n, blinds, points, npt, comm_eval_aff, blind_eval, rng, rng_blocks,
                      out, &sh);
  c->opening_job = j;
  if (rc) return rc;
  // ---- is this the opening that was begun? By value: the caller's buffers may have been rewritten since
  const Shape& s = j->sh;
  const Plan& P = j->P;
  const size_t cols = s.cols, nvr = s.nvr;
  bool same = j->ck == ck && j->ck_eval == ck_eval && s.count == count && s.rows == rows && s.n == n && s.npt == npt;
  for (size_t k = 0; same && k < count; ++k)
    same = j->poly[k] == poly[k] && j->in.poly_d[k] == poly[k]->d && j->comm_ptr[k] == comm_rows_aff[k] && memcmp(j->in.comm[k], comm_rows_aff[k], rows * sizeof(aff_t)) == 0 &&
           memcmp(j->in.blinds[k], blinds[k], rows * sizeof(fe_t)) == 0 && memcmp(j->in.rng[k], rng[k], 64 * (cols + 2)) == 0 &&
           (!nvr || !j->rows_done || memcmp(&j->row_pts[k * nvr], points + 4 * npt * k, nvr * sizeof(fe_t)) == 0);
  if (!same) return plain();
  rc = sp_hyrax_prove_retract(c);
  if (rc) return rc;
  for (size_t k = 0; k < count; ++k) tr[k]->join();
  (void)sp_walkers_keep_hot(300 + 50 * count);
  if (!j->rows_done && (rc = queue_rows(c, j, points, npt))) return rc;  // _rows was not called: its stage now, behind the delta walk
  // ---- the full points, then the block sums of <R, d>; their copy lands behind both walks' sums
  const Run R = j->run(c);
  const Job J{R, ck_eval, tr, comm_eval_aff, blind_eval, out};
  if ((rc = upload_params(R, 2, points, npt, npt))) return rc;
  c->timed_on(c->stream2, "opening_batch_ip", 64ull * count * cols, [&] {
    hipLaunchKernelGGL(spk::k_ob_ip, stream_grid(R), dim3(spk::OB_STREAM_THREADS), 0, c->stream2, d_inst(R), (unsigned)cols, (int)nvr, (int)(npt - nvr), (const fe_t*)P.d_d, P.d_ip);
  });
  SP_HIP(hipMemcpyAsync(R.pinned() + P.off_ip, P.d_ip, count * P.nb_ip * sizeof(fe_t), hipMemcpyDeviceToHost, c->stream2));
  // host beside the device: the sponges hashed ahead stay for the transcripts that have absorbed nothing since their last squeeze; the others are hashed now
  c->pcs_worker->wait();
  for_instances(count, [&](size_t k) {
    const sp::Keccak256State& h = tr[k]->t.h;
    bool fresh = h.fill == 0;
    for (int i = 0; i < 25 && fresh; ++i) fresh = h.a[i] == 0;
    if (!fresh) stage_hash(J, k);
  });
  SP_HIP(sp::stream_sync(c->stream2));
  // ---- beta, the IPA's transcript part per instance, then z_vec = r LZ + d for all of them
  (void)sp_walkers_keep_hot(300);
  for_instances(count, [&](size_t k) {
    stage_beta(J, k);
    stage_ipa(J, k);
  });
  return finish_z(R, out);
}
