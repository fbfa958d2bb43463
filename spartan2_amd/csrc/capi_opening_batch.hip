// sp_hyrax_prove_batch (include/spartan_hip.h): `count` instances of HyraxPCS::prove (hyrax_pc.rs:387-478) + InnerProductArgumentLinear::prove
// (ipa.rs:125-170) on one commitment key, opened in one pass. sp_hyrax_prove (capi_group.hip) is latency-shaped: two 65-block table walks, one L^T W,
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
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "group_common.hpp"
#include "kernels_opening_ahead.hpp"
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
struct Job {
  const Shape* sh;
  const sp_ck* ck_eval;
  sp_transcript* const* tr;
  const uint64_t* const* comm;
  const uint64_t* const* blinds;
  const uint64_t* points;
  const uint64_t* comm_eval;
  const uint64_t* blind_eval;
  uint64_t* out;
  Item* items;
  const fe_t* ip_part;  // count x nb_ip block sums of <R, d>
  size_t nb_ip;
  const jac_t* sums;    // delta_0 .. delta_(count-1), then comm_LZ_0 .. (two or more rows)
};
inline size_t out_words(const Shape& s) { return 16 + 4 * s.cols + 8; }

template <class F>
void for_instances(Job& J, F f) {  // f(J, k) for every instance, the instances dealt over the parts
  struct Ctx {
    Job* J;
    F* f;
  } cx{&J, &f};
  const unsigned parts = (unsigned)(J.sh->count < 32 ? J.sh->count : 32);
  sp_host_parallel_for(parts, [](void* a, unsigned part, unsigned np) {
    Ctx& c = *static_cast<Ctx*>(a);
    for (size_t k = part; k < c.J->sh->count; k += np) (*c.f)(*c.J, k);
  }, &cx);
}

// before the uploads: r_LZ = <L, blinds> with L = eq(row point) (hyrax_pc.rs:446-455), h's scalar in comm_LZ's walk - 2 rows products an instance; a
// single row's commitment is the row itself and r_LZ its blind (:417-423)
void stage_r_lz(Job& J, size_t k) {
  const Shape& s = *J.sh;
  const fe_t* blind = reinterpret_cast<const fe_t*>(J.blinds[k]);
  fe_t r_lz = blind[0];
  if (s.nvr) {
    std::vector<fe_t> L(s.rows);
    sp::eq_evals_host(reinterpret_cast<const fe_t*>(J.points) + k * s.npt, s.nvr, L.data());
    r_lz = fe_zero();
    for (size_t i = 0; i < s.rows; ++i) r_lz = fe_add<SF>(r_lz, fe_mul<SF>(L[i], blind[i]));
  }
  J.items[k].r_LZ = r_lz;
}
// while the device works: transcript.absorb(b"poly_com", comm) (hyrax_pc.rs:410) into a copy of the running hasher
void stage_hash(Job& J, size_t k) {
  const Shape& s = *J.sh;
  Item& it = J.items[k];
  const aff_t* comm = reinterpret_cast<const aff_t*>(J.comm[k]);
  static const char* b = "poly_commitment_begin";  // HyraxCommitment::to_transcript_bytes (hyrax_pc.rs:714-729)
  static const char* e = "poly_commitment_end";
  it.hashed = J.tr[k]->t.h;
  it.hashed.update(reinterpret_cast<const uint8_t*>("poly_com"), 8);
  it.hashed.update(reinterpret_cast<const uint8_t*>(b), strlen(b));
  uint8_t buf[64 * 16];
  for (size_t i = 0; i < s.rows; i += 16) {
    const size_t m = s.rows - i < 16 ? s.rows - i : 16;
    for (size_t q = 0; q < m; ++q) sp::point_transcript_bytes(comm[i + q], buf + 64 * q);
    it.hashed.update(buf, 64 * m);
  }
  it.hashed.update(reinterpret_cast<const uint8_t*>(e), strlen(e));
}
// behind the event: beta = ck_c <R, d> + h_c r_beta (ipa.rs:148-149), two walks over the host tables
void stage_beta(Job& J, size_t k) {
  Item& it = J.items[k];
  fe_t ip = fe_zero();
  for (size_t b = 0; b < J.nb_ip; ++b) ip = fe_add<SF>(ip, J.ip_part[k * J.nb_ip + b]);
  it.ip = ip;
  const jac_t c = sp::ck_table_mul_host(J.ck_eval, 0, ip), h = sp::ck_table_mul_host(J.ck_eval, J.ck_eval->n_tables - 1, it.r_beta);
  it.beta = jac_to_affine(jac_add(c, h));
}
// behind the walks: InnerProductArgumentLinear::prove's transcript part (ipa.rs:132-158) and the two scalars of its answer (:164-168)
void stage_ipa(Job& J, size_t k) {
  const Shape& s = *J.sh;
  Item& it = J.items[k];
  const aff_t delta = jac_to_affine(J.sums[k]);
  aff_t comm_LZ, comm_eval;
  if (s.nvr == 0) memcpy(&comm_LZ, J.comm[k], sizeof(aff_t));
  else comm_LZ = jac_to_affine(J.sums[s.count + k]);
  memcpy(&comm_eval, J.comm_eval + 8 * k, sizeof(aff_t));
  sp::Transcript& t = J.tr[k]->t;
  t.h = it.hashed;
  static const char* ds = "inner product argument (linear)";
  t.dom_sep(reinterpret_cast<const uint8_t*>(ds), strlen(ds));
  uint8_t b[128];
  sp::point_transcript_bytes(comm_LZ, b);
  sp::point_transcript_bytes(comm_eval, b + 64);
  t.absorb(reinterpret_cast<const uint8_t*>("U"), 1, b, 128);
  sp::point_transcript_bytes(delta, b);
  t.absorb(reinterpret_cast<const uint8_t*>("delta"), 5, b, 64);
  sp::point_transcript_bytes(it.beta, b);
  t.absorb(reinterpret_cast<const uint8_t*>("beta"), 4, b, 64);
  if (!t.squeeze<SF>(reinterpret_cast<const uint8_t*>("r"), 1, &it.r)) {
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

// every copy this call made of mask material - the uniform blocks, d, the instances' blinds, <R, d> - on every exit path.
// Deliberately NOT wiped: z = r LZ + d, which is the proof's z_vec, and LZ = L^T W in WS_OPENING_VECS, which is no mask material and which
// sp_hyrax_prove leaves behind in WS_ROWMAT_OUT the same way.
struct Wipe {
  sp_ctx* c;
  void *d_blocks = nullptr, *d_d = nullptr, *d_params = nullptr, *d_ip = nullptr;
  size_t blocks_bytes = 0, d_bytes = 0, params_bytes = 0, ip_bytes = 0, pinned_bytes = 0;
  std::vector<Item>* items = nullptr;
  ~Wipe() {
    if (d_blocks) (void)hipMemsetAsync(d_blocks, 0, blocks_bytes, c->stream);
    if (d_d) (void)hipMemsetAsync(d_d, 0, d_bytes, c->stream);
    if (d_params) (void)hipMemsetAsync(d_params, 0, params_bytes, c->stream);
    if (d_ip) (void)hipMemsetAsync(d_ip, 0, ip_bytes, c->stream);
    (void)sp::stream_sync(c->stream);  // (also: nothing of this call still reads the pinned buffer)
    if (pinned_bytes) explicit_bzero(c->h_opening, pinned_bytes);
    if (items && !items->empty()) explicit_bzero(items->data(), items->size() * sizeof(Item));
  }
};
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

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
  const size_t nvr = sh.nvr, cols = sh.cols, num_cols = sh.num_cols;

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
  const size_t nsc = num_cols + 1;
  if (count == 1 || !batched_shape(sh)) return per_instance();
  const int kt = sp::ck_key_tables(c, ck);
  if (kt < 0) return kt;
  if (kt != 0) return per_instance();

  // ---- buffers: device workspaces (grow-only) and one pinned buffer [blocks | params | ip block sums | walk sums | z]
  const size_t nb_ip = (cols + spk::OB_STREAM_THREADS - 1) / spk::OB_STREAM_THREADS, nvec = nvr ? 2 * count : count;
  const unsigned nb_walk = (unsigned)((nsc * 32 + spk::OB_WALK_ITEMS - 1) / spk::OB_WALK_ITEMS);
  const size_t blocks_bytes = count * cols * 64, vec_bytes = count * cols * sizeof(fe_t);
  const size_t params_bytes = align256(count * sizeof(spk::ObInst)) + count * (npt ? npt : 1) * sizeof(fe_t);
  const size_t ip_bytes = align256(count * nb_ip * sizeof(fe_t)), sums_bytes = align256(nvec * sizeof(jac_t));
  const size_t tick_bytes = align256(nvec * sizeof(unsigned)), part_bytes = nvec * (size_t)spk::OB_WALK_MAX_BLOCKS * sizeof(xyzz_t);
  char* d_blocks = (char*)c->workspace(sp_ctx::WS_OPENING_BLOCKS, blocks_bytes);
  fe_t* d_vecs = (fe_t*)c->workspace(sp_ctx::WS_OPENING_VECS, 3 * vec_bytes);
  char* d_params = (char*)c->workspace(sp_ctx::WS_OPENING_PARAMS, params_bytes);
  char* d_walk = (char*)c->workspace(sp_ctx::WS_OPENING_WALK, tick_bytes + part_bytes + sums_bytes + ip_bytes);
  if (!d_blocks || !d_vecs || !d_params || !d_walk) return SP_ERR_NO_DEVICE;
  fe_t *d_d = d_vecs, *d_lz = d_vecs + count * cols, *d_z = d_vecs + 2 * count * cols;
  unsigned* d_ticket = reinterpret_cast<unsigned*>(d_walk);
  xyzz_t* d_part = reinterpret_cast<xyzz_t*>(d_walk + tick_bytes);
  jac_t* d_sums = reinterpret_cast<jac_t*>(d_walk + tick_bytes + part_bytes);
  fe_t* d_ip = reinterpret_cast<fe_t*>(d_walk + tick_bytes + part_bytes + sums_bytes);
  const size_t off_params = align256(blocks_bytes), off_ip = off_params + align256(params_bytes), off_sums = off_ip + ip_bytes, off_z = off_sums + sums_bytes;
  const size_t pinned_bytes = off_z + vec_bytes;
  if (c->h_opening_bytes < pinned_bytes) {
    if (c->h_opening) hipHostFree(c->h_opening);
    c->h_opening = nullptr;
    c->h_opening_bytes = 0;
    SP_HIP(hipHostMalloc(&c->h_opening, pinned_bytes + pinned_bytes / 4));
    c->h_opening_bytes = pinned_bytes + pinned_bytes / 4;
  }
  if (!c->opening_ev) SP_HIP(hipEventCreateWithFlags(&c->opening_ev, hipEventDisableTiming));
  char* hp = static_cast<char*>(c->h_opening);
  for (size_t k = 0; k < count; ++k) tr[k]->join();
  // The per-instance host stages below are spread over the polling threads, which only claim parts while they are awake: woken here, ahead of the
  // uploads (a wake-up is 5-50 us, the first one starts the threads), for the length of the call - profiles/prove_batch.md: ~0.13 ms an instance at
  // K = 16, ~0.17 at K = 4 - and again before each stage, which costs two loads while they are awake.
  const uint64_t hot_us = 400 + 150 * count;
  (void)sp_walkers_keep_hot(hot_us);

  std::vector<Item> items(count);
  Wipe wipe{c};
  wipe.items = &items;
  wipe.pinned_bytes = pinned_bytes;
  wipe.d_blocks = d_blocks, wipe.blocks_bytes = blocks_bytes;
  wipe.d_d = d_d, wipe.d_bytes = vec_bytes;
  wipe.d_params = d_params, wipe.params_bytes = params_bytes;
  wipe.d_ip = d_ip, wipe.ip_bytes = ip_bytes;

  // ---- uploads: the mask vectors' blocks, the instances, the points
  const fe_t* d_points = reinterpret_cast<const fe_t*>(d_params + align256(count * sizeof(spk::ObInst)));
  Job J{&sh, ck_eval, tr, comm_rows_aff, blinds, points, comm_eval_aff, blind_eval, out, items.data(), reinterpret_cast<const fe_t*>(hp + off_ip), nb_ip,
        reinterpret_cast<const jac_t*>(hp + off_sums)};
  for_instances(J, stage_r_lz);
  {
    spk::ObInst* hi = reinterpret_cast<spk::ObInst*>(hp + off_params);
    for (size_t k = 0; k < count; ++k) {
      memcpy(hp + k * cols * 64, rng[k], cols * 64);
      hi[k].blocks = reinterpret_cast<const uint8_t*>(d_blocks + k * cols * 64);
      hi[k].poly = poly[k]->d;
      hi[k].lz = nvr ? d_lz + k * cols : poly[k]->d;
      hi[k].point = d_points + k * npt;
      // E::Scalar::random draws behind the mask vector (ipa.rs:146-149): the blinds of delta and beta
      items[k].r_delta = hi[k].r_delta = fe_from_uniform<SF>(rng[k] + 64 * cols);
      items[k].r_beta = fe_from_uniform<SF>(rng[k] + 64 * (cols + 1));
      hi[k].r_lz = items[k].r_LZ;
    }
    if (npt) memcpy(hp + off_params + align256(count * sizeof(spk::ObInst)), points, count * npt * sizeof(fe_t));
  }
  const spk::ObInst* d_inst = reinterpret_cast<const spk::ObInst*>(d_params);
  SP_HIP(hipMemcpyAsync(d_blocks, hp, blocks_bytes, hipMemcpyHostToDevice, c->stream));
  SP_HIP(hipMemcpyAsync(d_params, hp + off_params, params_bytes, hipMemcpyHostToDevice, c->stream));
  SP_HIP(hipMemsetAsync(d_ticket, 0, tick_bytes, c->stream));
  // ---- stage: the mask vectors and the block sums of <R, d>
  c->timed("opening_batch_mask", 96ull * count * cols, [&] {
    hipLaunchKernelGGL(spk::k_ob_mask, dim3((unsigned)nb_ip, (unsigned)count), dim3(spk::OB_STREAM_THREADS), 0, c->stream, d_inst, (unsigned)cols, (int)nvr, (int)(npt - nvr), d_d,
                       d_ip);
  });
  SP_HIP(hipMemcpyAsync(hp + off_ip, d_ip, count * nb_ip * sizeof(fe_t), hipMemcpyDeviceToHost, c->stream));
  SP_HIP(hipEventRecord(c->opening_ev, c->stream));
  // ---- stage: LZ = L^T W for every polynomial, then the walks of every delta and comm_LZ
  if (nvr)
    c->timed("opening_batch_rowmat", 32ull * count * (rows * cols + cols), [&] {
      hipLaunchKernelGGL(spk::k_ob_rowmat, dim3((unsigned)((cols + spk::OB_RMV_COLS - 1) / spk::OB_RMV_COLS), (unsigned)count), dim3(spk::OB_RMV_THREADS), 0, c->stream, d_inst,
                         (unsigned)rows, (unsigned)cols, (int)nvr, d_lz);
    });
  c->timed("opening_batch_walk", 32ull * nvec * nsc, [&] {
    hipLaunchKernelGGL(spk::k_ob_walk, dim3(nb_walk, (unsigned)nvec), dim3(512), 0, c->stream, d_inst, (unsigned)count, 0u, nsc, cols, (const aff_t*)ck->d_keytables, d_part, d_ticket,
                       d_sums);
  });
  SP_HIP(hipMemcpyAsync(hp + off_sums, d_sums, nvec * sizeof(jac_t), hipMemcpyDeviceToHost, c->stream));
  // host beside the device: the commitments' hashing, then - the block sums of <R, d> have landed - beta
  (void)sp_walkers_keep_hot(hot_us);
  for_instances(J, stage_hash);
  SP_HIP(sp::event_sync(c->opening_ev));
  for_instances(J, stage_beta);
  SP_HIP(sp::stream_sync(c->stream));
  // ---- the IPA's transcript part per instance, then z_vec = r LZ + d for all of them
  (void)sp_walkers_keep_hot(200);
  for_instances(J, stage_ipa);
  spk::ObChallenges ch;
  memset(&ch, 0, sizeof ch);
  for (size_t k = 0; k < count; ++k) {
    if (items[k].rc) return fail(items[k].rc, "transcript round counter overflow");
    ch.r[k] = items[k].r;
  }
  c->timed("opening_batch_z", 96ull * count * cols, [&] {
    hipLaunchKernelGGL(spk::k_ob_z, dim3((unsigned)nb_ip, (unsigned)count), dim3(spk::OB_STREAM_THREADS), 0, c->stream, d_inst, ch, (unsigned)cols, (const fe_t*)d_d, d_z);
  });
  SP_HIP(hipMemcpyAsync(hp + off_z, d_z, vec_bytes, hipMemcpyDeviceToHost, c->stream));
  SP_HIP(sp::stream_sync(c->stream));
  for (size_t k = 0; k < count; ++k) memcpy(out + k * out_words(sh) + 16, hp + off_z + k * cols * sizeof(fe_t), cols * sizeof(fe_t));
  return SP_OK;
}

// ---- the same opening, begun ahead of its point -------------------------------------------------------------------------------------------------
// What _begin was given, by value where _finish compares by value (the caller's buffers may be rewritten in between), and where each stage's data lives.
struct sp_opening_job {
  Shape sh{};
  const sp_ck *ck = nullptr, *ck_eval = nullptr;
  bool started = false;    // false: a shape sp_hyrax_prove_batch opens instance by instance - nothing is queued, _finish runs that loop
  bool rows_done = false;  // the row stage is queued (or the polynomial has one row: there is none)
  bool hash_posted = false;
  bool failed = false;     // a stage could not be queued: _finish computes everything as sp_hyrax_prove_batch does
  std::vector<const uint64_t*> comm_ptr;
  std::vector<const sp_table*> poly;
  std::vector<const fe_t*> poly_d;
  std::vector<aff_t> comm;        // count x rows
  std::vector<fe_t> blinds;       // count x rows
  std::vector<uint8_t> rng;       // count x (cols + 2) blocks
  std::vector<fe_t> row_pts;      // count x nvr, as _rows saw them
  std::vector<fe_t> r_delta, r_beta, r_LZ;
  std::vector<sp::Keccak256State> hashed;  // "poly_com" || commitment bytes in a fresh sponge, per instance
  // device: WS_OPENING_BLOCKS | WS_OPENING_VECS (d, LZ, z) | WS_OPENING_PARAMS (instances, points) | WS_OPENING_WALK (tickets, block sums, sums, ip block sums)
  char *d_blocks = nullptr, *d_params = nullptr;
  fe_t *d_d = nullptr, *d_lz = nullptr, *d_z = nullptr, *d_ip = nullptr;
  unsigned* d_ticket = nullptr;
  xyzz_t* d_part = nullptr;
  jac_t* d_sums = nullptr;
  // pinned: [blocks | params of _begin | of _rows | of _finish | ip block sums | walk sums | z] - a stage never rewrites what an earlier copy may still read
  size_t blocks_bytes = 0, vec_bytes = 0, params_bytes = 0, ip_bytes = 0, sums_bytes = 0, tick_bytes = 0, nb_ip = 0;
  size_t off_params[3] = {0, 0, 0}, off_ip = 0, off_sums = 0, off_z = 0, pinned_bytes = 0;
  unsigned nb_walk = 0;
};

namespace {
template <class F>
void par_instances(size_t count, F f) {  // f(k) for every instance, the instances dealt over the polling host threads
  struct Ctx {
    size_t count;
    F* f;
  } cx{count, &f};
  sp_host_parallel_for((unsigned)(count < 32 ? count : 32), [](void* a, unsigned part, unsigned np) {
    Ctx& c = *static_cast<Ctx*>(a);
    for (size_t k = part; k < c.count; k += np) (*c.f)(k);
  }, &cx);
}
template <class T>
void wipe_vec(std::vector<T>& v) {
  if (!v.empty()) explicit_bzero(v.data(), v.size() * sizeof(T));
}
// the instance records and the points of one stage into its pinned slot, then to the device behind whatever the auxiliary stream holds
int upload_params(sp_ctx* c, sp_opening_job* j, int slot, const uint64_t* pts, size_t pts_stride, size_t pts_take) {
  const Shape& s = j->sh;
  char* hp = static_cast<char*>(c->h_opening) + j->off_params[slot];
  memset(hp, 0, j->params_bytes);
  spk::ObInst* hi = reinterpret_cast<spk::ObInst*>(hp);
  fe_t* hpts = reinterpret_cast<fe_t*>(hp + align256(s.count * sizeof(spk::ObInst)));
  const fe_t* d_points = reinterpret_cast<const fe_t*>(j->d_params + align256(s.count * sizeof(spk::ObInst)));
  for (size_t k = 0; k < s.count; ++k) {
    hi[k].blocks = reinterpret_cast<const uint8_t*>(j->d_blocks + k * s.cols * 64);
    hi[k].poly = j->poly_d[k];
    hi[k].lz = s.nvr ? j->d_lz + k * s.cols : j->poly_d[k];
    hi[k].point = d_points + k * s.npt;
    hi[k].r_delta = j->r_delta[k];
    hi[k].r_lz = j->r_LZ[k];
    if (pts_take) memcpy(hpts + k * s.npt, pts + 4 * pts_stride * k, pts_take * sizeof(fe_t));
  }
  SP_HIP(hipMemcpyAsync(j->d_params, hp, j->params_bytes, hipMemcpyHostToDevice, c->stream2));
  return SP_OK;
}
// r_LZ_k = <eq(row point k), blinds_k> on the host (hyrax_pc.rs:446-455), then k_ob_rowmat and the walk of the comm_LZ vectors behind the delta walk
int queue_rows(sp_ctx* c, sp_opening_job* j, const uint64_t* pts, size_t pts_stride) {
  const Shape& s = j->sh;
  j->row_pts.resize(s.count * s.nvr);
  for (size_t k = 0; k < s.count; ++k) memcpy(&j->row_pts[k * s.nvr], pts + 4 * pts_stride * k, s.nvr * sizeof(fe_t));
  (void)sp_walkers_keep_hot(100);
  par_instances(s.count, [j, &s](size_t k) {
    std::vector<fe_t> L(s.rows);
    sp::eq_evals_host(&j->row_pts[k * s.nvr], s.nvr, L.data());
    fe_t r_lz = fe_zero();
    const fe_t* blind = &j->blinds[k * s.rows];
    for (size_t i = 0; i < s.rows; ++i) r_lz = fe_add<SF>(r_lz, fe_mul<SF>(L[i], blind[i]));
    j->r_LZ[k] = r_lz;
  });
  j->rows_done = true;  // (set before the launches: a failure below leaves `failed`, which is all _finish looks at then)
  j->failed = true;
  int rc = upload_params(c, j, 1, pts, pts_stride, s.nvr);
  if (rc) return rc;
  const spk::ObInst* d_inst = reinterpret_cast<const spk::ObInst*>(j->d_params);
  c->timed_on(c->stream2, "opening_batch_rowmat", 32ull * s.count * (s.rows * s.cols + s.cols), [&] {
    hipLaunchKernelGGL(spk::k_ob_rowmat, dim3((unsigned)((s.cols + spk::OB_RMV_COLS - 1) / spk::OB_RMV_COLS), (unsigned)s.count), dim3(spk::OB_RMV_THREADS), 0, c->stream2, d_inst,
                       (unsigned)s.rows, (unsigned)s.cols, (int)s.nvr, j->d_lz);
  });
  c->timed_on(c->stream2, "opening_batch_walk", 32ull * s.count * (s.num_cols + 1), [&] {
    hipLaunchKernelGGL(spk::k_ob_walk, dim3(j->nb_walk, (unsigned)s.count), dim3(512), 0, c->stream2, d_inst, (unsigned)s.count, (unsigned)s.count, s.num_cols + 1, s.cols,
                       (const aff_t*)j->ck->d_keytables, j->d_part, j->d_ticket, j->d_sums);
  });
  SP_HIP(hipMemcpyAsync(static_cast<char*>(c->h_opening) + j->off_sums + s.count * sizeof(jac_t), j->d_sums + s.count, s.count * sizeof(jac_t), hipMemcpyDeviceToHost, c->stream2));
  j->failed = false;
  return SP_OK;
}
}  // namespace

namespace sp {
// waits for what the job queued, wipes every copy of the mask vectors, the randomness blocks and the blinds - pinned, device and the job's own - and
// frees the job (the discipline of Wipe above; z and LZ are no mask material)
void opening_job_free(sp_ctx* c) {
  if (!c || !c->opening_job) return;
  sp_opening_job* j = c->opening_job;
  c->opening_job = nullptr;
  if (j->hash_posted && c->pcs_worker) c->pcs_worker->wait();
  if (j->started) {
    (void)hipMemsetAsync(j->d_blocks, 0, j->blocks_bytes, c->stream2);
    (void)hipMemsetAsync(j->d_d, 0, j->vec_bytes, c->stream2);
    (void)hipMemsetAsync(j->d_params, 0, j->params_bytes, c->stream2);
    (void)hipMemsetAsync(j->d_ip, 0, j->ip_bytes, c->stream2);
    (void)hipMemsetAsync(j->d_ticket, 0, j->tick_bytes, c->stream2);  // (a walk that was never joined leaves no count behind)
    (void)sp::stream_sync(c->stream2);  // (also: nothing of the job still reads the pinned buffer)
    if (c->h_opening && c->h_opening_bytes >= j->pinned_bytes) explicit_bzero(c->h_opening, j->pinned_bytes);
  }
  wipe_vec(j->blinds);
  wipe_vec(j->rng);
  wipe_vec(j->r_delta);
  wipe_vec(j->r_beta);
  wipe_vec(j->r_LZ);
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
  j->poly_d.resize(count);
  j->comm.resize(count * rows);
  j->blinds.resize(count * rows);
  j->rng.resize(count * 64 * (cols + 2));
  j->r_delta.assign(count, fe_zero());
  j->r_beta.assign(count, fe_zero());
  j->r_LZ.assign(count, fe_zero());
  for (size_t k = 0; k < count; ++k) {
    j->poly_d[k] = poly[k]->d;
    memcpy(&j->comm[k * rows], comm_rows_aff[k], rows * sizeof(aff_t));
    memcpy(&j->blinds[k * rows], blinds[k], rows * sizeof(fe_t));
    memcpy(&j->rng[k * 64 * (cols + 2)], rng[k], 64 * (cols + 2));
    // E::Scalar::random draws behind the mask vector (ipa.rs:146-149): the blinds of delta and beta
    j->r_delta[k] = fe_from_uniform<SF>(rng[k] + 64 * cols);
    j->r_beta[k] = fe_from_uniform<SF>(rng[k] + 64 * (cols + 1));
    j->r_LZ[k] = j->blinds[k * rows];  // a single row's commitment is the row itself and r_LZ its blind (hyrax_pc.rs:417-423)
  }
  j->rows_done = nvr == 0;
  if (!started) {
    c->opening_job = owner.release();
    *job = j;
    return SP_OK;
  }
  // ---- buffers: as sp_hyrax_prove_batch's, with room for both halves of the walk and one params slot per stage
  const size_t nsc = sh.num_cols + 1, npt = sh.npt;
  j->nb_ip = (cols + spk::OB_STREAM_THREADS - 1) / spk::OB_STREAM_THREADS;
  j->nb_walk = (unsigned)((nsc * 32 + spk::OB_WALK_ITEMS - 1) / spk::OB_WALK_ITEMS);
  j->blocks_bytes = count * cols * 64;
  j->vec_bytes = count * cols * sizeof(fe_t);
  j->params_bytes = align256(align256(count * sizeof(spk::ObInst)) + count * (npt ? npt : 1) * sizeof(fe_t));
  j->ip_bytes = align256(count * j->nb_ip * sizeof(fe_t));
  j->sums_bytes = align256(2 * count * sizeof(jac_t));
  j->tick_bytes = align256(2 * count * sizeof(unsigned));
  const size_t part_bytes = 2 * count * (size_t)spk::OB_WALK_MAX_BLOCKS * sizeof(xyzz_t);
  j->d_blocks = (char*)c->workspace(sp_ctx::WS_OPENING_BLOCKS, j->blocks_bytes);
  fe_t* d_vecs = (fe_t*)c->workspace(sp_ctx::WS_OPENING_VECS, 3 * j->vec_bytes);
  j->d_params = (char*)c->workspace(sp_ctx::WS_OPENING_PARAMS, j->params_bytes);
  char* d_walk = (char*)c->workspace(sp_ctx::WS_OPENING_WALK, j->tick_bytes + part_bytes + j->sums_bytes + j->ip_bytes);
  if (!j->d_blocks || !d_vecs || !j->d_params || !d_walk) return SP_ERR_NO_DEVICE;
  j->d_d = d_vecs, j->d_lz = d_vecs + count * cols, j->d_z = d_vecs + 2 * count * cols;
  j->d_ticket = reinterpret_cast<unsigned*>(d_walk);
  j->d_part = reinterpret_cast<xyzz_t*>(d_walk + j->tick_bytes);
  j->d_sums = reinterpret_cast<jac_t*>(d_walk + j->tick_bytes + part_bytes);
  j->d_ip = reinterpret_cast<fe_t*>(d_walk + j->tick_bytes + part_bytes + j->sums_bytes);
  j->off_params[0] = align256(j->blocks_bytes);
  j->off_params[1] = j->off_params[0] + j->params_bytes;
  j->off_params[2] = j->off_params[1] + j->params_bytes;
  j->off_ip = j->off_params[2] + j->params_bytes;
  j->off_sums = j->off_ip + j->ip_bytes;
  j->off_z = j->off_sums + j->sums_bytes;
  j->pinned_bytes = j->off_z + j->vec_bytes;
  if (c->h_opening_bytes < j->pinned_bytes) {
    if (c->h_opening) hipHostFree(c->h_opening);
    c->h_opening = nullptr;
    c->h_opening_bytes = 0;
    SP_HIP(hipHostMalloc(&c->h_opening, j->pinned_bytes + j->pinned_bytes / 4));
    c->h_opening_bytes = j->pinned_bytes + j->pinned_bytes / 4;
  }
  if (!c->opening_ev) SP_HIP(hipEventCreateWithFlags(&c->opening_ev, hipEventDisableTiming));
  if (!c->pcs_worker) c->pcs_worker = new sp::Worker();
  j->started = true;
  c->opening_job = owner.release();  // from here on every exit leaves the job to _finish / _drop, which wait and wipe
  *job = nullptr;
  auto queue = [&]() -> int {
    // ---- the auxiliary stream takes over behind what the main stream holds now (the tables' and the workspaces' last writers)
    SP_HIP(hipEventRecord(c->opening_ev, c->stream));
    SP_HIP(hipStreamWaitEvent(c->stream2, c->opening_ev, 0));
    char* hp = static_cast<char*>(c->h_opening);
    for (size_t k = 0; k < count; ++k) memcpy(hp + k * cols * 64, rng[k], cols * 64);
    SP_HIP(hipMemcpyAsync(j->d_blocks, hp, j->blocks_bytes, hipMemcpyHostToDevice, c->stream2));
    if ((rc = upload_params(c, j, 0, nullptr, 0, 0))) return rc;
    SP_HIP(hipMemsetAsync(j->d_ticket, 0, j->tick_bytes, c->stream2));
    const spk::ObInst* d_inst = reinterpret_cast<const spk::ObInst*>(j->d_params);
    c->timed_on(c->stream2, "opening_batch_dvec", 96ull * count * cols, [&] {
      hipLaunchKernelGGL(spk::k_ob_dvec, dim3((unsigned)j->nb_ip, (unsigned)count), dim3(spk::OB_STREAM_THREADS), 0, c->stream2, d_inst, (unsigned)cols, j->d_d);
    });
    c->timed_on(c->stream2, "opening_batch_walk", 32ull * count * nsc, [&] {
      hipLaunchKernelGGL(spk::k_ob_walk, dim3(j->nb_walk, (unsigned)count), dim3(512), 0, c->stream2, d_inst, (unsigned)count, 0u, nsc, cols, (const aff_t*)ck->d_keytables, j->d_part,
                         j->d_ticket, j->d_sums);
    });
    SP_HIP(hipMemcpyAsync(hp + j->off_sums, j->d_sums, count * sizeof(jac_t), hipMemcpyDeviceToHost, c->stream2));
    return SP_OK;
  };
  if ((rc = queue())) {  // nothing of a job that could not be queued stays behind
    sp::opening_job_free(c);
    return rc;
  }
  *job = j;
  // ---- the helper thread: transcript.absorb(b"poly_com", comm) (hyrax_pc.rs:410) of every instance into a fresh sponge
  j->hashed.resize(count);
  j->hash_posted = true;
  c->pcs_worker->keep_hot(200);
  c->pcs_worker->submit([j] {
    static const char* b = "poly_commitment_begin";  // HyraxCommitment::to_transcript_bytes (hyrax_pc.rs:714-729)
    static const char* e = "poly_commitment_end";
    const size_t rows = j->sh.rows;
    uint8_t buf[64 * 16];
    for (size_t k = 0; k < j->sh.count; ++k) {
      sp::Keccak256State& h = j->hashed[k];
      h.init();
      h.update(reinterpret_cast<const uint8_t*>("poly_com"), 8);
      h.update(reinterpret_cast<const uint8_t*>(b), strlen(b));
      const aff_t* comm = &j->comm[k * rows];
      for (size_t i = 0; i < rows; i += 16) {
        const size_t m = rows - i < 16 ? rows - i : 16;
        for (size_t q = 0; q < m; ++q) sp::point_transcript_bytes(comm[i + q], buf + 64 * q);
        h.update(buf, 64 * m);
      }
      h.update(reinterpret_cast<const uint8_t*>(e), strlen(e));
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
  const size_t cols = s.cols, nvr = s.nvr;
  bool same = j->ck == ck && j->ck_eval == ck_eval && s.count == count && s.rows == rows && s.n == n && s.npt == npt;
  for (size_t k = 0; same && k < count; ++k)
    same = j->poly[k] == poly[k] && j->poly_d[k] == poly[k]->d && j->comm_ptr[k] == comm_rows_aff[k] && memcmp(&j->comm[k * rows], comm_rows_aff[k], rows * sizeof(aff_t)) == 0 &&
           memcmp(&j->blinds[k * rows], blinds[k], rows * sizeof(fe_t)) == 0 && memcmp(&j->rng[k * 64 * (cols + 2)], rng[k], 64 * (cols + 2)) == 0 &&
           (!nvr || !j->rows_done || memcmp(&j->row_pts[k * nvr], points + 4 * npt * k, nvr * sizeof(fe_t)) == 0);
  if (!same) return plain();
  rc = sp_hyrax_prove_retract(c);
  if (rc) return rc;
  for (size_t k = 0; k < count; ++k) tr[k]->join();
  (void)sp_walkers_keep_hot(300 + 50 * count);
  if (!j->rows_done && (rc = queue_rows(c, j, points, npt))) return rc;  // _rows was not called: its stage now, behind the delta walk
  // ---- the full points, then the block sums of <R, d>; their copy lands behind both walks' sums
  if ((rc = upload_params(c, j, 2, points, npt, npt))) return rc;
  const spk::ObInst* d_inst = reinterpret_cast<const spk::ObInst*>(j->d_params);
  char* hp = static_cast<char*>(c->h_opening);
  c->timed_on(c->stream2, "opening_batch_ip", 64ull * count * cols, [&] {
    hipLaunchKernelGGL(spk::k_ob_ip, dim3((unsigned)j->nb_ip, (unsigned)count), dim3(spk::OB_STREAM_THREADS), 0, c->stream2, d_inst, (unsigned)cols, (int)nvr, (int)(npt - nvr),
                       (const fe_t*)j->d_d, j->d_ip);
  });
  SP_HIP(hipMemcpyAsync(hp + j->off_ip, j->d_ip, count * j->nb_ip * sizeof(fe_t), hipMemcpyDeviceToHost, c->stream2));
  // host beside the device: the sponges hashed ahead go to the transcripts that have absorbed nothing since their last squeeze; the others are hashed now
  std::vector<Item> items(count);
  struct WipeItems {
    std::vector<Item>& v;
    ~WipeItems() { explicit_bzero(v.data(), v.size() * sizeof(Item)); }
  } wipe_items{items};
  Job J{&s, ck_eval, tr, comm_rows_aff, blinds, points, comm_eval_aff, blind_eval, out, items.data(), reinterpret_cast<const fe_t*>(hp + j->off_ip), j->nb_ip,
        reinterpret_cast<const jac_t*>(hp + j->off_sums)};
  c->pcs_worker->wait();
  for (size_t k = 0; k < count; ++k) {
    items[k].r_delta = j->r_delta[k];
    items[k].r_beta = j->r_beta[k];
    items[k].r_LZ = j->r_LZ[k];
  }
  par_instances(count, [&](size_t k) {
    const sp::Keccak256State& h = tr[k]->t.h;
    bool fresh = h.fill == 0;
    for (int i = 0; i < 25 && fresh; ++i) fresh = h.a[i] == 0;
    if (fresh) items[k].hashed = j->hashed[k];
    else stage_hash(J, k);
  });
  SP_HIP(sp::stream_sync(c->stream2));
  // ---- beta, the IPA's transcript part per instance, then z_vec = r LZ + d for all of them
  (void)sp_walkers_keep_hot(300);
  par_instances(count, [&](size_t k) {
    stage_beta(J, k);
    stage_ipa(J, k);
  });
  spk::ObChallenges ch;
  memset(&ch, 0, sizeof ch);
  for (size_t k = 0; k < count; ++k) {
    if (items[k].rc) return fail(items[k].rc, "transcript round counter overflow");
    ch.r[k] = items[k].r;
  }
  c->timed_on(c->stream2, "opening_batch_z", 96ull * count * cols, [&] {
    hipLaunchKernelGGL(spk::k_ob_z, dim3((unsigned)j->nb_ip, (unsigned)count), dim3(spk::OB_STREAM_THREADS), 0, c->stream2, d_inst, ch, (unsigned)cols, (const fe_t*)j->d_d, j->d_z);
  });
  SP_HIP(hipMemcpyAsync(hp + j->off_z, j->d_z, j->vec_bytes, hipMemcpyDeviceToHost, c->stream2));
  SP_HIP(sp::stream_sync(c->stream2));
  for (size_t k = 0; k < count; ++k) memcpy(out + k * out_words(s) + 16, hp + j->off_z + k * cols * sizeof(fe_t), cols * sizeof(fe_t));
  return SP_OK;
}
