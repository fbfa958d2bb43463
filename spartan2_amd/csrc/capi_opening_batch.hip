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
#include <cstring>
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
}  // namespace

extern "C" int sp_hyrax_prove_batch(sp_ctx* c, const sp_ck* ck, const sp_ck* ck_eval, size_t count, sp_transcript* const* tr, const uint64_t* const* comm_rows_aff,
                                    size_t rows, const sp_table* const* poly, size_t n, const uint64_t* const* blinds, const uint64_t* points, size_t npt,
                                    const uint64_t* comm_eval_aff, const uint64_t* blind_eval, const uint8_t* const* rng, const size_t* rng_blocks, uint64_t* out) {
  const std::string w(WHO);
  // ---- refusals: nothing is launched, absorbed or written before the last of them
  if (count == 0 || count > SP_LOCKSTEP_MAX) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": count must be 1 .. SP_LOCKSTEP_MAX");
  if (!c || !ck || !ck_eval || !tr || !comm_rows_aff || !poly || !blinds || (!points && npt) || !comm_eval_aff || !blind_eval || !rng || !rng_blocks || !out)
    return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null argument");
  for (size_t k = 0; k < count; ++k) {
    const char* what = !tr[k] ? "transcript" : !comm_rows_aff[k] ? "commitment" : (!poly[k] || !poly[k]->d) ? "table" : !blinds[k] ? "blinds" : !rng[k] ? "randomness stream" : nullptr;
    if (what) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null " + what + ", instance " + std::to_string(k));
  }
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
  for (size_t k = 0; k < count; ++k)
    for (size_t j = 0; j < k; ++j)
      if (tr[j] == tr[k]) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": the same transcript twice, instances " + std::to_string(j) + " and " + std::to_string(k));
  if (!ck_eval->d_cktables || ck_eval->num_cols < 1) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": ck_eval must be a narrow key with tables");

  SP_HIP(hipSetDevice(c->device));
  int rc = sp_hyrax_prove_retract(c);  // an announced opening is not this call's: withdrawn, never consumed
  if (rc) return rc;
  const Shape sh{count, rows, n, npt, nvr, cols, num_cols};
  auto per_instance = [&]() -> int {
    for (size_t k = 0; k < count; ++k) {
      const int r = sp_hyrax_prove(c, ck, ck_eval, tr[k], comm_rows_aff[k], rows, poly[k], n, blinds[k], points + 4 * npt * k, npt, comm_eval_aff + 8 * k, blind_eval + 4 * k,
                                   rng[k], rng_blocks[k], out + k * out_words(sh));
      if (r) return r;
    }
    return SP_OK;
  };
  // the batched stages walk the window tables of a key of 1023 .. 4095 columns (k_ob_walk is k_multi_mul_wide's shape) and keep the row weights in LDS
  const size_t nsc = num_cols + 1;
  const bool shape_ok = nsc >= sp::multi_mul_wide_min() && nsc * 32 <= (size_t)spk::OB_WALK_MAX_BLOCKS * spk::OB_WALK_ITEMS && cols <= num_cols && nvr <= (size_t)spk::OB_ROW_BITS_MAX;
  if (count == 1 || !shape_ok) return per_instance();
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
    hipLaunchKernelGGL(spk::k_ob_walk, dim3(nb_walk, (unsigned)nvec), dim3(512), 0, c->stream, d_inst, (unsigned)count, nsc, cols, (const aff_t*)ck->d_keytables, d_part, d_ticket,
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
