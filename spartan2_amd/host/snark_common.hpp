// Pieces shared by the host-side protocol drivers above the C ABI (spartan_snark.cpp, sharded_snark.cpp, neutronnova_zk.cpp): the integer R1CS view and
// SplitR1CSShape::new padding, this build's generator derivation, the vk digest (the reference's SHA-256 stream), the O(sqrt N) host-side eq tables,
// the verifier-side pieces (sum-check verification, canonicity) and the prover-side ones: each host-side statement of SpartanSNARK::prove
// (src/spartan.rs:226-466) that more than one driver makes, stated once.
#pragma once
#include "host_common.hpp"

// What ss_verify_batch / ss_verify_bytes_batch and nnz_verify_batch / nnz_verify_bytes_batch report beside the codes (C layout: four 64-bit words; host.py VerifyBatchInfo mirrors it). The ss_* surface
// of this library has no header of its own: its types are declared at global scope, as a C caller would repeat them.
extern "C" {
typedef struct ss_verify_batch_info {
  uint64_t matrix_chunks;       // sp_shape_matrix_evals_batched calls
  uint64_t opening_batched_ok;  // 1: the combined equations held (or no proof reached them)
  uint64_t fallback_proofs;     // proofs that went through the single-proof opening check
  uint64_t opening_proofs;      // proofs that reached the combined equations
} ss_verify_batch_info;
}

namespace spartan2 {

// ---- integer R1CS as produced by the frontend (arguments of SplitR1CSShape::new) ---------------------------------------
struct CsrIntView {
  const int64_t* data;
  const uint32_t* indices;
  const uint64_t* indptr;
};
struct R1CSIntView {
  size_t num_cons, num_shared, num_precommitted, num_rest, num_public, num_challenges;
  CsrIntView m[3];
};

struct PaddedShape {
  sp_dims dims;
  std::vector<fe_t> data[3];
  std::vector<uint32_t> idx[3];
  std::vector<uint64_t> ptr[3];
  size_t num_vars() const { return dims.num_shared + dims.num_precommitted + dims.num_rest; }
  size_t num_cols() const { return num_vars() + 1 + dims.num_public + dims.num_challenges; }
};

inline size_t pad_to_width(size_t w, size_t n) { return (n + w - 1) / w * w; }
inline size_t next_pow2(size_t n) {
  size_t p = 1;
  while (p < n) p <<= 1;
  return p;
}
inline size_t log2_ceil(size_t n) {
  size_t l = 0;
  while (((size_t)1 << l) < n) ++l;
  return l;
}

// SplitR1CSShape::new (src/r1cs/mod.rs:810-911)
// the ten dimensions it gives a circuit of these sizes (:810-854): what a loaded key's dimensions are checked against
inline sp_dims padded_dims(size_t num_cons, size_t num_shared, size_t num_precommitted, size_t num_rest, size_t num_public, size_t num_challenges) {
  const size_t width = DEFAULT_COMMITMENT_WIDTH;
  size_t sp_ = pad_to_width(width, num_shared), pp = pad_to_width(width, num_precommitted), rp = pad_to_width(width, num_rest);
  size_t nvp = sp_ + pp + rp;
  if (nvp < num_public + num_challenges + 1) rp = std::max(num_public + num_challenges + 1, nvp) - (sp_ + pp);
  nvp = sp_ + pp + rp;
  if (next_pow2(nvp) != nvp) rp = next_pow2(nvp) - (sp_ + pp);
  sp_dims d;
  d.num_cons = next_pow2(num_cons);
  d.num_cons_unpadded = num_cons;
  d.num_shared = sp_;
  d.num_precommitted = pp;
  d.num_rest = rp;
  d.num_shared_unpadded = num_shared;
  d.num_precommitted_unpadded = num_precommitted;
  d.num_rest_unpadded = num_rest;
  d.num_public = num_public;
  d.num_challenges = num_challenges;
  return d;
}
inline PaddedShape pad_shape(const R1CSIntView& R) {
  PaddedShape P;
  P.dims = padded_dims(R.num_cons, R.num_shared, R.num_precommitted, R.num_rest, R.num_public, R.num_challenges);
  const size_t sp_ = P.dims.num_shared, pp = P.dims.num_precommitted, nvp = sp_ + pp + P.dims.num_rest;
  const size_t num_vars = R.num_shared + R.num_precommitted + R.num_rest;
  const size_t ncp = P.dims.num_cons;
  // small coefficient cache: the SHA circuits only use +-2^k
  for (int m = 0; m < 3; ++m) {
    const size_t nnz = R.m[m].indptr[R.num_cons];
    P.data[m].resize(nnz);
    P.idx[m].resize(nnz);
    for (size_t k = 0; k < nnz; ++k) {
      P.data[m][k] = fe_from_i64<S>(R.m[m].data[k]);
      size_t c = R.m[m].indices[k];
      if (c >= R.num_shared && c < R.num_shared + R.num_precommitted) c += sp_ - R.num_shared;
      else if (c >= R.num_shared + R.num_precommitted && c < num_vars) c += sp_ + pp - R.num_shared - R.num_precommitted;
      else if (c >= num_vars) c += nvp - num_vars;
      P.idx[m][k] = (uint32_t)c;
    }
    P.ptr[m].assign(R.m[m].indptr, R.m[m].indptr + R.num_cons + 1);
    P.ptr[m].resize(ncp + 1, nnz);
  }
  return P;
}

// SplitR1CSShape::equalize (src/r1cs/mod.rs:913-971): the larger constraint count (row pointers extended with the last offset) and the larger variable
// count (growth into num_rest; the columns of 1 | public | challenges move up by it) for both shapes
inline void equalize(PaddedShape& A, PaddedShape& B) {
  const size_t cons = std::max<size_t>(A.dims.num_cons, B.dims.num_cons), vars = std::max(A.num_vars(), B.num_vars());
  auto grow = [&](PaddedShape& S) {
    const size_t orig_cons = S.dims.num_cons, nv = S.num_vars();
    S.dims.num_cons = cons;
    if (nv != vars) S.dims.num_rest = vars - (S.dims.num_shared + S.dims.num_precommitted);
    for (int m = 0; m < 3; ++m) {
      for (uint32_t& c : S.idx[m])
        if (c >= nv) c += (uint32_t)(vars - nv);
      const uint64_t nnz = S.ptr[m].empty() ? 0 : S.ptr[m].back();
      S.ptr[m].resize(S.ptr[m].size() + (cons - orig_cons), nnz);
    }
  };
  grow(A);
  grow(B);
}

// DigestHelperTrait::digest of SpartanVerifierKey (src/spartan.rs:73-104): SHA-256 over bincode(vk_ee) || bincode(ck_s) || S.write_bytes(), through the
// library's wire sink (include/spartan_hip.h "wire formats"). gens / gens_s = the num_cols + 1 generators of each key, h last.
inline void padded_csr(const PaddedShape& P, sp_csr cs[3]) {
  for (int m = 0; m < 3; ++m) cs[m] = sp_csr{u64p(P.data[m].data()), P.idx[m].data(), P.ptr[m].data()};
}
inline void spartan_vk_digest(const PaddedShape& P, const std::vector<aff_t>& gens, const std::vector<aff_t>& gens_s, uint8_t out[32]) {
  sp_csr cs[3];
  padded_csr(P, cs);
  ck(sp_vk_digest(&P.dims, &cs[0], &cs[1], &cs[2], u64p(&gens[0].x), gens.size() - 1, u64p(&gens.back().x), u64p(&gens_s[0].x), gens_s.size() - 1,
                  u64p(&gens_s.back().x), out),
     "vk digest");
}

// This build's generator derivation (documented in DESIGN.md; shape of src/provider/traits.rs:205-249):
// SHAKE256(label) stream, 32 bytes per generator -> x = bytes LE mod p; increment x until x^3 - 3x + b is a non-zero square;
// y = rhs^((p+1)/4), take the root with even canonical value.
inline std::vector<aff_t> from_label(const char* label, size_t n) {
  sp::Shake256State sh;
  sh.init();
  sh.update((const uint8_t*)label, strlen(label));
  uint32_t e[8], c = 0;
  for (int i = 0; i < 8; ++i) e[i] = sp_addc(FpP::P(i), i == 0 ? 1u : 0u, c);  // p + 1
  for (int i = 0; i < 7; ++i) e[i] = (e[i] >> 2) | (e[i + 1] << 30);
  e[7] >>= 2;
  std::vector<aff_t> out(n);
  const fe_t b = T256::b(), one = fe_one<B>();
  for (size_t i = 0; i < n; ++i) {
    uint8_t buf[64];
    memset(buf, 0, 64);
    sh.read(buf, 32);
    fe_t x = fe_from_uniform<B>(buf);
    for (;;) {
      fe_t rhs = fe_add<B>(fe_sub<B>(fe_mul<B>(fe_sqr<B>(x), x), fe_add<B>(fe_dbl<B>(x), x)), b);
      fe_t y = fe_pow<B>(rhs, e);
      if (!fe_is_zero(rhs) && fe_eq(fe_sqr<B>(y), rhs)) {
        fe_t yc = fe_to_canonical<B>(y);
        if (yc.v[0] & 1u) y = fe_neg<B>(y);
        out[i].x = x;
        out[i].y = y;
        break;
      }
      x = fe_add<B>(x, one);
    }
  }
  return out;
}

// EqPolynomial::evals_from_points on the host for the O(sqrt N) tables of the opening (src/polys/eq.rs:59-92)
inline std::vector<fe_t> eq_evals_host(const fe_t* r, size_t ell) {
  std::vector<fe_t> ev((size_t)1 << ell, fe_zero());
  ev[0] = fe_one<S>();
  size_t size = 1;
  for (size_t k = ell; k-- > 0;) {
    for (size_t i = 0; i < size; ++i) {
      fe_t y = fe_mul<S>(ev[i], r[k]);
      ev[size + i] = y;
      ev[i] = fe_sub<S>(ev[i], y);
    }
    size *= 2;
  }
  return ev;
}
// SparsePolynomial::evaluate (src/polys/multilinear.rs:190-207)
inline fe_t sparse_poly_evaluate(size_t num_vars, const std::vector<fe_t>& Z, const fe_t* r) {
  size_t nvz = log2_ceil(Z.size());
  // the reference asserts the same relation (SparsePolynomial::evaluate, multilinear.rs:196); an instance with log2(M) == log2_ceil(1 + num_public)
  // has no room for the (1, X) block beside W
  if (num_vars < nvz + 1) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "SparsePolynomial::evaluate: too many public values for this many variables");
  std::vector<fe_t> chis = eq_evals_host(r + (num_vars - 1 - nvz), nvz + 1);
  fe_t partial = fe_zero();
  for (size_t i = 0; i < Z.size(); ++i) partial = fe_add<S>(partial, fe_mul<S>(Z[i], chis[i]));
  fe_t common = fe_one<S>();
  for (size_t i = 0; i < num_vars - 1 - nvz; ++i) common = fe_mul<S>(common, fe_sub<S>(fe_one<S>(), r[i]));
  return fe_mul<S>(common, partial);
}

// ---- verifier-side pieces shared by SpartanSNARK::verify and NeutronNovaZkSNARK::verify ------------------------------------------------------
inline bool same_point(const jac_t& a, const jac_t& b) {
  const aff_t x = jac_to_affine(a), y = jac_to_affine(b);
  return fe_eq(x.x, y.x) && fe_eq(x.y, y.y);
}
// SumcheckProof::verify (src/sumcheck.rs:67-114) on compressed polynomials of `deg` + 1 coefficients minus the linear one
inline bool sumcheck_verify(Tr& tr, const fe_t& claim, size_t rounds, size_t deg, const fe_t* cpolys, fe_t* e_out, std::vector<fe_t>* r_out) {
  fe_t e = claim;
  r_out->clear();
  for (size_t i = 0; i < rounds; ++i) {
    const fe_t* c = cpolys + i * deg;  // c[0] = constant, c[1..] = degree 2.. coefficients
    fe_t lin = fe_sub<S>(fe_sub<S>(e, c[0]), c[0]);  // CompressedUniPoly::decompress (univariate.rs:166-179)
    for (size_t k = 1; k < deg; ++k) lin = fe_sub<S>(lin, c[k]);
    std::vector<uint8_t> b(32 * deg);
    for (size_t k = 0; k < deg; ++k) sp::fe_to_le_bytes<S>(c[k], b.data() + 32 * k);
    tr.absorb("p", b.data(), b.size());
    const fe_t r = tr.squeeze("c");
    r_out->push_back(r);
    fe_t eval = c[0], power = r;  // UniPoly::evaluate on (c0, lin, c[1], ...)
    eval = fe_add<S>(eval, fe_mul<S>(power, lin));
    for (size_t k = 1; k < deg; ++k) {
      power = fe_mul<S>(power, r);
      eval = fe_add<S>(eval, fe_mul<S>(power, c[k]));
    }
    e = eval;
  }
  *e_out = e;
  return true;
}

// every scalar / coordinate of an untrusted proof must be a canonical residue: the reference's deserialisation rejects anything >= the modulus,
// and x and x + p would otherwise be two encodings of one proof (same transcript bytes, same group elements)
template <class F>
inline bool limbs_canonical(const fe_t& v) {
  for (int i = 7; i >= 0; --i) {
    if (v.v[i] < F::P(i)) return true;
    if (v.v[i] > F::P(i)) return false;
  }
  return false;  // == p
}


struct ProofBuf {  // a proof in the canonical flat layout of DESIGN.md section 4, appended field by field
  std::vector<uint64_t> words;
  void pf(const fe_t& f) { words.insert(words.end(), u64p(&f), u64p(&f) + 4); }
  void pp(const aff_t& a) {
    pf(a.x);
    pf(a.y);
  }
  void pc(const std::vector<aff_t>& c) {
    for (const aff_t& a : c) pp(a);
  }
  void pfs(const fe_t* f, size_t n) { words.insert(words.end(), u64p(f), u64p(f) + 4 * n); }
  // the blocks a prover appends, in order: the instance (comm_W, public values, challenges - SplitR1CSInstance carries them, src/r1cs/mod.rs:1423-1437), ...
  void header(const std::vector<aff_t>& comm_W, const std::vector<fe_t>& publics, const std::vector<fe_t>& challenges) {
    pc(comm_W);
    pfs(publics.data(), publics.size());
    pfs(challenges.data(), challenges.size());
  }
  // ... the outer sum-check's 3 coefficients a round and its three claims (src/spartan.rs:291-310), the inner one's 2 a round (:323-404)
  void outer(const fe_t* polys, size_t rounds, const fe_t claims[3]) {
    pfs(polys, 3 * rounds);
    pfs(claims, 3);
  }
  void inner(const fe_t* polys, size_t rounds) { pfs(polys, 2 * rounds); }
};

// ---- prover-side pieces shared by the Spartan drivers -----------------------------------------------------------------------------------------------
// The statements of SpartanSNARK::prove (src/spartan.rs:226-466, bellpepper/r1cs.rs:411-540) that prove, prove_reference_order, prove_batch_chunk
// (spartan_snark.cpp), sharded_prove (sharded_snark.cpp) and is_sat make alike. Each driver stays straight-line code in its own order - what it issues
// when, on which thread, through which entry point - and calls these for the statement bodies. Nothing here knows a key or a prep-state type.

// `synth`: circuit.synthesize(.., Some(&challenges)) for circuits with verifier challenges (bellpepper/r1cs.rs:443-461): receives the challenges and
// writes the num_rest_unpadded values of the rest segment (Montgomery limbs); non-zero return = SynthesisError
typedef int (*ss_rest_hook)(void* user, const uint64_t* challenges, size_t num_challenges, uint64_t* out_rest);

inline std::vector<fe_t> publics_from_u64(const uint64_t* publics_u64, size_t n) {
  std::vector<fe_t> publics(n);
  for (size_t i = 0; i < n; ++i) publics[i] = fe_from_u64<S>(publics_u64[i]);
  return publics;
}
// the transcript up to the rest commitment (src/spartan.rs:226-236, bellpepper/r1cs.rs:422-427): vk, public_values, comm_W_shared, comm_W_precommitted.
// shared_bytes / pre_bytes: the commitments' transcript encodings (commitment_bytes), empty for a segment without variables
inline void absorb_instance_prefix(Tr& tr, const uint8_t vk_digest[32], const fe_t* publics, size_t n, const std::vector<uint8_t>& shared_bytes,
                                   const std::vector<uint8_t>& pre_bytes) {
  tr.absorb("vk", vk_digest, 32);
  tr.absorb_scalars("public_values", publics, n);
  if (!shared_bytes.empty()) tr.absorb("comm_W_shared", shared_bytes.data(), shared_bytes.size());
  if (!pre_bytes.empty()) tr.absorb("comm_W_precommitted", pre_bytes.data(), pre_bytes.size());
}
// verifier challenges (bellpepper/r1cs.rs:429-431): squeezed right after the precommitted commitment
inline std::vector<fe_t> squeeze_challenges(Tr& tr, size_t n) {
  std::vector<fe_t> challenges(n);
  for (auto& c : challenges) c = tr.squeeze("challenge");
  return challenges;
}
// the rest of the witness that depends on the challenges (bellpepper/r1cs.rs:443-461): n_rest_unpadded values (+ one spare element) from the circuit's hook
inline std::vector<fe_t> synthesize_rest(ss_rest_hook synth, void* synth_user, const uint64_t* challenges, size_t num_challenges, size_t n_rest_unpadded) {
  if (!synth) throw Error(SP_ERR_INTERNAL, "a circuit with verifier challenges needs its synthesize callback");
  std::vector<fe_t> rest(n_rest_unpadded + 1);
  if (synth(synth_user, challenges, num_challenges, u64p(rest.data())) != 0) throw Error(SP_ERR_INTERNAL, "SynthesisError: the circuit's synthesize callback failed");
  return rest;
}
// the last num_extra entries of z = [W | 1 | public | challenges] (src/spartan.rs:246-253)
inline std::vector<fe_t> z_tail(size_t num_extra, const std::vector<fe_t>& publics, const std::vector<fe_t>& challenges) {
  std::vector<fe_t> tail(num_extra);
  tail[0] = fe_one<S>();
  std::copy(publics.begin(), publics.end(), tail.begin() + 1);
  std::copy(challenges.begin(), challenges.end(), tail.begin() + 1 + publics.size());
  return tail;
}
// the rest segment's commitment for one proof, on the calling thread (bellpepper/r1cs.rs:463-491): PCS::commit of a segment with values ...
inline void commit_rest_values(sp_ctx* ctx, const sp_ck* key, const sp_table* W, const sp_dims& d, bool is_small, const fe_t* blinds, aff_t* out) {
  ck(sp_hyrax_commit(ctx, key, W, d.num_shared + d.num_precommitted, d.num_rest, u64p(blinds), is_small ? 1 : 0, u64p(&out->x)), "commit rest");
}
// ... and commit_zeros (hyrax_pc.rs:305-319; h * blind per row) of one that is all padding
inline void commit_rest_rows(sp_ctx* ctx, const sp_ck* key, const sp_table* W, const sp_dims& d, bool is_small, const fe_t* blinds, size_t rows_rest, aff_t* out) {
  if (rows_rest && d.num_rest_unpadded == 0) ck(sp_fixed_base_mul_h(ctx, key, u64p(blinds), rows_rest, u64p(&out->x)), "commit_zeros");  // :467-469
  else if (rows_rest) commit_rest_values(ctx, key, W, d, is_small, blinds, out);
}
inline void absorb_comm_W_rest(Tr& tr, const aff_t* rest_rows, size_t rows_rest) {
  const std::vector<uint8_t> b = commitment_bytes(rest_rows, rows_rest);
  tr.absorb("comm_W_rest", b.data(), b.size());
}
// combine_blinds (bellpepper/r1cs.rs:515-524): the blinds of the rows committed at prep time, then the rest rows'
inline std::vector<fe_t> combine_blinds(const std::vector<fe_t>& r_W_fixed, const std::vector<fe_t>& r_W_rest) {
  std::vector<fe_t> r_W = r_W_fixed;
  r_W.insert(r_W.end(), r_W_rest.begin(), r_W_rest.end());
  return r_W;
}
// an error exit between sp_fixed_base_mul_h_begin and _finish must not leave the context's one asynchronous fixed-base job outstanding
struct FbJobGuard {
  sp_ctx* ctx;
  sp_fb_job*& job;
  size_t n;
  ~FbJobGuard() {
    if (job) {
      std::vector<uint64_t> sink(8 * n + 8);
      (void)sp_fixed_base_mul_h_finish(ctx, job, sink.data());
      job = nullptr;
    }
  }
};
// claim_inner_joint = claims_outer[0] + r claims_outer[1] + r^2 claims_outer[2]   (src/spartan.rs:311-315)
inline fe_t joint_inner_claim(const fe_t claims_outer[3], const fe_t& r, const fe_t& r2) {  // (a caller that holds r^2)
  return fe_add<S>(fe_add<S>(claims_outer[0], fe_mul<S>(r, claims_outer[1])), fe_mul<S>(r2, claims_outer[2]));
}
inline fe_t joint_inner_claim(const fe_t claims_outer[3], const fe_t& r) { return joint_inner_claim(claims_outer, r, fe_mul<S>(r, r)); }
// eval_W = (eval_Z - r_y0 eval_X) / (1 - r_y0)   (src/spartan.rs:405-421): the division, once per point (NeutronNova has a step and a core claim at one r_y) ...
inline fe_t inv_one_minus(const fe_t& r_y0) {
  const fe_t denom = fe_sub<S>(fe_one<S>(), r_y0);
  if (fe_is_zero(denom)) throw Error(SP_ERR_DIVISION_BY_ZERO, "DivisionByZero");
  return fe_inv_vartime<S>(denom);
}
inline fe_t eval_W_from(const fe_t& eval_Z, const fe_t& r_y0, const fe_t& eval_X, const fe_t& inv) { return fe_mul<S>(fe_sub<S>(eval_Z, fe_mul<S>(r_y0, eval_X)), inv); }
// ... and the whole of it; to_regular_instance: X = public_values ++ challenges (src/r1cs/mod.rs:1546-1549)
inline fe_t eval_W_from(const fe_t& eval_Z, const fe_t* r_y, size_t num_rounds_y, const std::vector<fe_t>& publics, const std::vector<fe_t>& challenges) {
  const fe_t eval_X = sparse_poly_evaluate(num_rounds_y - 1, z_tail(1 + publics.size() + challenges.size(), publics, challenges), r_y + 1);
  return eval_W_from(eval_Z, r_y[0], eval_X, inv_one_minus(r_y[0]));
}
// the IPA's instance and first message in front of its challenge (ipa.rs:128-152): U = (comm_LZ, comm_eval_W), delta, beta
inline void absorb_ipa_instance(Tr& tr, const aff_t& comm_LZ, const aff_t& comm_eval_W, const aff_t& delta, const aff_t& beta) {
  uint8_t b[128];
  point_bytes(comm_LZ, b);
  point_bytes(comm_eval_W, b + 64);
  tr.absorb("U", b, 128);
  point_bytes(delta, b);
  tr.absorb("delta", b, 64);
  point_bytes(beta, b);
  tr.absorb("beta", b, 64);
}
// a prove's wall-clock per phase from its seven time stamps (ms): witness_commit, matvec, outer, poly_abc, inner, pcs, total. mv_issue: the time spent
// issuing the matrix-vector product inside the witness phase (the driver that issues it there books it with the product)
inline void fill_phase_ms(double ms[8], double t_start, double t_wit, double t_mv, double t_outer, double t_abc, double t_inner, double t_end, double mv_issue = 0) {
  ms[0] = t_wit - t_start - mv_issue;
  ms[1] = t_mv - t_wit + mv_issue;
  ms[2] = t_outer - t_mv;
  ms[3] = t_abc - t_outer;
  ms[4] = t_inner - t_abc;
  ms[5] = t_end - t_inner;
  ms[6] = t_end - t_start;
}

// <z_vec, ck> of the IPA check (ipa.rs:196-203) depends on nothing but the proof: a verifier starts its device part before the transcript work
struct ZJob {
  sp_ctx* ctx = nullptr;
  const sp_ck* key = nullptr;
  sp_msm_job* job = nullptr;
  ZJob() = default;
  ZJob(const ZJob&) = delete;
  ZJob& operator=(const ZJob&) = delete;
  ~ZJob() {
    uint64_t sink[8];
    if (job) sp_msm_ck_finish(ctx, key, job, nullptr, sink);  // an early return still owns the job
  }
};

inline R1CSIntView make_view(size_t num_cons, size_t num_shared, size_t num_precommitted, size_t num_rest, size_t num_public, size_t num_challenges,
                             const int64_t* Ad, const uint32_t* Ai, const uint64_t* Ap, const int64_t* Bd, const uint32_t* Bi, const uint64_t* Bp,
                             const int64_t* Cd, const uint32_t* Ci, const uint64_t* Cp) {
  R1CSIntView R{num_cons, num_shared, num_precommitted, num_rest, num_public, num_challenges, {{Ad, Ai, Ap}, {Bd, Bi, Bp}, {Cd, Ci, Cp}}};
  return R;
}

}  // namespace spartan2
