// Lockstep sum-checks (include/spartan_hip.h, "many sum-checks of one length in lockstep"): `count` independent instances of
// prove_cubic_with_three_inputs / prove_quad over `count` table sets of one length. One launch computes round i of every instance
// (kernels_lockstep.hpp), one wait collects the `count` records, the host finishes `count` round polynomials (sumcheck_round.hpp: the algebra of the
// host-table provers), feeds each to its own transcript and hands the `count` challenges to the next launch by value. A round trip per round, as for
// a lone instance - shared by all of them. Every instance's polynomials, challenges, final claims and transcript are those of sp_sumcheck_cubic3 /
// sp_sumcheck_quad on that instance alone. The _observed forms report each round's challenges to a hook of the caller once the next launch is queued.
// gfx950 only; no CPU fallback.
#include <cstring>
#include <string>
#include <vector>

#include "core.hpp"
#include "kernels_lockstep.hpp"
#include "sumcheck_round.hpp"

using sp::fail;
typedef FqP S;
static_assert(SP_LOCKSTEP_MAX == spk::LS_MAX, "the kernels' argument structs hold SP_LOCKSTEP_MAX instances");
static_assert(SP_LOCKSTEP_MAX <= spk::HOST_SUM_MAX_BLOCKS, "a record is a result slot of the mapped buffer");

namespace {
inline fe_t load_fe(const uint64_t* p) {
  fe_t r;
  memcpy(&r, p, 32);
  return r;
}
inline void store_fe(uint64_t* p, const fe_t& a) { memcpy(p, &a, 32); }

// the refusals shared by both entry points: nothing has been launched and no table touched when one of them is returned
int check_instances(const char* who, size_t count, size_t vars, sp_table* const* const* tabs, int ntab, sp_transcript* const* tr) {
  const std::string w(who);
  if (count == 0 || count > SP_LOCKSTEP_MAX) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": count must be 1 .. SP_LOCKSTEP_MAX");
  if (!tr) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null argument");
  for (int t = 0; t < ntab; ++t)
    if (!tabs[t]) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null argument");
  for (size_t k = 0; k < count; ++k) {
    if (!tr[k]) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null transcript, instance " + std::to_string(k));
    for (int t = 0; t < ntab; ++t)
      if (!tabs[t][k] || !tabs[t][k]->d) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null table, instance " + std::to_string(k));
  }
  const size_t len0 = tabs[0][0]->len;
  for (size_t k = 0; k < count; ++k)
    for (int t = 0; t < ntab; ++t)
      if (tabs[t][k]->len != len0) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": tables of differing length, instance " + std::to_string(k));
  if (vars == 0 || vars > 30 || len0 != ((size_t)1 << vars)) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": tables must have 2^rounds elements");
  for (size_t k = 0; k < count; ++k) {
    for (size_t j = 0; j < k; ++j)
      if (tr[j] == tr[k]) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": the same transcript twice, instances " + std::to_string(j) + " and " + std::to_string(k));
    for (int t = 0; t < ntab; ++t)
      for (size_t j = 0; j <= k; ++j)
        for (int u = 0; u < ntab; ++u) {
          if (j == k && u >= t) break;
          if (tabs[u][j] == tabs[t][k] || tabs[u][j]->d == tabs[t][k]->d)
            return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": the same table twice, instances " + std::to_string(j) + " and " + std::to_string(k));
        }
  }
  return SP_OK;
}
unsigned next_seq(sp_ctx* c) {
  c->pending_slots = 0;
  return ++c->result_seq;
}
// the `count` records of the launch that carries `seq`: nvals elements each, record k in v[3 k ..)
int wait_records(sp_ctx* c, size_t count, unsigned seq, int nvals, fe_t* v) {
  long spins = 0;
  for (size_t k = 0; k < count; ++k) {
    const int rc = sp::wait_result_slot(c, c->h_pinned + spk::SLOT_BASE_ELEM + 4 * k, seq, nvals, v + 3 * k, &spins);
    if (rc) return rc;
  }
  return SP_OK;
}
unsigned blocks_per_instance(size_t q) { return (unsigned)((q + spk::LS_CHUNK - 1) / spk::LS_CHUNK); }
// the caller's hook (sp_*_lockstep_observed): the challenges of `round`, reported once the launch that consumes them is queued
void report(sp_lockstep_hook observe, void* user, size_t round, const spk::LsChallenges& ch) {
  if (observe) observe(user, round, reinterpret_cast<const uint64_t*>(ch.r));
}
}  // namespace

extern "C" {

int sp_sumcheck_cubic3_lockstep_observed(sp_ctx* c, size_t count, const uint64_t* claims, const uint64_t* taus_, size_t ell, sp_table* const* A, sp_table* const* B,
                                         sp_table* const* C, sp_transcript* const* tr, uint64_t* out_cpolys, uint64_t* out_r, uint64_t* out_final, sp_lockstep_hook observe,
                                         void* user) {
  static const char* who = "prove_cubic_with_three_inputs (lockstep)";
  if (!c || !claims || !taus_ || !out_cpolys || !out_r || !out_final) return fail(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": null argument");
  sp_table* const* tabs[3] = {A, B, C};
  int rc = check_instances(who, count, ell, tabs, 3, tr);
  if (rc) return rc;
  const size_t N = (size_t)1 << ell;
  // EqSumCheckInstance::new (src/sumcheck.rs:956-1016), per instance: pyramids over taus[1..first_half) and taus[first_half..ell). The split is this
  // prover's own (the weights are the product either way): the right table takes the last LS_EQ_IN_BITS variables, one chunk of pairs
  const size_t second_half = ell < (size_t)spk::LS_EQ_IN_BITS ? ell : (size_t)spk::LS_EQ_IN_BITS, first_half = ell - second_half;
  const size_t nleft = first_half > 0 ? first_half - 1 : 0;
  if (nleft > 16) return fail(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": tables must have 2^rounds elements, rounds <= 27");
  const size_t pyr_left = (size_t)2 << nleft, pyr_right = (size_t)2 << second_half, stride = pyr_left + pyr_right;
  fe_t* d_eq = static_cast<fe_t*>(c->workspace(sp_ctx::WS_LOCKSTEP_EQ, count * stride * sizeof(fe_t)));
  const unsigned nb_max = blocks_per_instance(N / 2);
  fe_t* d_part = static_cast<fe_t*>(c->workspace(sp_ctx::WS_LOCKSTEP_PARTIALS, count * (size_t)nb_max * 3 * sizeof(fe_t)));
  if (!d_eq || !d_part) return SP_ERR_NO_DEVICE;
  for (size_t k = 0; k < count; ++k) tr[k]->join();

  std::vector<fe_t> taus(count * ell), inv_tau(count * ell), claim(count), p(count, fe_one<S>());
  spk::LsTables3 tb;
  for (size_t k = 0; k < count; ++k) {
    for (size_t i = 0; i < ell; ++i) taus[k * ell + i] = load_fe(taus_ + 4 * (k * ell + i));
    sp::batch_inv_taus(&taus[k * ell], ell, &inv_tau[k * ell]);  // one inversion per instance
    claim[k] = load_fe(claims + 4 * k);
    tb.a[k] = A[k]->d;
    tb.b[k] = B[k]->d;
    tb.c[k] = C[k]->d;
  }
  {  // the taus go up once; every instance's two pyramids are one launch
    fe_t* d_taus = static_cast<fe_t*>(c->workspace(sp_ctx::WS_LOCKSTEP_PARAMS, taus.size() * sizeof(fe_t)));
    if (!d_taus) return SP_ERR_NO_DEVICE;
    SP_HIP(hipMemcpyAsync(d_taus, taus.data(), taus.size() * sizeof(fe_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(spk::k_ls_eq_levels, dim3(2, (unsigned)count), dim3(256), 0, c->stream, (const fe_t*)d_taus, (int)ell, (int)first_half, d_eq,
                       (unsigned long long)stride, (unsigned long long)pyr_left);
  }
  for (size_t k = count; k < SP_LOCKSTEP_MAX; ++k) tb.a[k] = tb.b[k] = tb.c[k] = nullptr;

  const uint8_t lbl_c[1] = {'c'};
  spk::LsChallenges ch;
  memset(&ch, 0, sizeof ch);
  std::vector<fe_t> rec(3 * count);
  for (size_t rnd = 1; rnd <= ell; ++rnd) {
    const size_t q = N >> rnd;  // pairs of this round
    spk::LsEq e;
    e.base = d_eq;
    e.stride = stride;
    if (rnd < first_half) {  // poly_eqs_first_half (:1407-1420): q = 2^(first_half - rnd) chunks, one x_out each
      e.off_out = (unsigned)spk::eq_level_offset((int)(first_half - rnd));
      e.off_in = (unsigned)(pyr_left + spk::eq_level_offset((int)second_half));
      e.factored = 1;
    } else {  // poly_eq_right_last_half (:1422-1428): q <= LS_CHUNK
      e.off_out = 0;
      e.off_in = (unsigned)(pyr_left + spk::eq_level_offset((int)(ell - rnd)));
      e.factored = 0;
    }
    const unsigned nb = blocks_per_instance(q);
    spk::LsOut o{d_part, c->d_pinned, next_seq(c)};
    const dim3 grid(nb, (unsigned)count);
    if (rnd == 1) {
      c->timed_kernel("ls_eval_cubic", 192ull * q * count, spk::k_ls_eval_cubic, grid, dim3(256), tb, (unsigned long long)q, e, o);
    } else {
      c->timed_kernel("ls_bind_eval_cubic", 576ull * q * count, spk::k_ls_bind_eval_cubic, grid, dim3(256), tb, ch, (unsigned long long)q, e, o);
      for (size_t k = 0; k < count; ++k)
        for (sp_table* t : {A[k], B[k], C[k]}) sp::after_bind(t);
    }
    if (nb > 1) c->timed_kernel("ls_sum_partials", 96ull * nb * count, spk::k_ls_sum_partials<3>, dim3((unsigned)count), dim3(64), (const fe_t*)d_part, nb, c->d_pinned, o.seq);
    if (rnd > 1) report(observe, user, rnd - 2, ch);
    if ((rc = wait_records(c, count, o.seq, 3, rec.data()))) return rc;
    for (size_t k = 0; k < count; ++k) {
      const fe_t tau = taus[k * ell + rnd - 1];
      const sp::UniPoly poly = sp::cubic3_round_poly(claim[k], p[k], tau, inv_tau[k * ell + rnd - 1], &rec[3 * k]);
      sp::absorb_poly(tr[k]->t, poly);
      fe_t r_i;
      if (!tr[k]->t.squeeze<S>(lbl_c, 1, &r_i)) return fail(SP_ERR_INTERNAL_TRANSCRIPT, "transcript round counter overflow");
      const size_t ri = k * ell + rnd - 1;
      store_fe(out_r + 4 * ri, r_i);
      store_fe(out_cpolys + 12 * ri, poly.c[0]);
      store_fe(out_cpolys + 12 * ri + 4, poly.c[2]);
      store_fe(out_cpolys + 12 * ri + 8, poly.c[3]);
      claim[k] = sp::poly_eval(poly, r_i);
      p[k] = sp::cubic3_next_p(p[k], tau, r_i);
      ch.r[k] = r_i;
    }
  }
  const unsigned seq = next_seq(c);
  hipLaunchKernelGGL((spk::k_ls_bind_last<3>), dim3((unsigned)count), dim3(64), 0, c->stream, tb, ch, (const spk::LsEff*)nullptr, c->d_pinned, seq);
  for (size_t k = 0; k < count; ++k)
    for (sp_table* t : {A[k], B[k], C[k]}) sp::after_bind(t);
  report(observe, user, ell - 1, ch);
  if ((rc = wait_records(c, count, seq, 3, rec.data()))) return rc;
  for (size_t k = 0; k < count; ++k)
    for (int j = 0; j < 3; ++j) store_fe(out_final + 12 * k + 4 * j, rec[3 * k + j]);
  return SP_OK;
}

int sp_sumcheck_cubic3_lockstep(sp_ctx* c, size_t count, const uint64_t* claims, const uint64_t* taus, size_t ell, sp_table* const* A, sp_table* const* B,
                                sp_table* const* C, sp_transcript* const* tr, uint64_t* out_cpolys, uint64_t* out_r, uint64_t* out_final) {
  return sp_sumcheck_cubic3_lockstep_observed(c, count, claims, taus, ell, A, B, C, tr, out_cpolys, out_r, out_final, nullptr, nullptr);
}

int sp_sumcheck_quad_lockstep_observed(sp_ctx* c, size_t count, const uint64_t* claims, size_t rounds, sp_table* const* A, sp_table* const* B, sp_transcript* const* tr,
                                       uint64_t* out_cpolys, uint64_t* out_r, uint64_t* out_final, sp_lockstep_hook observe, void* user) {
  static const char* who = "prove_quad (lockstep)";
  if (!c || !claims || !out_cpolys || !out_r || !out_final) return fail(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": null argument");
  sp_table* const* tabs[2] = {A, B};
  int rc = check_instances(who, count, rounds, tabs, 2, tr);
  if (rc) return rc;
  const size_t N = (size_t)1 << rounds;
  const unsigned nb_max = blocks_per_instance(N / 2);
  fe_t* d_part = static_cast<fe_t*>(c->workspace(sp_ctx::WS_LOCKSTEP_PARTIALS, count * (size_t)nb_max * 3 * sizeof(fe_t)));
  spk::LsEff* d_eff = static_cast<spk::LsEff*>(c->workspace(sp_ctx::WS_LOCKSTEP_PARAMS, rounds * count * sizeof(spk::LsEff)));
  if (!d_part || !d_eff) return SP_ERR_NO_DEVICE;
  for (size_t k = 0; k < count; ++k) tr[k]->join();

  // (lo_eff, hi_eff) of every table in every round follow from the ones at entry (after_bind): uploaded once, in front of the first launch
  std::vector<spk::LsEff> eff(rounds * count);
  for (size_t k = 0; k < count; ++k) {
    sp_table a = *A[k], b = *B[k];
    for (size_t i = 0; i < rounds; ++i) {
      eff[i * count + k] = spk::LsEff{(unsigned)sp::eff_lo(&a), (unsigned)sp::eff_hi(&a), (unsigned)sp::eff_lo(&b), (unsigned)sp::eff_hi(&b)};
      sp::after_bind(&a);
      sp::after_bind(&b);
    }
  }
  SP_HIP(hipMemcpyAsync(d_eff, eff.data(), eff.size() * sizeof(spk::LsEff), hipMemcpyHostToDevice, c->stream));

  std::vector<fe_t> claim(count);
  spk::LsTables2 tb;
  spk::LsTables3 tb3;
  for (size_t k = 0; k < SP_LOCKSTEP_MAX; ++k) {
    tb.a[k] = tb3.a[k] = k < count ? A[k]->d : nullptr;
    tb.b[k] = tb3.b[k] = k < count ? B[k]->d : nullptr;
    tb3.c[k] = nullptr;
    if (k < count) claim[k] = load_fe(claims + 4 * k);
  }
  const uint8_t lbl_c[1] = {'c'};
  spk::LsChallenges ch;
  memset(&ch, 0, sizeof ch);
  std::vector<fe_t> rec(3 * count);
  for (size_t round = 0; round < rounds; ++round) {
    const size_t q = N >> (round + 1);  // pairs of this round
    const unsigned nb = blocks_per_instance(q);
    spk::LsOut o{d_part, c->d_pinned, next_seq(c)};
    const dim3 grid(nb, (unsigned)count);
    if (round == 0) {
      c->timed_kernel("ls_eval_quad", 128ull * q * count, spk::k_ls_eval_quad, grid, dim3(256), tb, (unsigned long long)q, (const spk::LsEff*)d_eff, o);
    } else {
      c->timed_kernel("ls_bind_eval_quad", 384ull * q * count, spk::k_ls_bind_eval_quad, grid, dim3(256), tb, ch, (unsigned long long)q,
                      (const spk::LsEff*)(d_eff + (round - 1) * count), o);
      for (size_t k = 0; k < count; ++k) {
        sp::after_bind(A[k]);
        sp::after_bind(B[k]);
      }
    }
    if (nb > 1) c->timed_kernel("ls_sum_partials", 64ull * nb * count, spk::k_ls_sum_partials<2>, dim3((unsigned)count), dim3(64), (const fe_t*)d_part, nb, c->d_pinned, o.seq);
    if (round > 0) report(observe, user, round - 1, ch);
    if ((rc = wait_records(c, count, o.seq, 2, rec.data()))) return rc;
    for (size_t k = 0; k < count; ++k) {
      const sp::UniPoly poly = sp::quad_round_poly(claim[k], &rec[3 * k]);
      sp::absorb_poly(tr[k]->t, poly);
      fe_t r_i;
      if (!tr[k]->t.squeeze<S>(lbl_c, 1, &r_i)) return fail(SP_ERR_INTERNAL_TRANSCRIPT, "transcript round counter overflow");
      const size_t ri = k * rounds + round;
      store_fe(out_r + 4 * ri, r_i);
      store_fe(out_cpolys + 8 * ri, poly.c[0]);
      store_fe(out_cpolys + 8 * ri + 4, poly.c[2]);
      claim[k] = sp::poly_eval(poly, r_i);
      ch.r[k] = r_i;
    }
  }
  const unsigned seq = next_seq(c);
  hipLaunchKernelGGL((spk::k_ls_bind_last<2>), dim3((unsigned)count), dim3(64), 0, c->stream, tb3, ch, (const spk::LsEff*)(d_eff + (rounds - 1) * count), c->d_pinned, seq);
  for (size_t k = 0; k < count; ++k) {
    sp::after_bind(A[k]);
    sp::after_bind(B[k]);
  }
  report(observe, user, rounds - 1, ch);
  if ((rc = wait_records(c, count, seq, 2, rec.data()))) return rc;
  for (size_t k = 0; k < count; ++k)
    for (int j = 0; j < 2; ++j) store_fe(out_final + 8 * k + 4 * j, rec[3 * k + j]);
  return SP_OK;
}

int sp_sumcheck_quad_lockstep(sp_ctx* c, size_t count, const uint64_t* claims, size_t rounds, sp_table* const* A, sp_table* const* B, sp_transcript* const* tr,
                              uint64_t* out_cpolys, uint64_t* out_r, uint64_t* out_final) {
  return sp_sumcheck_quad_lockstep_observed(c, count, claims, rounds, A, B, tr, out_cpolys, out_r, out_final, nullptr, nullptr);
}

}  // extern "C"
