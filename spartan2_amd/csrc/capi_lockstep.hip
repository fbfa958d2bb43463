// Lockstep sum-checks (include/spartan_hip.h, "many sum-checks of one length in lockstep"): `count` independent instances of
// prove_cubic_with_three_inputs / prove_quad over `count` table sets of one length. One launch computes round i of every instance
// (kernels_lockstep.hpp), one wait collects the `count` records, the host finishes `count` round polynomials (sumcheck_round.hpp: the algebra of the
// host-table provers), feeds each to its own transcript and hands the `count` challenges to the next launch by value. A round trip per round, as for
// a lone instance - shared by all of them. Every instance's polynomials, challenges, final claims and transcript are those of sp_sumcheck_cubic3 /
// sp_sumcheck_quad on that instance alone. The _observed forms report each round's challenges to a hook of the caller once the next launch is queued.
// The _batched_lockstep forms are the two batched ZK sum-checks of NeutronNova (sp_sumcheck_cubic_outer_pow_batched, sp_sumcheck_quad_batched) for `count`
// (step, core) pairs: instance 2p + b of a launch is branch b of pair p, the round polynomials go to the pair's round hook, which answers with the pair's
// challenge. Nothing is queued ahead of a hook and nothing waits on a mailbox, so a hook may use the context (not for a lockstep sum-check of its own: the
// per-round table of effective lengths sits in the context's lockstep workspace for the length of the call).
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
static_assert(SP_LOCKSTEP_PAIRS_MAX == spk::LS_PAIRS_MAX, "a pair is two instances of a launch");

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
// the refusals of the _batched_lockstep forms, in the same style: `ntab` arrays of tables 2^vars long, then (npow = 2) the pairs' power tables
int check_pairs(const char* who, size_t count, size_t vars, const sp_table* const* const* tabs, int ntab, int npow, const void* hook, void* const* users) {
  const std::string w(who);
  if (count == 0 || count > SP_LOCKSTEP_PAIRS_MAX) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": count must be 1 .. SP_LOCKSTEP_PAIRS_MAX");
  if (!hook) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null hook");
  if (!users) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null argument");
  const int all = ntab + npow;
  for (int t = 0; t < all; ++t)
    if (!tabs[t]) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null argument");
  for (size_t p = 0; p < count; ++p)
    for (int t = 0; t < all; ++t)
      if (!tabs[t][p] || !tabs[t][p]->d) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": null table, pair " + std::to_string(p));
  if (vars == 0 || vars > 30) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": tables must have 2^num_rounds elements");
  const size_t n = (size_t)1 << vars;
  for (size_t p = 0; p < count; ++p) {
    for (int t = 0; t < ntab; ++t)
      if (tabs[t][p]->len != n) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": tables must have 2^num_rounds elements, pair " + std::to_string(p));
    if (npow) {
      const size_t left = tabs[ntab][p]->len, right = tabs[ntab + 1][p]->len;
      if (left == 0 || right == 0 || left * right != n) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": pow tables must factor 2^num_rounds, pair " + std::to_string(p));
      if (left != tabs[ntab][0]->len) return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": pow tables of another split than pair 0's, pair " + std::to_string(p));
    }
  }
  for (size_t p = 0; p < count; ++p)
    for (int t = 0; t < all; ++t)
      for (size_t j = 0; j <= p; ++j)
        for (int u = 0; u < all; ++u) {
          if (j == p && u >= t) break;
          if (tabs[u][j] == tabs[t][p] || tabs[u][j]->d == tabs[t][p]->d)
            return fail(SP_ERR_INVALID_INPUT_LENGTH, w + ": the same table twice, pairs " + std::to_string(j) + " and " + std::to_string(p));
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

// prove_cubic_with_additive_term_batched_zk (src/sumcheck.rs:786-917) of `count` pairs, a launch a round (see the head of this file)
int sp_sumcheck_cubic_outer_pow_batched_lockstep(sp_ctx* c, size_t count, size_t num_rounds, sp_table* const* pow_left, const sp_table* const* pow_right,
                                                 sp_table* const* A_step, sp_table* const* B_step, sp_table* const* C_step, sp_table* const* A_core, sp_table* const* B_core,
                                                 sp_table* const* C_core, const uint64_t* t_out_step, size_t start_round, sp_round_hook hook, void* const* users, uint64_t* out_r) {
  static const char* who = "prove_cubic_batched (lockstep)";
  if (!c || !t_out_step || !out_r) return fail(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": null argument");
  const sp_table* const* tabs[8] = {A_step, B_step, C_step, A_core, B_core, C_core, pow_left, pow_right};
  int rc = check_pairs(who, count, num_rounds, tabs, 6, 2, (const void*)hook, users);
  if (rc) return rc;
  const size_t n = (size_t)1 << num_rounds, left = pow_left[0]->len, right = pow_right[0]->len, inst = 2 * count;
  unsigned lg_left = 0;
  while (((size_t)1 << lg_left) < left) ++lg_left;
  fe_t* d_part = static_cast<fe_t*>(c->workspace(sp_ctx::WS_LOCKSTEP_PARTIALS, inst * (size_t)blocks_per_instance(n / 2) * 3 * sizeof(fe_t)));
  if (!d_part) return SP_ERR_NO_DEVICE;
  std::vector<fe_t> pl(count * left), pr(count * right);
  for (size_t p = 0; p < count; ++p) {
    if ((rc = sp_table_read(c, pow_left[p], 0, left, reinterpret_cast<uint64_t*>(&pl[p * left])))) return rc;
    if ((rc = sp_table_read(c, pow_right[p], 0, right, reinterpret_cast<uint64_t*>(&pr[p * right])))) return rc;
  }
  const fe_t one = fe_one<S>();
  std::vector<fe_t> base_tau(count, one), claim(inst, fe_zero()), rec(3 * inst);
  std::vector<sp::UniPoly> poly(inst);
  spk::LsTables3 tb;
  spk::LsPow pw;
  for (size_t p = 0; p < SP_LOCKSTEP_PAIRS_MAX; ++p) {
    const bool on = p < count;
    tb.a[2 * p] = on ? A_step[p]->d : nullptr, tb.a[2 * p + 1] = on ? A_core[p]->d : nullptr;
    tb.b[2 * p] = on ? B_step[p]->d : nullptr, tb.b[2 * p + 1] = on ? B_core[p]->d : nullptr;
    tb.c[2 * p] = on ? C_step[p]->d : nullptr, tb.c[2 * p + 1] = on ? C_core[p]->d : nullptr;
    pw.pl[p] = on ? pow_left[p]->d : nullptr;
    pw.pr[p] = on ? pow_right[p]->d : nullptr;
    if (on) claim[2 * p] = load_fe(t_out_step + 4 * p);
  }
  auto bound = [&] {
    for (size_t p = 0; p < count; ++p)
      for (sp_table* t : {A_step[p], B_step[p], C_step[p], A_core[p], B_core[p], C_core[p]}) sp::after_bind(t);
  };
  spk::LsPairChallenges ch;
  memset(&ch, 0, sizeof ch);
  for (size_t i = 0; i < num_rounds; ++i) {
    const size_t q = n >> (i + 1);  // pairs of this round
    const bool fallback = q < left;
    const unsigned nb = blocks_per_instance(q);
    spk::LsOut o{d_part, c->d_pinned, next_seq(c)};
    const dim3 grid(nb, (unsigned)inst);
    if (i == 0) {
      if (fallback) c->timed_kernel("ls_eval_cubic_pow", 224ull * q * inst, spk::k_ls_eval_cubic_pow<true>, grid, dim3(256), tb, pw, (unsigned long long)q, lg_left, o);
      else c->timed_kernel("ls_eval_cubic_pow", 224ull * q * inst, spk::k_ls_eval_cubic_pow<false>, grid, dim3(256), tb, pw, (unsigned long long)q, lg_left, o);
    } else {
      if (fallback) c->timed_kernel("ls_bind_eval_cubic_pow", 608ull * q * inst, spk::k_ls_bind_eval_cubic_pow<true>, grid, dim3(256), tb, pw, ch, (unsigned long long)q, lg_left, o);
      else c->timed_kernel("ls_bind_eval_cubic_pow", 608ull * q * inst, spk::k_ls_bind_eval_cubic_pow<false>, grid, dim3(256), tb, pw, ch, (unsigned long long)q, lg_left, o);
      bound();
    }
    if (nb > 1) c->timed_kernel("ls_sum_partials", 96ull * nb * inst, spk::k_ls_sum_partials<3>, dim3((unsigned)inst), dim3(64), (const fe_t*)d_part, nb, c->d_pinned, o.seq);
    if ((rc = wait_records(c, inst, o.seq, 3, rec.data()))) return rc;
    for (size_t k = 0; k < inst; ++k) {  // the sums at 0, 2, 3 carry base_tau; the value at 1 follows from the claim (:846-861)
      const fe_t bt = base_tau[k / 2], e0 = fe_mul<S>(rec[3 * k], bt);
      const fe_t ev[4] = {e0, fe_sub<S>(claim[k], e0), fe_mul<S>(rec[3 * k + 1], bt), fe_mul<S>(rec[3 * k + 2], bt)};
      poly[k] = sp::from_evals_deg3(ev);
    }
    for (size_t p = 0; p < count; ++p) {
      uint64_t co[2][16], r_raw[4];
      for (int b = 0; b < 2; ++b)
        for (int j = 0; j < 4; ++j) store_fe(co[b] + 4 * j, poly[2 * p + b].c[j]);
      const int hrc = hook(users[p], start_round + i, co[0], co[1], 4, r_raw);
      if (hrc) return fail(hrc, std::string(who) + ": the round hook failed, pair " + std::to_string(p));
      const fe_t r_i = load_fe(r_raw);
      store_fe(out_r + 4 * (p * num_rounds + i), r_i);
      claim[2 * p] = sp::poly_eval(poly[2 * p], r_i);
      claim[2 * p + 1] = sp::poly_eval(poly[2 * p + 1], r_i);
      ch.r[p] = r_i;
      const fe_t w = fe_mul<S>(pl[p * left + q % left], pr[p * right + q / left]);  // pow_tau[len / 2] (:905-911)
      base_tau[p] = fe_mul<S>(base_tau[p], fe_add<S>(fe_mul<S>(fe_sub<S>(w, one), r_i), one));
    }
  }
  spk::LsChallenges last;
  memset(&last, 0, sizeof last);
  for (size_t p = 0; p < count; ++p) last.r[2 * p] = last.r[2 * p + 1] = ch.r[p];
  const unsigned seq = next_seq(c);
  hipLaunchKernelGGL((spk::k_ls_bind_last<3>), dim3((unsigned)inst), dim3(64), 0, c->stream, tb, last, (const spk::LsEff*)nullptr, c->d_pinned, seq);
  bound();
  if ((rc = wait_records(c, inst, seq, 3, rec.data()))) return rc;  // the final claims: element 0 of every table is in place
  for (size_t p = 0; p < count; ++p)
    if ((rc = sp_table_write(c, pow_left[p], 0, reinterpret_cast<const uint64_t*>(&base_tau[p]), 1))) return rc;
  return SP_OK;
}

// prove_quad_batched_zk (src/sumcheck.rs:702-782) of `count` pairs: the kernels of sp_sumcheck_quad_lockstep, a hook instead of a transcript
int sp_sumcheck_quad_batched_lockstep(sp_ctx* c, size_t count, const uint64_t* claims, size_t num_rounds, sp_table* const* A0, sp_table* const* A1, sp_table* const* B0,
                                      sp_table* const* B1, size_t start_round, sp_round_hook hook, void* const* users, uint64_t* out_r, uint64_t* out_final) {
  static const char* who = "prove_quad_batched (lockstep)";
  if (!c || !claims || !out_r || !out_final) return fail(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": null argument");
  const sp_table* const* tabs[4] = {A0, A1, B0, B1};
  int rc = check_pairs(who, count, num_rounds, tabs, 4, 0, (const void*)hook, users);
  if (rc) return rc;
  const size_t n = (size_t)1 << num_rounds, inst = 2 * count;
  fe_t* d_part = static_cast<fe_t*>(c->workspace(sp_ctx::WS_LOCKSTEP_PARTIALS, inst * (size_t)blocks_per_instance(n / 2) * 3 * sizeof(fe_t)));
  spk::LsEff* d_eff = static_cast<spk::LsEff*>(c->workspace(sp_ctx::WS_LOCKSTEP_PARAMS, num_rounds * inst * sizeof(spk::LsEff)));
  if (!d_part || !d_eff) return SP_ERR_NO_DEVICE;
  auto A = [&](size_t k) { return (k & 1 ? A1 : A0)[k / 2]; };
  auto B = [&](size_t k) { return (k & 1 ? B1 : B0)[k / 2]; };
  // (lo_eff, hi_eff) of every table in every round, as sp_sumcheck_quad_lockstep_observed: uploaded once, in front of the first launch
  std::vector<spk::LsEff> eff(num_rounds * inst);
  for (size_t k = 0; k < inst; ++k) {
    sp_table a = *A(k), b = *B(k);
    for (size_t i = 0; i < num_rounds; ++i) {
      eff[i * inst + k] = spk::LsEff{(unsigned)sp::eff_lo(&a), (unsigned)sp::eff_hi(&a), (unsigned)sp::eff_lo(&b), (unsigned)sp::eff_hi(&b)};
      sp::after_bind(&a);
      sp::after_bind(&b);
    }
  }
  SP_HIP(hipMemcpyAsync(d_eff, eff.data(), eff.size() * sizeof(spk::LsEff), hipMemcpyHostToDevice, c->stream));

  std::vector<fe_t> claim(inst), rec(3 * inst);
  std::vector<sp::UniPoly> poly(inst);
  spk::LsTables2 tb;
  spk::LsTables3 tb3;
  for (size_t k = 0; k < SP_LOCKSTEP_MAX; ++k) {
    tb.a[k] = tb3.a[k] = k < inst ? A(k)->d : nullptr;
    tb.b[k] = tb3.b[k] = k < inst ? B(k)->d : nullptr;
    tb3.c[k] = nullptr;
    if (k < inst) claim[k] = load_fe(claims + 4 * k);  // claims: {step, core} of pair 0, of pair 1, ...
  }
  auto bound = [&] {
    for (size_t k = 0; k < inst; ++k) {
      sp::after_bind(A(k));
      sp::after_bind(B(k));
    }
  };
  spk::LsChallenges ch;
  memset(&ch, 0, sizeof ch);
  for (size_t j = 0; j < num_rounds; ++j) {
    const size_t q = n >> (j + 1);  // pairs of this round
    const unsigned nb = blocks_per_instance(q);
    spk::LsOut o{d_part, c->d_pinned, next_seq(c)};
    const dim3 grid(nb, (unsigned)inst);
    if (j == 0) {
      c->timed_kernel("ls_eval_quad", 128ull * q * inst, spk::k_ls_eval_quad, grid, dim3(256), tb, (unsigned long long)q, (const spk::LsEff*)d_eff, o);
    } else {
      c->timed_kernel("ls_bind_eval_quad", 384ull * q * inst, spk::k_ls_bind_eval_quad, grid, dim3(256), tb, ch, (unsigned long long)q, (const spk::LsEff*)(d_eff + (j - 1) * inst), o);
      bound();
    }
    if (nb > 1) c->timed_kernel("ls_sum_partials", 64ull * nb * inst, spk::k_ls_sum_partials<2>, dim3((unsigned)inst), dim3(64), (const fe_t*)d_part, nb, c->d_pinned, o.seq);
    if ((rc = wait_records(c, inst, o.seq, 2, rec.data()))) return rc;
    for (size_t k = 0; k < inst; ++k) {  // eval_0, eval_1 = claim - eval_0, eval_2 = 2 claim - 3 eval_0 + 2 t_inf (:730-742)
      const fe_t e0 = rec[3 * k], tinf = rec[3 * k + 1], three_e0 = fe_add<S>(fe_add<S>(e0, e0), e0);
      const fe_t ev[3] = {e0, fe_sub<S>(claim[k], e0), fe_add<S>(fe_add<S>(fe_sub<S>(fe_add<S>(claim[k], claim[k]), three_e0), tinf), tinf)};
      poly[k] = sp::from_evals_deg2(ev);
    }
    for (size_t p = 0; p < count; ++p) {
      uint64_t co[2][12], r_raw[4];
      for (int b = 0; b < 2; ++b)
        for (int t = 0; t < 3; ++t) store_fe(co[b] + 4 * t, poly[2 * p + b].c[t]);
      const int hrc = hook(users[p], start_round + j, co[0], co[1], 3, r_raw);
      if (hrc) return fail(hrc, std::string(who) + ": the round hook failed, pair " + std::to_string(p));
      const fe_t r_j = load_fe(r_raw);
      store_fe(out_r + 4 * (p * num_rounds + j), r_j);
      claim[2 * p] = sp::poly_eval(poly[2 * p], r_j);
      claim[2 * p + 1] = sp::poly_eval(poly[2 * p + 1], r_j);
      ch.r[2 * p] = ch.r[2 * p + 1] = r_j;
    }
  }
  const unsigned seq = next_seq(c);
  hipLaunchKernelGGL((spk::k_ls_bind_last<2>), dim3((unsigned)inst), dim3(64), 0, c->stream, tb3, ch, (const spk::LsEff*)(d_eff + (num_rounds - 1) * inst), c->d_pinned, seq);
  bound();
  if ((rc = wait_records(c, inst, seq, 2, rec.data()))) return rc;
  for (size_t p = 0; p < count; ++p) {  // {A0[0], A1[0], B0[0], B1[0]} of pair p
    store_fe(out_final + 16 * p, rec[3 * (2 * p)]);
    store_fe(out_final + 16 * p + 4, rec[3 * (2 * p + 1)]);
    store_fe(out_final + 16 * p + 8, rec[3 * (2 * p) + 1]);
    store_fe(out_final + 16 * p + 12, rec[3 * (2 * p + 1) + 1]);
  }
  return SP_OK;
}

}  // extern "C"
