// The host's O(1) share of a sum-check round, shared by the host-table provers of capi_core.hip and the lockstep provers of capi_lockstep.hip:
// UniPoly (src/polys/univariate.rs), its transcript encoding, and the round polynomials of prove_cubic_with_three_inputs and prove_quad from the
// round's device sums.
#pragma once
#include "field.hpp"
#include "keccak.hpp"

namespace sp {

struct UniPoly {
  fe_t c[4];
  int n;
};
inline fe_t two_inv() {
  static const fe_t v = fe_inv_vartime<FqP>(fe_from_u64<FqP>(2));
  return v;
}
inline fe_t poly_eval(const UniPoly& p, const fe_t& r) {  // univariate.rs:136-144
  fe_t ev = p.c[0], pw = r;
  for (int i = 1; i < p.n; ++i) {
    ev = fe_add<FqP>(ev, fe_mul<FqP>(pw, p.c[i]));
    pw = fe_mul<FqP>(pw, r);
  }
  return ev;
}
// UniPoly::from_evals of the batched ZK sum-checks (prove_quad_batched_zk, prove_cubic_with_additive_term_batched_zk): evaluations at 0, 1, 2 (, 3)
inline fe_t six_inv() {
  static const fe_t v = fe_inv_vartime<FqP>(fe_from_u64<FqP>(6));
  return v;
}
inline UniPoly from_evals_deg2(const fe_t e[3]) {  // univariate.rs:84-93
  UniPoly p;
  p.n = 3;
  fe_t c0 = e[0];
  fe_t a = fe_mul<FqP>(fe_add<FqP>(fe_sub<FqP>(e[0], fe_dbl<FqP>(e[1])), e[2]), two_inv());
  fe_t b = fe_sub<FqP>(fe_sub<FqP>(e[1], c0), a);
  p.c[0] = c0;
  p.c[1] = b;
  p.c[2] = a;
  return p;
}
inline UniPoly from_evals_deg3(const fe_t e[4]) {  // univariate.rs:102-118
  UniPoly p;
  p.n = 4;
  fe_t d = e[0];
  fe_t e1_3 = fe_add<FqP>(fe_dbl<FqP>(e[1]), e[1]), e2_3 = fe_add<FqP>(fe_dbl<FqP>(e[2]), e[2]);
  fe_t delta3 = fe_sub<FqP>(fe_add<FqP>(fe_sub<FqP>(e[3], e2_3), e1_3), e[0]);
  fe_t a = fe_mul<FqP>(delta3, six_inv());
  fe_t delta2 = fe_add<FqP>(fe_sub<FqP>(e[2], fe_dbl<FqP>(e[1])), e[0]);
  fe_t b = fe_sub<FqP>(fe_mul<FqP>(delta2, two_inv()), fe_add<FqP>(fe_dbl<FqP>(a), a));
  fe_t c1 = fe_sub<FqP>(fe_sub<FqP>(fe_sub<FqP>(e[1], d), b), a);
  p.c[0] = d;
  p.c[1] = c1;
  p.c[2] = b;
  p.c[3] = a;
  return p;
}
// absorb(b"p", &poly): compressed coefficients, to_repr LE each (univariate.rs:182-190)
inline void absorb_poly(Transcript& t, const UniPoly& p) {
  uint8_t buf[32 * 3];
  int k = 0;
  fe_to_le_bytes<FqP>(p.c[0], buf);
  k = 1;
  for (int i = 2; i < p.n; ++i) fe_to_le_bytes<FqP>(p.c[i], buf + 32 * k++);
  const uint8_t lbl[1] = {'p'};
  t.absorb(lbl, 1, buf, 32 * k);
}
// 1 / tau_k for every round by one inversion; zeros stay zero (those rounds take the three-sum form)
inline void batch_inv_taus(const fe_t* taus, size_t ell, fe_t* inv_tau) {
  std::vector<fe_t> pref(ell);
  fe_t run = fe_one<FqP>();
  for (size_t i = 0; i < ell; ++i) {
    pref[i] = run;
    inv_tau[i] = fe_zero();
    if (!fe_is_zero(taus[i])) run = fe_mul<FqP>(run, taus[i]);
  }
  fe_t inv = fe_inv_vartime<FqP>(run);
  for (size_t i = ell; i-- > 0;) {
    if (fe_is_zero(taus[i])) continue;
    inv_tau[i] = fe_mul<FqP>(inv, pref[i]);
    inv = fe_mul<FqP>(inv, taus[i]);
  }
}
// The round polynomial of prove_cubic_with_three_inputs from sums = {t0, t_inf, t(-1)} of the round's eq-weighted pairs; p = the product of the
// earlier rounds' eq(tau_j, r_j). derive_from_claim (src/sumcheck.rs:1276-1324: the division by l(1) p = tau p through 1 / tau) or, when tau p = 0,
// fallback_three_inputs (:1327-1396), which is the only reader of sums[2].
inline UniPoly cubic3_round_poly(const fe_t& claim, const fe_t& p, const fe_t& tau, const fe_t& inv_tau, const fe_t sums[3]) {
  const fe_t one = fe_one<FqP>();
  const fe_t eq0 = fe_sub<FqP>(one, tau), slope = fe_sub<FqP>(tau, eq0), eqm1 = fe_sub<FqP>(eq0, slope);
  const fe_t t0 = sums[0], tinf = sums[1];
  const fe_t l_1_p = fe_mul<FqP>(fe_add<FqP>(eq0, slope), p);
  const fe_t s_0 = fe_mul<FqP>(fe_mul<FqP>(eq0, p), t0);
  const fe_t s_1 = fe_sub<FqP>(claim, s_0);
  const fe_t s_leading = fe_mul<FqP>(fe_mul<FqP>(slope, p), tinf);
  fe_t s_m1;
  if (!fe_is_zero(l_1_p)) {
    const fe_t two_sum = fe_add<FqP>(fe_dbl<FqP>(tinf), fe_dbl<FqP>(t0));
    s_m1 = fe_mul<FqP>(eqm1, fe_sub<FqP>(fe_mul<FqP>(p, two_sum), fe_mul<FqP>(s_1, inv_tau)));
  } else {
    s_m1 = fe_mul<FqP>(fe_mul<FqP>(eqm1, p), sums[2]);
  }
  const fe_t halfc = two_inv();
  UniPoly poly;
  poly.n = 4;
  poly.c[0] = s_0;
  poly.c[1] = fe_sub<FqP>(fe_mul<FqP>(fe_sub<FqP>(s_1, s_m1), halfc), s_leading);
  poly.c[2] = fe_sub<FqP>(fe_mul<FqP>(fe_add<FqP>(s_1, s_m1), halfc), s_0);
  poly.c[3] = s_leading;
  return poly;
}
// p after the round's challenge: p * eq(tau, r)
inline fe_t cubic3_next_p(const fe_t& p, const fe_t& tau, const fe_t& r) {
  return fe_mul<FqP>(p, fe_add<FqP>(fe_sub<FqP>(fe_sub<FqP>(fe_one<FqP>(), tau), r), fe_dbl<FqP>(fe_mul<FqP>(r, tau))));
}
// prove_quad's round polynomial from sums = {eval_0, t_inf}. BDDT: eval_2 = 2 claim - 3 eval_0 + 2 t_inf and its interpolation
// (src/sumcheck.rs:211-215, univariate.rs:84-93): c0 = eval_0, c2 = t_inf, c1 = claim - 2 eval_0 - t_inf
inline UniPoly quad_round_poly(const fe_t& claim, const fe_t sums[2]) {
  UniPoly poly;
  poly.n = 3;
  poly.c[0] = sums[0];
  poly.c[1] = fe_sub<FqP>(fe_sub<FqP>(claim, fe_dbl<FqP>(sums[0])), sums[1]);
  poly.c[2] = sums[1];
  return poly;
}

}  // namespace sp
