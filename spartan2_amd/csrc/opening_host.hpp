// Host arithmetic of the lone opening (capi_opening.hip) over field.hpp alone, checked on the CPU by tests/native/opening_fold_check.hip.
#pragma once
#include <cstring>
#include <vector>

#include "field.hpp"

namespace sp {
namespace host {
// one level of eq expansion (eq.rs:66-76): Q[2 i] = P[i] (1 - r), Q[2 i + 1] = P[i] r, the new variable on the index LSB; entries from `nq` on are not
// formed. Walks downwards, so Q may be P itself.
template <class F>
inline void eq_expand(const fe_t* P, size_t np, const fe_t& r, fe_t* Q, size_t nq = ~(size_t)0) {
  for (size_t i = np; i-- > 0;) {
    const fe_t hi = fe_mul<F>(P[i], r);
    if (2 * i < nq) Q[2 * i] = fe_sub<F>(P[i], hi);
    if (2 * i + 1 < nq) Q[2 * i + 1] = hi;
  }
}
// eq table of k variables, r[0] on the index MSB (EqPolynomial::evals_from_points, src/polys/eq.rs:59-93): 2^k elements
template <class F>
inline void eq_table(const fe_t* r, size_t k, fe_t* out) {
  out[0] = fe_one<F>();
  for (size_t j = 0; j < k; ++j) eq_expand<F>(out, (size_t)1 << j, r[j], out);
}
// v folded by its top variable: v[j] <- v[j] + r (v[j + h] - v[j]) for the lower half, the upper half wiped and dropped. Folding by r_0 .. r_(k-1)
// leaves <eq(r), v> (the multilinear extension of v at r)
template <class F>
inline void fold_top(std::vector<fe_t>& v, const fe_t& r) {
  const size_t h = v.size() / 2;
  for (size_t j = 0; j < h; ++j) v[j] = fe_add<F>(v[j], fe_mul<F>(r, fe_sub<F>(v[j + h], v[j])));
  explicit_bzero(v.data() + h, h * sizeof(fe_t));
  v.resize(h);
}
// <eq(point), d> in tensor form, eq(point) = left (x) right with left = eq of the first hb variables: T[b] = sum_a left[a] d[a * |T| + b] needs the
// first half of the point only; <right, T> closes it (|d| + |T| products instead of 2 |d|)
template <class F>
inline void tensor_partial_sums(const fe_t* point, size_t hb, const fe_t* d, size_t nd, std::vector<fe_t>& T) {
  const size_t nleft = (size_t)1 << hb, nright = nd >> hb;
  std::vector<fe_t> left(nleft);
  eq_table<F>(point, hb, left.data());
  T.assign(nright, fe_zero());
  for (size_t a = 0; a < nleft; ++a)
    for (size_t b = 0; b < nright; ++b) T[b] = fe_add<F>(T[b], fe_mul<F>(left[a], d[a * nright + b]));
}
template <class F>
inline fe_t tensor_close(const fe_t* point_right, size_t kb, const fe_t* T) {
  std::vector<fe_t> right((size_t)1 << kb);
  eq_table<F>(point_right, kb, right.data());
  fe_t ip = fe_zero();
  for (size_t b = 0; b < right.size(); ++b) ip = fe_add<F>(ip, fe_mul<F>(right[b], T[b]));
  return ip;
}
// the same inner product row by row, for a caller that has the whole point at once: no vector of partial sums, every row's sum stays in registers
template <class F>
inline fe_t tensor_inner_product(const fe_t* point, size_t k, const fe_t* d) {
  const size_t hb = k / 2;
  std::vector<fe_t> left((size_t)1 << hb), right((size_t)1 << (k - hb));
  eq_table<F>(point, hb, left.data());
  eq_table<F>(point + hb, k - hb, right.data());
  fe_t ip = fe_zero();
  for (size_t a = 0; a < left.size(); ++a) {
    fe_t inner = fe_zero();
    for (size_t b = 0; b < right.size(); ++b) inner = fe_add<F>(inner, fe_mul<F>(right[b], d[a * right.size() + b]));
    ip = fe_add<F>(ip, fe_mul<F>(left[a], inner));
  }
  return ip;
}
}  // namespace host
}  // namespace sp
