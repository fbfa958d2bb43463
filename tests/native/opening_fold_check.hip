// The host arithmetic of the lone opening (spartan2_amd/csrc/opening_host.hpp) against the definitions it shortens, over the scalar field with seeded
// inputs: the fold by the top variable, the level-by-level eq expansion, the tensor form of <R, d>. Host code only; nothing is launched.
// Usage: opening_fold_check <trials>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../spartan2_amd/csrc/opening_host.hpp"

typedef FqP F;
namespace oh = sp::host;

static unsigned long long g_st = 0x9E3779B97F4A7C15ull;
static fe_t rnd_fe() {
  fe_t v;
  for (int i = 0; i < 8; ++i) {
    g_st ^= g_st << 13;
    g_st ^= g_st >> 7;
    g_st ^= g_st << 17;
    v.v[i] = (uint32_t)(g_st >> 16);
  }
  v = fe_add<F>(v, fe_zero());  // into [0, p): two conditional subtractions cover any 256-bit pattern (p > 2^255)
  return fe_add<F>(v, fe_zero());
}
static std::vector<fe_t> rnd_vec(size_t n) {
  std::vector<fe_t> v(n);
  for (fe_t& x : v) x = rnd_fe();
  return v;
}
static bool same(const fe_t& a, const fe_t& b) { return memcmp(&a, &b, sizeof(fe_t)) == 0; }
// eq(r, i) from its definition: the product over the variables of r_j or 1 - r_j, r[0] on the index MSB
static fe_t eq_at(const std::vector<fe_t>& r, size_t i) {
  fe_t e = fe_one<F>();
  for (size_t j = 0; j < r.size(); ++j) e = fe_mul<F>(e, ((i >> (r.size() - 1 - j)) & 1) ? r[j] : fe_sub<F>(fe_one<F>(), r[j]));
  return e;
}
static fe_t dot_eq(const std::vector<fe_t>& r, const std::vector<fe_t>& v) {
  fe_t acc = fe_zero();
  for (size_t i = 0; i < v.size(); ++i) acc = fe_add<F>(acc, fe_mul<F>(eq_at(r, i), v[i]));
  return acc;
}

// folding by r_0 .. r_(k-1) leaves <eq(r), v>; every fold halves the vector
static int check_fold(size_t k) {
  const std::vector<fe_t> r = rnd_vec(k), v = rnd_vec((size_t)1 << k);
  std::vector<fe_t> f = v;
  int bad = 0;
  for (size_t j = 0; j < k; ++j) {
    oh::fold_top<F>(f, r[j]);
    bad += f.size() != v.size() >> (j + 1);
  }
  return bad + !(f.size() == 1 && same(f[0], dot_eq(r, v)));
}
// expanding level by level gives the eq table, and so does the last level formed as (P[i] - P[i] r, P[i] r) from the table one variable short
static int check_expand(size_t k) {
  const std::vector<fe_t> r = rnd_vec(k);
  std::vector<fe_t> table((size_t)1 << k), P(1, fe_one<F>());
  oh::eq_table<F>(r.data(), k, table.data());
  int bad = 0;
  for (size_t j = 0; j < k; ++j) {
    std::vector<fe_t> Q(2 * P.size());
    oh::eq_expand<F>(P.data(), P.size(), r[j], Q.data());
    if (j + 1 == k)
      for (size_t i = 0; i < P.size(); ++i) {
        const fe_t hi = fe_mul<F>(P[i], r[j]);
        bad += !same(Q[2 * i], fe_sub<F>(P[i], hi)) || !same(Q[2 * i + 1], hi);
      }
    P.swap(Q);
  }
  for (size_t i = 0; i < table.size(); ++i) bad += !same(table[i], eq_at(r, i)) || !same(P[i], table[i]);
  // the bounded form leaves what lies behind its bound alone
  if (k >= 1) {
    std::vector<fe_t> prev((size_t)1 << (k - 1)), Q(table.size(), fe_zero());
    oh::eq_table<F>(r.data(), k - 1, prev.data());
    const size_t nq = table.size() - 1;
    oh::eq_expand<F>(prev.data(), prev.size(), r[k - 1], Q.data(), nq);
    for (size_t i = 0; i < table.size(); ++i) bad += !same(Q[i], i < nq ? table[i] : fe_zero());
  }
  return bad;
}
// the partial sums over the first half of the column variables, closed by <right, T>, are the direct <eq(point), d>, and so is the row-by-row form
static int check_tensor(size_t k) {
  const std::vector<fe_t> pt = rnd_vec(k), d = rnd_vec((size_t)1 << k);
  const size_t hb = k / 2;
  std::vector<fe_t> T;
  oh::tensor_partial_sums<F>(pt.data(), hb, d.data(), d.size(), T);
  const fe_t ip = oh::tensor_close<F>(pt.data() + hb, k - hb, T.data());
  return !(T.size() == d.size() >> hb && same(ip, dot_eq(pt, d)) && same(oh::tensor_inner_product<F>(pt.data(), k, d.data()), ip));
}

int main(int argc, char** argv) {
  const int trials = argc > 1 ? atoi(argv[1]) : 20;
  int bad_fold = 0, bad_expand = 0, bad_tensor = 0;
  for (int t = 0; t < trials; ++t) {
    for (size_t k = 1; k <= 6; ++k) bad_fold += check_fold(k);
    for (size_t k = 0; k <= 6; ++k) bad_expand += check_expand(k);
    for (size_t k : {0, 1, 5}) bad_tensor += check_tensor(k);  // hb = 0, 0, 2
  }
  printf("fold_top: %d trials, %d mismatches\n", trials, bad_fold);
  printf("eq_expand: %d trials, %d mismatches\n", trials, bad_expand);
  printf("tensor: %d trials, %d mismatches\n", trials, bad_tensor);
  return bad_fold || bad_expand || bad_tensor ? 1 : 0;
}
