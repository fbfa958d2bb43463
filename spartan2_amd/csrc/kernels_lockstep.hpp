// HIP kernels of the lockstep sum-checks (gfx950, wave64): K independent sum-check instances over K table sets of one length, one launch per round
// for all of them (capi_lockstep.hip).
//   k_ls_eval_cubic / k_ls_bind_eval_cubic   the round sums of sp_sumcheck_cubic3_host (t0, t_inf and the third sum of the tau p = 0 fallback)
//   k_ls_eval_quad / k_ls_bind_eval_quad     eval_0 and t_inf of prove_quad on tables with (lo_eff, hi_eff)
//   k_ls_eval_cubic_pow / k_ls_bind_eval_cubic_pow   the sums at 0, 2, 3 of the batched NeutronNova outer rounds (split power table), two instances a pair
//   k_ls_eq_levels                           the two eq pyramids of every instance (split eq tables, as k_eq_levels_pair builds them for one)
//   k_ls_sum_partials                        second stage: the block partials of an instance -> its record
//   k_ls_bind_last                           the bind behind the last challenge: element 0 of every table, which is also the final claim
// Every kernel is a plain launch that ends by itself: nothing here waits on host memory, a mailbox or another block. grid = (blocks per instance, K);
// the instance's table pointers and its challenge travel by value (LsTables3 / LsTables2 / LsChallenges, as BindArgs does for its tables).
//
// A block owns LS_CHUNK consecutive pairs of its instance. With one block per instance (<= LS_SINGLE_MAX_PAIRS pairs) the block writes the instance's
// record itself; above that it leaves NACC block partials in device memory and k_ls_sum_partials follows. A record is result slot k of the mapped
// pinned buffer (SLOT_BASE_ELEM + 4 k: three sums and the self-validating tag of slot_store_tag carrying the round's sequence word), which the host
// collects with the bounded wait it uses for every other round result.
//
// The fused kernels bind in place: the thread of pair id reads elements id, id + q, id + 2q, id + 3q of the 4q-long tables, writes the bound elements id
// and id + q and evaluates the pair (id, id + q) of the next round from registers. No other thread of the launch reads or writes those four elements.
#pragma once
#include "kernels_shared.hpp"

namespace spk {

constexpr int LS_MAX = 64;                        // SP_LOCKSTEP_MAX: 3 x 64 pointers + 64 challenges stay below the 4 KiB of a kernel argument
constexpr unsigned LS_CHUNK = 1024;               // pairs per block: four per thread
constexpr unsigned LS_SINGLE_MAX_PAIRS = LS_CHUNK;  // up to here one block per instance does the whole round, no second stage
constexpr int LS_EQ_IN_BITS = 10;                 // log2(LS_CHUNK): variables of the inner (right) eq table of the cubic rounds
static_assert((1u << LS_EQ_IN_BITS) == LS_CHUNK, "a block's chunk is one x_out of the split eq tables");

struct LsTables3 {
  fe_t* a[LS_MAX];
  fe_t* b[LS_MAX];
  fe_t* c[LS_MAX];
};
struct LsTables2 {
  fe_t* a[LS_MAX];
  fe_t* b[LS_MAX];
};
struct LsChallenges {
  fe_t r[LS_MAX];
};
// The split eq tables of one round (EqSumCheckInstance, src/sumcheck.rs:956-1016): every instance has its two pyramids (k_ls_eq_levels) at
// base + k * stride, the right one over the last LS_EQ_IN_BITS taus (all of them up to that many), the left one over the taus in front of those. The
// weight of pair id is in[id & (LS_CHUNK - 1)] * out[id / LS_CHUNK]: a block's chunk is exactly one x_out, so
//   factored = 1 (rounds of more than LS_CHUNK pairs): the block sum is multiplied by out[blockIdx.x] once
//   factored = 0 (one block per instance): weight = in[id], `in` being the right pyramid's level of this round
struct LsEq {
  const fe_t* base;
  unsigned long long stride;
  unsigned off_in, off_out;
  int factored;
};
// Every instance's pair of pyramids (EqSumCheckInstance::new, src/sumcheck.rs:956-992) in one launch: grid = (2, K), block (0, k) the left one over
// taus_k[1 .. first_half), block (1, k) the right one over taus_k[first_half .. ell), at out + k * stride and pyr_left elements behind it. taus: K x ell
// elements in device memory.
__global__ void __launch_bounds__(256) k_ls_eq_levels(const fe_t* __restrict__ taus, int ell, int first_half, fe_t* __restrict__ out, unsigned long long stride,
                                                      unsigned long long pyr_left) {
  __shared__ fe_t lv[EQ_LDS_ENTRIES];
  const fe_t* t = taus + (size_t)blockIdx.y * ell;
  fe_t* o = out + (size_t)blockIdx.y * stride;
  const int nleft = first_half > 0 ? first_half - 1 : 0;
  if (blockIdx.x == 0) eq_levels_block(t + nleft, nleft, o, lv);
  else eq_levels_block(t + (ell - 1), ell - first_half, o + pyr_left, lv);
}

struct LsOut {
  fe_t* partials;  // [instance][block][NACC], read by k_ls_sum_partials
  fe_t* mapped;    // device address of the mapped pinned buffer
  unsigned seq;    // the round's sequence word
};
// min(lo_eff, half) / min(hi_eff, half) of A and of B for every (round, instance): a table's elements from lo on in its low half and from hi on in its
// high half count as zero, whatever memory holds there
struct LsEff {
  unsigned loA, hiA, loB, hiB;
};

template <int NACC>
__device__ __forceinline__ void ls_record(const fe_t (&acc)[NACC], fe_t* __restrict__ mapped, unsigned k, unsigned seq) {
  fe_t* slot = mapped + SLOT_BASE_ELEM + 4 * k;
  slot_chk chk = {0u, 0u};
#pragma unroll
  for (int j = 0; j < NACC; ++j) {
    slot_store_elem(slot + j, acc[j]);
    slot_chk_add(chk, acc[j], j);
  }
  slot_store_tag(slot, seq, chk);
}
template <int NACC>
__device__ __forceinline__ void ls_emit(const fe_t (&acc)[NACC], const LsOut& o) {
  if (gridDim.x == 1) ls_record<NACC>(acc, o.mapped, blockIdx.y, o.seq);
  else {
#pragma unroll
    for (int j = 0; j < NACC; ++j) o.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NACC + j] = acc[j];
  }
}
__device__ __forceinline__ fe_t ls_bind(const fe_t& lo, const fe_t& hi, const fe_t& r) { return fe_add<S>(lo, fe_mul<S>(r, fe_sub<S>(hi, lo))); }

// ---- cubic ---------------------------------------------------------------------------------------------------------------------------------------
// BIND: the tables hold 4q elements and are bound with the instance's challenge first; otherwise they hold 2q. q = pairs of the round evaluated.
template <bool BIND>
__device__ __forceinline__ void ls_cubic_block(fe_t* __restrict__ A, fe_t* __restrict__ B, fe_t* __restrict__ C, unsigned long long q, const fe_t& r, const LsEq& e,
                                               const LsOut& o) {
  __shared__ fe_t smem[3 * 4];
  const fe_t* __restrict__ eq = e.base + (size_t)blockIdx.y * e.stride;
  const fe_t* __restrict__ eq_in = eq + e.off_in;
  const fe_t* __restrict__ eq_out = eq + e.off_out;
  const unsigned long long base = (unsigned long long)blockIdx.x * LS_CHUNK;
  fe_t acc[3] = {fe_zero(), fe_zero(), fe_zero()};
#pragma unroll 1
  for (unsigned j = 0; j < LS_CHUNK / 256; ++j) {
    const unsigned long long id = base + j * 256 + threadIdx.x;
    if (id >= q) break;
    fe_t a0, a1, b0, b1, c0, c1;
    if (BIND) {
      a0 = ls_bind(A[id], A[id + 2 * q], r);
      a1 = ls_bind(A[id + q], A[id + 3 * q], r);
      b0 = ls_bind(B[id], B[id + 2 * q], r);
      b1 = ls_bind(B[id + q], B[id + 3 * q], r);
      c0 = ls_bind(C[id], C[id + 2 * q], r);
      c1 = ls_bind(C[id + q], C[id + 3 * q], r);
      A[id] = a0;
      A[id + q] = a1;
      B[id] = b0;
      B[id + q] = b1;
      C[id] = c0;
      C[id + q] = c1;
    } else {
      a0 = A[id];
      a1 = A[id + q];
      b0 = B[id];
      b1 = B[id + q];
      c0 = C[id];
      c1 = C[id + q];
    }
    const fe_t w = eq_in[id & (LS_CHUNK - 1)];  // (one block per instance: id < LS_CHUNK)
    const fe_t v0 = fe_sub<S>(fe_mul<S>(a0, b0), c0);
    const fe_t v1 = fe_mul<S>(fe_sub<S>(a1, a0), fe_sub<S>(b1, b0));
    const fe_t v2 = fe_sub<S>(fe_mul<S>(fe_sub<S>(fe_dbl<S>(a0), a1), fe_sub<S>(fe_dbl<S>(b0), b1)), fe_sub<S>(fe_dbl<S>(c0), c1));
    acc[0] = fe_add<S>(acc[0], fe_mul<S>(w, v0));
    acc[1] = fe_add<S>(acc[1], fe_mul<S>(w, v1));
    acc[2] = fe_add<S>(acc[2], fe_mul<S>(w, v2));
  }
  block_sum<3>(acc, smem);
  if (threadIdx.x == 0) {
    if (e.factored) {
      const fe_t eo = eq_out[blockIdx.x];
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = fe_mul<S>(acc[j], eo);
    }
    ls_emit<3>(acc, o);
  }
}
__global__ void __launch_bounds__(256) k_ls_eval_cubic(LsTables3 t, unsigned long long q, LsEq e, LsOut o) {
  const unsigned k = blockIdx.y;
  ls_cubic_block<false>(t.a[k], t.b[k], t.c[k], q, fe_zero(), e, o);
}
__global__ void __launch_bounds__(256) k_ls_bind_eval_cubic(LsTables3 t, LsChallenges ch, unsigned long long q, LsEq e, LsOut o) {
  const unsigned k = blockIdx.y;
  ls_cubic_block<true>(t.a[k], t.b[k], t.c[k], q, ch.r[k], e, o);
}

// ---- cubic with the split power table: the batched NeutronNova outer rounds of `count` (step, core) pairs ---------------------------------------------
// Instance 2p + b is branch b (0 = step, 1 = core) of pair p; both branches of a pair share the pair's power tables and its challenge. A round of q pairs
// of elements writes the three sums at 0, 2, 3 of w (A B - C), as k_eval_cubic_outer_pow does for one instance:
//   q >= left                  w_lo = pl[low % left] pr[low / left], w_hi = pl[low % left] pr[low / left + q / left]
//   q <  left (FALLBACK)       w_lo = pl[low], w_hi = pl[low + q]
// left = 2^lg_left is one value for the launch (the pairs' tables have one length and one split). The power tables are read only: base_tau is the host's.
constexpr int LS_PAIRS_MAX = LS_MAX / 2;  // SP_LOCKSTEP_PAIRS_MAX
struct LsPow {
  const fe_t* pl[LS_PAIRS_MAX];
  const fe_t* pr[LS_PAIRS_MAX];
};
struct LsPairChallenges {
  fe_t r[LS_PAIRS_MAX];
};
// the arguments of k_ls_bind_eval_cubic_pow: tables (1536 B), power tables (512 B), ONE challenge a pair (1024 B; LsChallenges' 2048 B would not fit),
// q and lg_left (8 B each with padding), LsOut (24 B) = 3112 B of the 4 KiB argument block
static_assert(sizeof(LsTables3) + sizeof(LsPow) + sizeof(LsPairChallenges) + 2 * sizeof(unsigned long long) + sizeof(LsOut) == 3112,
              "k_ls_bind_eval_cubic_pow: the argument block");
template <bool BIND, bool FALLBACK>
__device__ __forceinline__ void ls_cubic_pow_block(fe_t* __restrict__ A, fe_t* __restrict__ B, fe_t* __restrict__ C, const fe_t* __restrict__ pl,
                                                   const fe_t* __restrict__ pr, unsigned long long q, unsigned lg_left, const fe_t& r, const LsOut& o) {
  __shared__ fe_t smem[3 * 4];
  const unsigned long long base = (unsigned long long)blockIdx.x * LS_CHUNK;
  fe_t acc[3] = {fe_zero(), fe_zero(), fe_zero()};
#pragma unroll 1
  for (unsigned j = 0; j < LS_CHUNK / 256; ++j) {
    const unsigned long long id = base + j * 256 + threadIdx.x;
    if (id >= q) break;
    fe_t al, ah, bl, bh, cl, ch;
    if (BIND) {
      al = ls_bind(A[id], A[id + 2 * q], r);
      ah = ls_bind(A[id + q], A[id + 3 * q], r);
      bl = ls_bind(B[id], B[id + 2 * q], r);
      bh = ls_bind(B[id + q], B[id + 3 * q], r);
      cl = ls_bind(C[id], C[id + 2 * q], r);
      ch = ls_bind(C[id + q], C[id + 3 * q], r);
      A[id] = al;
      A[id + q] = ah;
      B[id] = bl;
      B[id + q] = bh;
      C[id] = cl;
      C[id + q] = ch;
    } else {
      al = A[id];
      ah = A[id + q];
      bl = B[id];
      bh = B[id + q];
      cl = C[id];
      ch = C[id + q];
    }
    fe_t tl, th;
    if (FALLBACK) {
      tl = pl[id];
      th = pl[id + q];
    } else {
      const unsigned long long i = id & ((1ull << lg_left) - 1), jj = id >> lg_left;
      const fe_t p = pl[i];
      tl = fe_mul<S>(p, pr[jj]);
      th = fe_mul<S>(p, pr[jj + (q >> lg_left)]);
    }
    acc[0] = fe_add<S>(acc[0], fe_mul<S>(tl, fe_sub<S>(fe_mul<S>(al, bl), cl)));
    fe_t tb = fe_sub<S>(fe_dbl<S>(th), tl), ab = fe_sub<S>(fe_dbl<S>(ah), al), bb = fe_sub<S>(fe_dbl<S>(bh), bl), cb = fe_sub<S>(fe_dbl<S>(ch), cl);
    acc[1] = fe_add<S>(acc[1], fe_mul<S>(tb, fe_sub<S>(fe_mul<S>(ab, bb), cb)));
    tb = fe_sub<S>(fe_add<S>(tb, th), tl);
    ab = fe_sub<S>(fe_add<S>(ab, ah), al);
    bb = fe_sub<S>(fe_add<S>(bb, bh), bl);
    cb = fe_sub<S>(fe_add<S>(cb, ch), cl);
    acc[2] = fe_add<S>(acc[2], fe_mul<S>(tb, fe_sub<S>(fe_mul<S>(ab, bb), cb)));
  }
  block_sum<3>(acc, smem);
  if (threadIdx.x == 0) ls_emit<3>(acc, o);
}
// grid = (blocks per instance, 2 * pairs); the tables hold 2q elements
template <bool FALLBACK>
__global__ void __launch_bounds__(256) k_ls_eval_cubic_pow(LsTables3 t, LsPow pw, unsigned long long q, unsigned lg_left, LsOut o) {
  const unsigned k = blockIdx.y, p = k >> 1;
  ls_cubic_pow_block<false, FALLBACK>(t.a[k], t.b[k], t.c[k], pw.pl[p], pw.pr[p], q, lg_left, fe_zero(), o);
}
// the tables hold 4q elements and are bound with their pair's challenge first
template <bool FALLBACK>
__global__ void __launch_bounds__(256) k_ls_bind_eval_cubic_pow(LsTables3 t, LsPow pw, LsPairChallenges ch, unsigned long long q, unsigned lg_left, LsOut o) {
  const unsigned k = blockIdx.y, p = k >> 1;
  ls_cubic_pow_block<true, FALLBACK>(t.a[k], t.b[k], t.c[k], pw.pl[p], pw.pr[p], q, lg_left, ch.r[p], o);
}

// ---- quadratic -----------------------------------------------------------------------------------------------------------------------------------
// element x of the low half / of the high half of a table whose halves are `half` long, zero from lo / hi on (not read there)
__device__ __forceinline__ fe_t ls_low(const fe_t* __restrict__ Z, unsigned long long x, unsigned lo) { return x < lo ? Z[x] : fe_zero(); }
__device__ __forceinline__ fe_t ls_high(const fe_t* __restrict__ Z, unsigned long long x, unsigned long long half, unsigned hi) { return x < hi ? Z[x + half] : fe_zero(); }
// bound element x of a 4q-long table with (lo, hi); written back only below eff = max(lo, hi): past it the bound table counts as zero (after_bind)
__device__ __forceinline__ fe_t ls_bind_eff(fe_t* __restrict__ Z, unsigned long long x, unsigned long long q, unsigned lo, unsigned hi, const fe_t& r) {
  const unsigned eff = lo > hi ? lo : hi;
  if (x >= eff) return fe_zero();
  const fe_t v = ls_bind(ls_low(Z, x, lo), ls_high(Z, x, 2 * q, hi), r);
  Z[x] = v;
  return v;
}
template <bool BIND>
__device__ __forceinline__ void ls_quad_block(fe_t* __restrict__ A, fe_t* __restrict__ B, unsigned long long q, const fe_t& r, const LsEff f, const LsOut& o) {
  __shared__ fe_t smem[2 * 4];
  const unsigned long long base = (unsigned long long)blockIdx.x * LS_CHUNK;
  fe_t acc[2] = {fe_zero(), fe_zero()};
#pragma unroll 1
  for (unsigned j = 0; j < LS_CHUNK / 256; ++j) {
    const unsigned long long id = base + j * 256 + threadIdx.x;
    if (id >= q) break;
    fe_t a0, a1, b0, b1;
    if (BIND) {
      a0 = ls_bind_eff(A, id, q, f.loA, f.hiA, r);
      a1 = ls_bind_eff(A, id + q, q, f.loA, f.hiA, r);
      b0 = ls_bind_eff(B, id, q, f.loB, f.hiB, r);
      b1 = ls_bind_eff(B, id + q, q, f.loB, f.hiB, r);
    } else {
      a0 = ls_low(A, id, f.loA);
      a1 = ls_high(A, id, q, f.hiA);
      b0 = ls_low(B, id, f.loB);
      b1 = ls_high(B, id, q, f.hiB);
    }
    acc[0] = fe_add<S>(acc[0], fe_mul<S>(a0, b0));
    acc[1] = fe_add<S>(acc[1], fe_mul<S>(fe_sub<S>(a1, a0), fe_sub<S>(b1, b0)));
  }
  block_sum<2>(acc, smem);
  if (threadIdx.x == 0) ls_emit<2>(acc, o);
}
// eff: the LsEff of this launch's round, one per instance
__global__ void __launch_bounds__(256) k_ls_eval_quad(LsTables2 t, unsigned long long q, const LsEff* __restrict__ eff, LsOut o) {
  const unsigned k = blockIdx.y;
  ls_quad_block<false>(t.a[k], t.b[k], q, fe_zero(), eff[k], o);
}
__global__ void __launch_bounds__(256) k_ls_bind_eval_quad(LsTables2 t, LsChallenges ch, unsigned long long q, const LsEff* __restrict__ eff, LsOut o) {
  const unsigned k = blockIdx.y;
  ls_quad_block<true>(t.a[k], t.b[k], q, ch.r[k], eff[k], o);
}

// ---- second stage: nb block partials of instance k = blockIdx.x -> its record (the lazy 9-limb sums of k_sum_partials) -----------------------------
template <int NACC>
__global__ void __launch_bounds__(64) k_ls_sum_partials(const fe_t* __restrict__ partials, unsigned nb, fe_t* __restrict__ mapped, unsigned seq) {
  const unsigned k = blockIdx.x;
  const fe_t* __restrict__ P = partials + (size_t)k * nb * NACC;
  lazy9_t t[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) t[j] = lazy_from(fe_zero());
  for (unsigned b = threadIdx.x; b < nb; b += 64) {
#pragma unroll
    for (int j = 0; j < NACC; ++j) t[j] = lazy_add(t[j], lazy_from(P[(size_t)b * NACC + j]));
  }
  fe_t acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = lazy_reduce(lazy_wave_sum(t[j]));
  if (threadIdx.x == 0) ls_record<NACC>(acc, mapped, k, seq);
}

// ---- the last bind: two elements -> one per table; the record carries the bound elements 0 (the final claims) ---------------------------------------
// block = instance, thread t < NTAB = table t. eff == nullptr: dense tables (cubic).
template <int NTAB>
__global__ void __launch_bounds__(64) k_ls_bind_last(LsTables3 t, LsChallenges ch, const LsEff* __restrict__ eff, fe_t* __restrict__ mapped, unsigned seq) {
  __shared__ fe_t fin[3];
  const unsigned k = blockIdx.x;
  if (threadIdx.x < NTAB) {
    fe_t* Z = threadIdx.x == 0 ? t.a[k] : (threadIdx.x == 1 ? t.b[k] : t.c[k]);
    unsigned lo = 1, hi = 1;
    if (eff) {
      const LsEff f = eff[k];
      lo = threadIdx.x == 0 ? f.loA : f.loB;
      hi = threadIdx.x == 0 ? f.hiA : f.hiB;
    }
    const fe_t v = ls_bind(ls_low(Z, 0, lo), ls_high(Z, 0, 1, hi), ch.r[k]);
    Z[0] = v;
    fin[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    fe_t acc[NTAB];
#pragma unroll
    for (int j = 0; j < NTAB; ++j) acc[j] = fin[j];
    ls_record<NTAB>(acc, mapped, k, seq);
  }
}

}  // namespace spk
