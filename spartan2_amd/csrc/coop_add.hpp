// The block-cooperative point addition of the latency kernels (CoopAdd / xyzz_add_block4) and the XYZZ shuffle, shared by the translation units that walk
// window tables (kernels_msm.hpp in capi_group.hip, kernels_opening_batch.hpp, the one header of both forms of the batched opening, in capi_opening_batch.hip).
#pragma once
#include "curve.hpp"
#include "device_utils.hpp"

// SP_STAMP(i): wall-clock stamps (100 MHz) of block 0 / thread 0 for the latency kernels - compiled in only by tools/fb_stamps.hip
#ifdef SP_KERNEL_STAMPS
__device__ unsigned long long sp_stamps[192];
#define SP_STAMP(i)                                                     \
  do {                                                                  \
    if (threadIdx.x == 0 && blockIdx.x == 0) {                          \
      sp_stamps[i] = wall_clock64();                                    \
      sp_stamps[32 + (i)] = clock64();                                  \
    }                                                                   \
  } while (0)
__device__ unsigned sp_stage_ctr[4];
__device__ unsigned sp_hwid[4];
__device__ unsigned sp_predelay;  // 10 ns ticks every wave spins for before it starts (is the slow phase tied to time since launch or to the tree level?)
#ifdef SP_KERNEL_STAGE_STAMPS  // (each stage stamp costs a global counter round trip: only for looking inside a level, not for timing one)
#define SP_STAGE_STAMP()                                                          \
  do {                                                                            \
    if ((threadIdx.x & 63) == 0 && blockIdx.x == 0) sp_stamps[64 + 32 * (threadIdx.x >> 6) + (sp_stage_ctr[threadIdx.x >> 6]++ & 31)] = wall_clock64(); \
  } while (0)
#else
#define SP_STAGE_STAMP()
#endif
#else
#define SP_STAMP(i)
#define SP_STAGE_STAMP()
#endif

namespace spk {

__device__ __forceinline__ xyzz_t shfl_down_xyzz(const xyzz_t& a, int delta) {
  xyzz_t r;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    r.x.v[i] = __shfl_down(a.x.v[i], delta, 64);
    r.y.v[i] = __shfl_down(a.y.v[i], delta, 64);
    r.zz.v[i] = __shfl_down(a.zz.v[i], delta, 64);
    r.zzz.v[i] = __shfl_down(a.zzz.v[i], delta, 64);
  }
  return r;
}

// ---- block-cooperative addition in XYZZ coordinates -------------------------------------------------------------------------------------------
// The MSM tail is a chain of DEPENDENT additions on few points; a lone wave issues the base-field products of one addition back to back (~1 us
// each: the SIMD is saturated by one wave's quarter-rate 64-bit multiply-adds), ~15 us per Jacobian addition. Here FOUR wave groups ("roles", each
// on its own SIMD) share every addition: each role computes one product per dependency level for all ITEMS point pairs and the levels meet in LDS.
// Coordinates are (X, Y, ZZ, ZZZ) with x = X / ZZ, y = Y / ZZZ (add-2008-s): 14 products in FOUR levels of <= 4 - the Jacobian add-2007-bl this
// replaces needs 16 in five - so a chain of dependent additions is a fifth shorter. Points enter (Jacobian buckets, affine table entries) and leave
// (Jacobian sums for the host's Horner / normalisation) through two products each; the group element, hence every byte downstream, is the same.
template <int ITEMS>
struct CoopAdd {
  fe_t t[9][ITEMS];   // U1 -> Q | U2 -> P -> Y3a | S1 | S2 -> R | PP -> Y3b | RR | ZZ1 ZZ2 -> ZZ3 | ZZZ1 ZZZ2 -> ZZZ3 | PPP
  xyzz_t fix[ITEMS];  // results of the special cases (identity operand, P = +-Q), computed while the inputs are still intact
  int flag[ITEMS];
};
// All ITEMS * 4 threads of the block call this (it synchronises). role = threadIdx / ITEMS, i = threadIdx % ITEMS; P[i] += Q index given by the
// caller as pointers into LDS; `active` = this item takes part. The sum is written to dst[i] (may alias P: results are stored after the last level).
// CODE SIZE is what this routine is written around. Every wave of a latency kernel runs each instruction once per tree level, and a product is ~3 KB
// of straight-line code: with one inlined product per (stage, role) - 14 of them, plus the doubling case - a level was ~100 KB against a 64 KB
// instruction cache, and the same level took 5 us with its code cached and 10-12 us without (tools/fb_stamps.hip). Here every stage has ONE product that
// all four roles execute on operands they pick by address, so a level is ~15 KB and stays cached from the second level on. (A real call per product is
// no way out: 18 us per level with the call ABI's moves and scratch set-up.)
template <int ITEMS>
__device__ __forceinline__ void xyzz_add_block4(CoopAdd<ITEMS>& L, const xyzz_t* P, const xyzz_t* Q, xyzz_t* dst, int role, int i, bool active) {
  // EXEC stays FULL through the products: items that do not take part compute on whatever their slots hold and only the flag / result stores are
  // predicated. Measured (tools/fb_stamps.hip, profiles/r03_sparse_exec.txt): the same level of the same tree takes 5.2 us with every lane computing
  // and, in two launches out of three, 10-13 us once only 8 or 4 lanes of each wave are enabled - the long dependent v_mad_u64_u32 / v_addc chains
  // run 2.5-3x slower under a sparse EXEC mask on this part.
  // (A wave none of whose items takes part skips the products altogether: it would only compete with the wave it shares its SIMD with.)
  fe_t(*t)[ITEMS] = L.t;
  const bool run = __ballot(active) != 0;  // wave-uniform
  // stage 1: U1 = X1 ZZ2 | U2 = X2 ZZ1 | S1 = Y1 ZZZ2 | S2 = Y2 ZZZ1
  if (run) {
    if (active && role == 0) {
      int f = 0;
      if (xyzz_is_identity(*P)) {
        L.fix[i] = *Q;
        f = 1;
      } else if (xyzz_is_identity(*Q)) {
        L.fix[i] = *P;
        f = 1;
      }
      L.flag[i] = f;
    }
    const xyzz_t* a = (role & 1) ? Q : P;
    const xyzz_t* b = (role & 1) ? P : Q;
    const fe_t* xp = (role & 2) ? &a->y : &a->x;
    const fe_t* yp = (role & 2) ? &b->zzz : &b->zz;
    t[role][i] = fe_mul_rowwise<B>(*xp, *yp);
  }
  SP_STAGE_STAMP();
  __syncthreads();
  // stage 2: PP = (U2 - U1)^2, P kept | RR = (S2 - S1)^2, R kept | ZZ1 ZZ2 | ZZZ1 ZZZ2
  if (run) {
    fe_t x, y;
    if (role < 2) {
      x = fe_sub<B>(t[2 * role + 1][i], t[2 * role][i]);
      t[2 * role + 1][i] = x;
      y = x;
    } else {
      x = *((role & 1) ? &P->zzz : &P->zz);
      y = *((role & 1) ? &Q->zzz : &Q->zz);
    }
    t[4 + role][i] = fe_mul_rowwise<B>(x, y);
  }
  SP_STAGE_STAMP();
  __syncthreads();
  // stage 3: PPP = P PP (+ the P = +-Q case) | Q = U1 PP | ZZ3 = ZZ1 ZZ2 PP
  if (run && role < 3) {
    if (role == 0 && active && __builtin_expect(fe_is_zero(t[1][i]) && !L.flag[i], 0)) {
      L.fix[i] = fe_is_zero(t[3][i]) ? xyzz_dbl(*P) : xyzz_identity();
      L.flag[i] = 1;
    }
    const int xi = role == 0 ? 1 : role == 1 ? 0 : 6, oi = role == 0 ? 8 : role == 1 ? 0 : 6;
    t[oi][i] = fe_mul_rowwise<B>(t[xi][i], t[4][i]);
  }
  SP_STAGE_STAMP();
  __syncthreads();
  // stage 4: R (Q - X3) | S1 PPP | ZZZ3 = ZZZ1 ZZZ2 PPP
  if (run && role < 3) {
    const int xi = role == 0 ? 3 : role == 1 ? 2 : 7, oi = role == 0 ? 1 : role == 1 ? 4 : 7;
    fe_t y = t[8][i];
    if (role == 0) {
      const fe_t q = t[0][i];
      const fe_t x3 = fe_sub<B>(fe_sub<B>(t[5][i], y), fe_dbl<B>(q));
      y = fe_sub<B>(q, x3);
    }
    t[oi][i] = fe_mul_rowwise<B>(t[xi][i], y);
  }
  SP_STAGE_STAMP();
  __syncthreads();
  if (active && role == 0) {
    xyzz_t r;
    if (L.flag[i]) {
      r = L.fix[i];
    } else {
      r.x = fe_sub<B>(fe_sub<B>(t[5][i], t[8][i]), fe_dbl<B>(t[0][i]));
      r.y = fe_sub<B>(t[1][i], t[4][i]);
      r.zz = t[6][i];
      r.zzz = t[7][i];
    }
    dst[i] = r;
  }
  __syncthreads();
}

}  // namespace spk
