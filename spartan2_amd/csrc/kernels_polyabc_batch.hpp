// evals_rx + poly_ABC for a CHUNK of up to PAB_KC proofs of one shape (sp_poly_abc_batch): EqPolynomial::evals_from_points (src/polys/eq.rs:59-117)
// and SplitR1CSShape::bind_and_prepare_poly_ABC[_full] (src/r1cs/mod.rs:1235-1321) with ONE walk over the column-major structures that
// k_polyabc_short_and_long walks once per proof.
//   k_pab_eq_levels   the two eq pyramids of every proof of the chunk (eq_levels_block, as k_ls_eq_levels builds them for the lockstep sum-checks):
//                     the left one over r_x[0 .. hi_bits), the right one over r_x[hi_bits .. ell), the points by value
//   k_pab_eq_outer    E[row * PAB_KC + j] = hi_j[row >> lo_bits] * lo_j[row & (2^lo_bits - 1)]: the chunk's eq tables INTERLEAVED, element `row` of
//                     all proofs in PAB_KC x 32 contiguous bytes. One exact field product per element, so the words are evals_from_points' whatever the
//                     split; one code path for every ell. Thread t = element t of E: the stores of a wave are 2 KiB contiguous.
//   k_pab_walk        per entry of a column one index and one code load, then PAB_KC element loads from E + idx * PAB_KC - the 64-byte request a lone
//                     32-byte gather pays (profiles/r06_pmc_calibration.json: 63-64 bytes fetched per gather) now serves two proofs, a 128-byte line
//                     four. PAB_KC accumulators per matrix; B's and C's sums are folded into the running totals with r_j, r_j^2 as soon as they are
//                     done, so a lane holds 2 x PAB_KC elements beside its gathers in flight, not 3 x. The grid is k_polyabc_short_and_long's: the long
//                     columns' blocks first (NB blocks a column, PAB_KC partial triples a block stored write-through, the column's last arrival adds
//                     them), then the short columns in `order`, then the blocks that write the PAB_KC zero tails.
// The interleaved table is what k_matrix_evals_batched could not have (its T_y tables are the caller's own): here evals_rx does not exist before the
// walk and nothing else reads it, so writing it interleaved costs no extra pass.
//
// A ragged chunk (kc < PAB_KC) runs the <false> instantiation: slots j >= kc are neither built, read nor written.
//
// PAB_KC is a compile-time constant (-DPOLYABC_BATCH_KC=2 builds the other candidate). PAB_KC = 4 from the measurement (profiles/prove_batch.md, K = 16 at
// config 2, launch totals a proof): 72 us against 86 us for PAB_KC = 2 and 81 us for sp_eq_table_into + sp_poly_abc back to back. Compiler's resource
// report (-Rpass-analysis=kernel-resource-usage, gfx950) of k_pab_walk<true>: PAB_KC = 4: 206 VGPRs, no spilled VGPR, 2 waves a SIMD; PAB_KC = 2: 173 VGPRs,
// no spilled VGPR, 2 waves a SIMD (k_polyabc_short_and_long: 149 VGPRs, 3 waves).
//
// Included by capi_sparse.hip behind SplitDev / acc_small / LONG_NB_MAX / long_nb.
#pragma once
#include "kernels_shared.hpp"

#ifndef POLYABC_BATCH_KC
#define POLYABC_BATCH_KC 4
#endif

namespace spk {

constexpr int PAB_KC = POLYABC_BATCH_KC;
static_assert(PAB_KC == 2 || PAB_KC == 4, "the in-flight depth of pab_gather_col is written for 2 and 4");
constexpr int PAB_MAX_ELL = 28;  // PAB_KC x 28 elements by value: the kernel argument stays the size of the lockstep kernels' (LsTables3 + LsChallenges), well below 4 KiB
// entries a lane has in flight (gather_major_x4 has 4 of one element each): 4 / PAB_KC, i.e. four 32-byte element loads either way. Twice that was
// measured and loses at both sizes (PAB_KC = 4: 256 VGPRs + 39 AGPRs, one wave a SIMD, 102 against 72 us a proof; PAB_KC = 2: 205 against 173 VGPRs at
// the same two waves, 88 against 86 us; profiles/prove_batch.md)
constexpr int PAB_INFLIGHT = 4 / PAB_KC;

struct PabPoints {
  fe_t v[PAB_KC][PAB_MAX_ELL];  // r_x of proof j
};
// pyramids of proof j at pyr + j * stride: the left one (hi_bits levels), then, pyr_hi elements behind it, the right one (ell - hi_bits levels)
__global__ void __launch_bounds__(1024) k_pab_eq_levels(PabPoints p, int ell, int hi_bits, fe_t* __restrict__ pyr, unsigned long long stride, unsigned long long pyr_hi) {
  __shared__ fe_t lv[EQ_LDS_ENTRIES];
  const int j = blockIdx.y;
  fe_t* o = pyr + (size_t)j * stride;
  if (blockIdx.x == 0) eq_levels_block(&p.v[j][hi_bits - 1], hi_bits, o, lv);
  else eq_levels_block(&p.v[j][ell - 1], ell - hi_bits, o + pyr_hi, lv);
}

__global__ void __launch_bounds__(256) k_pab_eq_outer(const fe_t* __restrict__ pyr, unsigned long long stride, unsigned long long off_hi, unsigned long long off_lo, int lo_bits,
                                                      size_t n_rows, int kc, fe_t* __restrict__ E) {
  const size_t mask = ((size_t)1 << lo_bits) - 1, total = n_rows * PAB_KC;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const size_t row = t / PAB_KC;
    const int j = (int)(t % PAB_KC);
    if (j >= kc) continue;
    const fe_t* __restrict__ q = pyr + (size_t)j * stride;
    E[t] = fe_mul<S>(q[off_hi + (row >> lo_bits)], q[off_lo + (row & mask)]);
  }
}

struct PabArgs {
  SplitDev m[3];  // column-major A, B, C
  fe_t r[PAB_KC], r2[PAB_KC];
  fe_t* out[PAB_KC];
  int kc;  // proofs in this chunk
};

// acc[j] += sum over the entries (first, first + step, ..) of one column of coefficient * E[row][j]: the long columns' share of a block
template <bool FULL>
__device__ __forceinline__ void pab_gather_strided(const SplitDev& m, size_t major, const fe_t* __restrict__ E, int kc, unsigned first, unsigned step, fe_t (&acc)[PAB_KC]) {
  for (unsigned k = m.sptr[major] + first, e = m.sptr[major + 1]; k < e; k += step) {
    const fe_t* __restrict__ x = E + (size_t)m.sidx[k] * PAB_KC;
    const int code = m.scode[k];
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j)
      if (FULL || j < kc) acc[j] = acc_small(acc[j], code, x[j]);
  }
  for (unsigned k = m.gptr[major] + first, e = m.gptr[major + 1]; k < e; k += step) {
    const fe_t* __restrict__ x = E + (size_t)m.gidx[k] * PAB_KC;
    const fe_t v = m.gval[k];
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j)
      if (FULL || j < kc) acc[j] = fe_add<S>(acc[j], fe_mul<S>(v, x[j]));
  }
}
// the whole column by one lane, PAB_INFLIGHT entries in flight: index / code loads first, then their PAB_KC-element gathers, then the accumulations
// (gather_major_x4's order)
template <bool FULL>
__device__ __forceinline__ void pab_gather_col(const SplitDev& m, size_t major, const fe_t* __restrict__ E, int kc, fe_t (&acc)[PAB_KC]) {
  unsigned k = m.sptr[major];
  const unsigned e = m.sptr[major + 1];
  for (; k + PAB_INFLIGHT <= e; k += PAB_INFLIGHT) {
    unsigned idx[PAB_INFLIGHT];
    int code[PAB_INFLIGHT];
#pragma unroll
    for (int u = 0; u < PAB_INFLIGHT; ++u) {
      idx[u] = m.sidx[k + u];
      code[u] = m.scode[k + u];
    }
    fe_t x[PAB_INFLIGHT][PAB_KC];
#pragma unroll
    for (int u = 0; u < PAB_INFLIGHT; ++u)
#pragma unroll
      for (int j = 0; j < PAB_KC; ++j)
        if (FULL || j < kc) x[u][j] = E[(size_t)idx[u] * PAB_KC + j];
#pragma unroll
    for (int u = 0; u < PAB_INFLIGHT; ++u)
#pragma unroll
      for (int j = 0; j < PAB_KC; ++j)
        if (FULL || j < kc) acc[j] = acc_small(acc[j], code[u], x[u][j]);
  }
  for (; k < e; ++k) {
    const fe_t* __restrict__ x = E + (size_t)m.sidx[k] * PAB_KC;
    const int code = m.scode[k];
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j)
      if (FULL || j < kc) acc[j] = acc_small(acc[j], code, x[j]);
  }
  for (unsigned g = m.gptr[major], ge = m.gptr[major + 1]; g < ge; ++g) {
    const fe_t* __restrict__ x = E + (size_t)m.gidx[g] * PAB_KC;
    const fe_t v = m.gval[g];
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j)
      if (FULL || j < kc) acc[j] = fe_add<S>(acc[j], fe_mul<S>(v, x[j]));
  }
}
__device__ __forceinline__ unsigned pab_col_len(const PabArgs& a, size_t col) {
  unsigned n = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) n += (a.m[i].sptr[col + 1] - a.m[i].sptr[col]) + (a.m[i].gptr[col + 1] - a.m[i].gptr[col]);
  return n;
}

// grid: [0, LONG_NB_MAX * n_long) the long columns' blocks, then `short_blocks` over the short columns, then the zero tails' blocks.
// partials: [n_long][LONG_NB_MAX][3][PAB_KC] elements; tickets: [n_long] arrival counters, zero between launches (each column's last block leaves zero).
template <bool FULL>
__global__ void __launch_bounds__(256) k_pab_walk(PabArgs a, const fe_t* __restrict__ E, const unsigned* __restrict__ order, size_t n_short,
                                                  const unsigned* __restrict__ long_cols, unsigned n_long, fe_t* __restrict__ partials, unsigned* __restrict__ tickets,
                                                  unsigned short_blocks, size_t zero_from, size_t zero_n, int permuted) {
  __shared__ fe_t smem[PAB_KC * 4];
  __shared__ unsigned s_last;
  const int kc = FULL ? PAB_KC : a.kc;
  const unsigned long_blocks = LONG_NB_MAX * n_long;
  if (blockIdx.x >= long_blocks + short_blocks) {
    const size_t n16 = zero_n * 2, nb = gridDim.x - long_blocks - short_blocks;
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j) {
      if (!FULL && j >= kc) break;
      uint4* z = reinterpret_cast<uint4*>(a.out[j] + zero_from);
      for (size_t i = (size_t)(blockIdx.x - long_blocks - short_blocks) * blockDim.x + threadIdx.x; i < n16; i += nb * blockDim.x) z[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  fe_t acc[PAB_KC], tot[PAB_KC];
  if (blockIdx.x < long_blocks) {
    const unsigned by = blockIdx.x / LONG_NB_MAX, bx = blockIdx.x % LONG_NB_MAX;
    const size_t col = long_cols[by];                 // the column's number: where its sums go
    const size_t at = permuted ? n_short + by : col;  // ... and where the structure keeps it
    const unsigned nb = long_nb(pab_col_len(a, at));
    if (bx >= nb) return;
    fe_t* trip = partials + (size_t)by * LONG_NB_MAX * 3 * PAB_KC;
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < PAB_KC; ++j) acc[j] = fe_zero();
      pab_gather_strided<FULL>(a.m[i], at, E, kc, bx * blockDim.x + threadIdx.x, nb * blockDim.x, acc);
      if (i) __syncthreads();  // smem reuse
      block_sum<PAB_KC>(acc, smem);
      if (threadIdx.x == 0) {
        unsigned* dst = reinterpret_cast<unsigned*>(trip + ((size_t)bx * 3 + i) * PAB_KC);
#pragma unroll
        for (int j = 0; j < PAB_KC; ++j)
#pragma unroll
          for (int w = 0; w < 8; ++w) __hip_atomic_store(dst + 8 * j + w, acc[j].v[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // release / acquire at agent scope on the column's ticket, as in k_polyabc_short_and_long
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(tickets + by, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nb - 1 ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < PAB_KC; ++j) acc[j] = fe_zero();
      if (threadIdx.x < nb) {
        const unsigned* src = reinterpret_cast<const unsigned*>(trip + ((size_t)threadIdx.x * 3 + i) * PAB_KC);
#pragma unroll
        for (int j = 0; j < PAB_KC; ++j)
#pragma unroll
          for (int w = 0; w < 8; ++w) acc[j].v[w] = __hip_atomic_load(src + 8 * j + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();  // smem reuse
      block_sum<PAB_KC>(acc, smem);
      if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < PAB_KC; ++j) tot[j] = i == 0 ? acc[j] : fe_add<S>(tot[j], fe_mul<S>(i == 1 ? a.r[j] : a.r2[j], acc[j]));
      }
    }
    if (threadIdx.x == 0) {
      __hip_atomic_store(tickets + by, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
#pragma unroll
      for (int j = 0; j < PAB_KC; ++j)
        if (FULL || j < kc) a.out[j][col] = tot[j];
    }
    return;
  }
  const size_t nblk = short_blocks;
  for (size_t i = (size_t)(blockIdx.x - long_blocks) * blockDim.x + threadIdx.x; i < n_short; i += nblk * blockDim.x) {
    const size_t col = order[i], at = permuted ? i : col;
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j) tot[j] = fe_zero();
    pab_gather_col<FULL>(a.m[0], at, E, kc, tot);
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j) acc[j] = fe_zero();
    pab_gather_col<FULL>(a.m[1], at, E, kc, acc);
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j)
      if (!fe_is_zero(acc[j])) tot[j] = fe_add<S>(tot[j], fe_mul<S>(a.r[j], acc[j]));
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j) acc[j] = fe_zero();
    pab_gather_col<FULL>(a.m[2], at, E, kc, acc);
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j)
      if (!fe_is_zero(acc[j])) tot[j] = fe_add<S>(tot[j], fe_mul<S>(a.r2[j], acc[j]));
#pragma unroll
    for (int j = 0; j < PAB_KC; ++j)
      if (FULL || j < kc) a.out[j][col] = tot[j];
  }
}

}  // namespace spk
