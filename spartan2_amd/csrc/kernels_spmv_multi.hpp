// k_spmv3_multi: PrecomputedSparseMatrix::multiply_vec_batched (src/r1cs/sparse.rs:237-302, called by SplitR1CSShape::multiply_vec_batched,
// src/r1cs/mod.rs:1130-1166) for a CHUNK of up to SPMV_KC vectors in ONE walk over the row-major structures of A, B and C:
//   out[M][k][row] = sum_col M[row, col] * z_k[col],   M in {A, B, C},  k < kc <= SPMV_KC.
// k_spmv3<true> - the product of one vector - is bound by its chains of dependent loads (index, then element), not by bandwidth: here every index, code
// and coefficient is loaded ONCE and used for the kc gathers z_k[col], which are independent of one another, so a lane has kc gathers in flight per
// entry where the single product has one, and the structure is streamed once per chunk instead of once per vector. One lane per row, kc accumulators,
// kc stores. Rows longer than SPMV_LONG_ROW (the 32-bit additions of a SHA-256 round) are walked by the whole wave, an entry per lane, and added with kc
// shuffle trees (wave_sum), the owner lane keeping the sums - as in k_spmv3<true>. Field sums are exact: the words are those of kc single products.
//
// The kc vectors stay separate allocations (the caller's tables as they are), as in k_matrix_evals_batched.
//
// SPMV_KC = 4 from the compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950): 164 VGPRs, 84 SGPRs, no scratch, no spilled VGPR or
// SGPR, three waves a SIMD - kc accumulators and, in a long row, kc partial sums of 8 VGPRs each beside the gathered elements (k_spmv3<true>: 116 VGPRs,
// four waves). SPMV_KC = 2 compiles to 146 VGPRs and the same three waves with half the gathers in flight per lane; SPMV_KC = 8 to 256 VGPRs + 4 AGPRs
// with 2 spilled SGPRs and ONE wave a SIMD, for a kernel that lives on gathers in flight.
//
// Included by capi_sparse.hip behind SplitDev / acc_small (the coefficient classes of sparse.rs:137-155) and SPMV_LONG_ROW.
#pragma once

namespace spk {

constexpr int SPMV_KC = 4;

struct SpmvMultiArgs {
  SplitDev m[3];
  const fe_t* z[SPMV_KC];
  fe_t* out[3][SPMV_KC];  // [matrix][vector]
  int kc;                 // vectors in this chunk; the slots from kc on are never dereferenced
};

// acc[k] += sum over the entries (first, first + step, ..) of `row` of coefficient * z_k[col]
__device__ __forceinline__ void spmv_multi_row(const SplitDev& m, size_t row, const SpmvMultiArgs& a, unsigned first, unsigned step, fe_t (&acc)[SPMV_KC]) {
  for (unsigned e = m.sptr[row] + first, end = m.sptr[row + 1]; e < end; e += step) {
    const unsigned col = m.sidx[e];
    const int code = m.scode[e];
#pragma unroll
    for (int k = 0; k < SPMV_KC; ++k)
      if (k < a.kc) acc[k] = acc_small(acc[k], code, a.z[k][col]);
  }
  for (unsigned e = m.gptr[row] + first, end = m.gptr[row + 1]; e < end; e += step) {
    const unsigned col = m.gidx[e];
    const fe_t v = m.gval[e];
#pragma unroll
    for (int k = 0; k < SPMV_KC; ++k)
      if (k < a.kc) acc[k] = fe_add<S>(acc[k], fe_mul<S>(v, a.z[k][col]));
  }
}

__global__ void __launch_bounds__(256) k_spmv3_multi(SpmvMultiArgs a, size_t nrows) {
  const int which = blockIdx.y;
  const SplitDev m = a.m[which];
  const unsigned lane = threadIdx.x & 63u;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t wbase = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); wbase < nrows; wbase += stride) {  // (uniform over a wave)
    const size_t row = wbase + lane;
    const bool valid = row < nrows;
    unsigned len = 0;
    if (valid) len = (m.sptr[row + 1] - m.sptr[row]) + (m.gptr[row + 1] - m.gptr[row]);
    const bool is_long = len > SPMV_LONG_ROW;
    fe_t acc[SPMV_KC];
#pragma unroll
    for (int k = 0; k < SPMV_KC; ++k) acc[k] = fe_zero();
    if (len && !is_long) spmv_multi_row(m, row, a, 0, 1, acc);
    unsigned long long pending = __ballot(is_long);
    while (pending) {
      const int owner = __ffsll((long long)pending) - 1;
      pending &= pending - 1;
      fe_t part[SPMV_KC];
#pragma unroll
      for (int k = 0; k < SPMV_KC; ++k) part[k] = fe_zero();
      spmv_multi_row(m, wbase + (size_t)owner, a, lane, 64, part);
#pragma unroll
      for (int k = 0; k < SPMV_KC; ++k)
        if (k < a.kc) {  // (uniform over the grid)
          const fe_t s = wave_sum(part[k]);
          if ((int)lane == owner) acc[k] = s;
        }
    }
    if (valid) {
#pragma unroll
      for (int k = 0; k < SPMV_KC; ++k)
        if (k < a.kc) a.out[which][k][row] = acc[k];
    }
  }
}

}  // namespace spk
