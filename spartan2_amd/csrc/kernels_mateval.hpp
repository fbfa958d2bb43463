// k_matrix_evals_batched: A(rx, ry), B(rx, ry), C(rx, ry) of `evaluate_with_tables_fast` (src/r1cs/mod.rs:1216-1226) for a CHUNK of up to MATEVAL_KC
// point pairs in one walk over the row-major structures k_spmv3 walks:
//   e[k][M] = sum_(row, col) M[row, col] * tx_k[row] * ty_k[col],   M in {A, B, C},  k < kc <= MATEVAL_KC.
// A verifier needs nothing but these 3 numbers per proof; the single-proof route (sp_multiply_vec against T_y, three sp_table_dot with T_x) writes and
// reads back three N-element product tables on the way and streams the structure once per proof. Here every index / code / coefficient is loaded ONCE
// and used for the kc gathers ty_k[col]; per row the kc row sums are multiplied once by tx_k[row] and added to the lane's kc running totals; nothing
// of size N is written. The totals are then summed wave -> block -> the last block to arrive at the matrix's ticket (the idiom of
// k_polyabc_short_and_long's long columns). Field sums are exact, so the result does not depend on the grid or on the order of arrival.
//
// Long rows (the 32-bit additions of a SHA-256 round: 33 .. 225 entries among rows of one to three) are walked by the whole wave, an entry per lane, as
// in k_spmv3<true> - but without its shuffle tree: the evaluation is linear in the row sum, so every lane multiplies ITS share of the row by tx_k[row]
// and keeps it in its own totals.
//
// The kc tables stay separate allocations: the entry point takes the caller's tables as they are, and an interleaved chunk (element `col` of all kc
// tables adjacent: one 128-byte fetch per entry instead of four 32-byte gathers that each pay a 64-byte request) would first have to be written, a pass
// over kc x num_cols elements per chunk. The kernel is bound by exactly these gathers (profiles/verify_batch.md); the interleaved form is not built.
//
// MATEVAL_KC = 4 from the compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950; profiles/verify_batch.md): 174 VGPRs, no scratch,
// two waves a SIMD - 2 x KC accumulators of 8 VGPRs each beside one Montgomery product in flight. KC = 8 compiles to 256 VGPRs with 21 spilled
// SGPRs and ONE wave a SIMD, for a kernel that lives on gathers in flight.
//
// Included by capi_sparse.hip behind SplitDev / acc_small (the coefficient classes of sparse.rs:137-155).
#pragma once

namespace spk {

constexpr int MATEVAL_KC = 4;
constexpr unsigned MATEVAL_MAX_BLOCKS = 1024;  // per matrix: the last block adds this many partial rows of kc elements at most

struct MatEvalArgs {
  SplitDev m[3];
  const fe_t* tx[MATEVAL_KC];
  const fe_t* ty[MATEVAL_KC];
  fe_t* partials;     // [3][gridDim.x][MATEVAL_KC] block sums
  unsigned* tickets;  // [3] arrival counters, zero between launches
  fe_t* out;          // [MATEVAL_KC][3]: A, B, C per pair
  int kc;             // pairs in this chunk
};

// sums[k] += sum over the entries (first, first + step, ..) of `row` of coefficient * ty_k[col]
__device__ __forceinline__ void mateval_row(const SplitDev& m, size_t row, const MatEvalArgs& a, unsigned first, unsigned step, fe_t (&sums)[MATEVAL_KC]) {
  for (unsigned e = m.sptr[row] + first, end = m.sptr[row + 1]; e < end; e += step) {
    const unsigned col = m.sidx[e];
    const int code = m.scode[e];
#pragma unroll
    for (int k = 0; k < MATEVAL_KC; ++k)
      if (k < a.kc) sums[k] = acc_small(sums[k], code, a.ty[k][col]);
  }
  for (unsigned e = m.gptr[row] + first, end = m.gptr[row + 1]; e < end; e += step) {
    const unsigned col = m.gidx[e];
    const fe_t v = m.gval[e];
#pragma unroll
    for (int k = 0; k < MATEVAL_KC; ++k)
      if (k < a.kc) sums[k] = fe_add<S>(sums[k], fe_mul<S>(v, a.ty[k][col]));
  }
}

__global__ void __launch_bounds__(256) k_matrix_evals_batched(MatEvalArgs a, size_t nrows) {
  __shared__ fe_t smem[MATEVAL_KC * 4];
  __shared__ unsigned s_last;
  const int which = blockIdx.y;
  const SplitDev m = a.m[which];
  const unsigned lane = threadIdx.x & 63u;
  fe_t tot[MATEVAL_KC], sums[MATEVAL_KC];
#pragma unroll
  for (int k = 0; k < MATEVAL_KC; ++k) tot[k] = fe_zero();
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t wbase = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); wbase < nrows; wbase += stride) {  // (uniform over a wave)
    const size_t row = wbase + lane;
    unsigned len = 0;
    if (row < nrows) len = (m.sptr[row + 1] - m.sptr[row]) + (m.gptr[row + 1] - m.gptr[row]);
    const bool is_long = len > SPMV_LONG_ROW;
    if (len && !is_long) {  // (padding rows and the rows a matrix leaves empty cost their two pointer loads)
#pragma unroll
      for (int k = 0; k < MATEVAL_KC; ++k) sums[k] = fe_zero();
      mateval_row(m, row, a, 0, 1, sums);
#pragma unroll
      for (int k = 0; k < MATEVAL_KC; ++k)
        if (k < a.kc) tot[k] = fe_add<S>(tot[k], fe_mul<S>(a.tx[k][row], sums[k]));
    }
    unsigned long long pending = __ballot(is_long);
    while (pending) {
      const size_t r = wbase + (size_t)(__ffsll((long long)pending) - 1);
      pending &= pending - 1;
#pragma unroll
      for (int k = 0; k < MATEVAL_KC; ++k) sums[k] = fe_zero();
      mateval_row(m, r, a, lane, 64, sums);
#pragma unroll
      for (int k = 0; k < MATEVAL_KC; ++k)
        if (k < a.kc) tot[k] = fe_add<S>(tot[k], fe_mul<S>(a.tx[k][r], sums[k]));
    }
  }
  block_sum<MATEVAL_KC>(tot, smem);
  fe_t* mine = a.partials + (size_t)which * gridDim.x * MATEVAL_KC;
  if (threadIdx.x == 0) {
    unsigned* dst = reinterpret_cast<unsigned*>(mine + (size_t)blockIdx.x * MATEVAL_KC);
#pragma unroll
    for (int k = 0; k < MATEVAL_KC; ++k)
#pragma unroll
      for (int w = 0; w < 8; ++w) __hip_atomic_store(dst + 8 * k + w, tot[k].v[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // release / acquire at agent scope on the ticket, as for the long columns of k_polyabc_short_and_long: one arrival per block, at the block's end
    s_last = __hip_atomic_fetch_add(a.tickets + which, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
#pragma unroll
  for (int k = 0; k < MATEVAL_KC; ++k) tot[k] = fe_zero();
  for (unsigned b = threadIdx.x; b < gridDim.x; b += blockDim.x) {
    const unsigned* src = reinterpret_cast<const unsigned*>(mine + (size_t)b * MATEVAL_KC);
#pragma unroll
    for (int k = 0; k < MATEVAL_KC; ++k) {
      fe_t p;
#pragma unroll
      for (int w = 0; w < 8; ++w) p.v[w] = __hip_atomic_load(src + 8 * k + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tot[k] = fe_add<S>(tot[k], p);
    }
  }
  __syncthreads();  // smem reuse
  block_sum<MATEVAL_KC>(tot, smem);
  if (threadIdx.x == 0) {
    __hip_atomic_store(a.tickets + which, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
#pragma unroll
    for (int k = 0; k < MATEVAL_KC; ++k)
      if (k < a.kc) a.out[k * 3 + which] = tot[k];
  }
}

}  // namespace spk
