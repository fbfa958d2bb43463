// Kernels of a batch opened ahead (sp_hyrax_prove_batch_begin / _rows / _finish, capi_opening_batch.hip) beside those of kernels_opening_batch.hpp:
// the mask vectors are drawn at _begin, when the evaluation point does not exist yet, so k_ob_mask comes in two halves:
//   k_ob_dvec     d_k = from_uniform(blocks_k) alone (ipa.rs:139-145)
//   k_ob_ip       the block sums of <R_k, d_k>, R_k = eq(column point k) (ipa.rs:148), from the stored d_k once the point is known
// Exact field arithmetic: the sums are those k_ob_mask forms, block by block.
#pragma once
#include "kernels_opening_batch.hpp"

namespace spk {

// grid (ceil(cols / 256), count): d[k][i] alone - the first half of k_ob_mask, for a caller that does not know R yet
__global__ void __launch_bounds__(OB_STREAM_THREADS) k_ob_dvec(const ObInst* __restrict__ inst, unsigned cols, fe_t* __restrict__ d) {
  const unsigned i = blockIdx.x * OB_STREAM_THREADS + threadIdx.x;
  if (i >= cols) return;
  d[(size_t)blockIdx.y * cols + i] = fe_from_uniform<SF>(inst[blockIdx.y].blocks + 64 * (size_t)i);
}

// grid (ceil(cols / 256), count): the second half of k_ob_mask - ip_part[k][block] = sum over the block's columns of R_k[i] d[k][i], d as k_ob_dvec left it
__global__ void __launch_bounds__(OB_STREAM_THREADS) k_ob_ip(const ObInst* __restrict__ inst, unsigned cols, int nvr, int ncv, const fe_t* __restrict__ d,
                                                             fe_t* __restrict__ ip_part) {
  __shared__ fe_t s[OB_STREAM_THREADS];
  const ObInst& I = inst[blockIdx.y];
  const unsigned i = blockIdx.x * OB_STREAM_THREADS + threadIdx.x;
  fe_t term = fe_zero();
  if (i < cols) term = fe_mul<SF>(ob_eq_at(I.point + nvr, ncv, i), d[(size_t)blockIdx.y * cols + i]);
  s[threadIdx.x] = term;
  __syncthreads();
  for (int off = OB_STREAM_THREADS / 2; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] = fe_add<SF>(s[threadIdx.x], s[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) ip_part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s[0];
}

}  // namespace spk
