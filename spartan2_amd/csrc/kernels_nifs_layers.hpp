// k_nifs_layers: the NIFS layers of prep_prove's cached_step_matvec (src/neutronnova_zk.rs:1520-1600) for ALL instances of ALL states in one launch:
//   out[M][v][row] = sum_col M[row, col] * z_v[col],   M in {A, B, C},   z_v = [W_v | 1 | X_v],
// for the vectors v of a device-resident descriptor list. It is the walk of k_spmv3_multi (kernels_spmv_multi.hpp) - one lane per row, a chunk of
// NIFS_LAYERS_KC vectors sharing every index / code / coefficient load, rows longer than SPMV_LONG_ROW walked by the whole wave and added with shuffle
// trees - with two differences:
//   z is never assembled. A gathered column reads W[col] when col < num_vars, else tail[col - num_vars]; `tail` = [1 | X] of the vector, a few
//     elements that the entry uploads once for the whole call. nifs_prepare copies W into a scratch z per layer (1 MiB a layer at 2^15 variables).
//   The vector descriptors (W, tail, the three layer pointers) are read from a device array, the chunk chosen by blockIdx.z: one launch covers
//     every chunk of every state (grid = row blocks x 3 matrices x chunks), whatever count * n_padded is. A chunk may span two states' objects.
// Padding layers are further descriptors on the W and tail of instance 0: their words are those of one more product of the same vector, which is what
// nifs_prepare computes for them. Field sums are exact, so the words do not depend on the grouping.
//
// NIFS_LAYERS_KC = 4 from the compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950); see the figures beside the constant.
//
// Included by capi_sparse.hip behind SplitDev / acc_small and SPMV_LONG_ROW; launched by sp::nifs_layers_launch for sp_nifs_layers_batch (capi_nifs.hip).
#pragma once

namespace spk {

// 4: 162 VGPRs, 98 SGPRs, no AGPR, no scratch, no spilled VGPR or SGPR, three waves a SIMD - the figures of k_spmv3_multi at SPMV_KC = 4 (164 VGPRs);
// the chunk's descriptors (three pointers a vector for the block's matrix) sit in SGPRs. 2: 142 VGPRs, 80 SGPRs, the same three waves with half the
// gathers in flight per lane. 8: 256 VGPRs + 4 AGPRs, 30 spilled SGPRs, ONE wave a SIMD.
constexpr int NIFS_LAYERS_KC = 4;

struct NifsLayersArgs {
  SplitDev m[3];
  const sp::NifsLayerVec* vecs;  // device: nvec descriptors
  unsigned nvec, num_vars;
  unsigned chunk0;  // the chunk of blockIdx.z == 0 (a call of more than 65535 chunks is several launches)
};

struct NifsLayersChunk {  // one chunk's descriptors for one matrix, uniform over the block
  const fe_t* W[NIFS_LAYERS_KC];
  const fe_t* tail[NIFS_LAYERS_KC];
  fe_t* out[NIFS_LAYERS_KC];
  int kc;
  unsigned num_vars;
};

// acc[k] += sum over the entries (first, first + step, ..) of `row` of coefficient * z_k[col]
__device__ __forceinline__ void nifs_layers_row(const SplitDev& m, size_t row, const NifsLayersChunk& c, unsigned first, unsigned step, fe_t (&acc)[NIFS_LAYERS_KC]) {
  for (unsigned e = m.sptr[row] + first, end = m.sptr[row + 1]; e < end; e += step) {
    const unsigned col = m.sidx[e];
    const int code = m.scode[e];
    const bool in_w = col < c.num_vars;
    const unsigned at = in_w ? col : col - c.num_vars;
#pragma unroll
    for (int k = 0; k < NIFS_LAYERS_KC; ++k)
      if (k < c.kc) acc[k] = acc_small(acc[k], code, (in_w ? c.W[k] : c.tail[k])[at]);
  }
  for (unsigned e = m.gptr[row] + first, end = m.gptr[row + 1]; e < end; e += step) {
    const unsigned col = m.gidx[e];
    const fe_t v = m.gval[e];
    const bool in_w = col < c.num_vars;
    const unsigned at = in_w ? col : col - c.num_vars;
#pragma unroll
    for (int k = 0; k < NIFS_LAYERS_KC; ++k)
      if (k < c.kc) acc[k] = fe_add<S>(acc[k], fe_mul<S>(v, (in_w ? c.W[k] : c.tail[k])[at]));
  }
}

__global__ void __launch_bounds__(256) k_nifs_layers(NifsLayersArgs a, size_t nrows) {
  const int which = blockIdx.y;
  const SplitDev m = a.m[which];
  const unsigned v0 = (a.chunk0 + blockIdx.z) * (unsigned)NIFS_LAYERS_KC;  // < nvec (the grid has no chunk beyond the list)
  NifsLayersChunk c;
  c.kc = (int)(a.nvec - v0 < (unsigned)NIFS_LAYERS_KC ? a.nvec - v0 : (unsigned)NIFS_LAYERS_KC);
  c.num_vars = a.num_vars;
#pragma unroll
  for (int k = 0; k < NIFS_LAYERS_KC; ++k) {  // (the slots of a ragged chunk repeat its first vector and are never dereferenced)
    const sp::NifsLayerVec& d = a.vecs[v0 + (k < c.kc ? k : 0)];
    c.W[k] = d.W;
    c.tail[k] = d.tail;
    c.out[k] = d.out[which];
  }
  const unsigned lane = threadIdx.x & 63u;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t wbase = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); wbase < nrows; wbase += stride) {  // (uniform over a wave)
    const size_t row = wbase + lane;
    const bool valid = row < nrows;
    unsigned len = 0;
    if (valid) len = (m.sptr[row + 1] - m.sptr[row]) + (m.gptr[row + 1] - m.gptr[row]);
    const bool is_long = len > SPMV_LONG_ROW;
    fe_t acc[NIFS_LAYERS_KC];
#pragma unroll
    for (int k = 0; k < NIFS_LAYERS_KC; ++k) acc[k] = fe_zero();
    if (len && !is_long) nifs_layers_row(m, row, c, 0, 1, acc);
    unsigned long long pending = __ballot(is_long);
    while (pending) {
      const int owner = __ffsll((long long)pending) - 1;
      pending &= pending - 1;
      fe_t part[NIFS_LAYERS_KC];
#pragma unroll
      for (int k = 0; k < NIFS_LAYERS_KC; ++k) part[k] = fe_zero();
      nifs_layers_row(m, wbase + (size_t)owner, c, lane, 64, part);
#pragma unroll
      for (int k = 0; k < NIFS_LAYERS_KC; ++k)
        if (k < c.kc) {  // (uniform over the block)
          const fe_t s = wave_sum(part[k]);
          if ((int)lane == owner) acc[k] = s;
        }
    }
    if (valid) {
#pragma unroll
      for (int k = 0; k < NIFS_LAYERS_KC; ++k)
        if (k < c.kc) c.out[k][row] = acc[k];
    }
  }
}

}  // namespace spk
