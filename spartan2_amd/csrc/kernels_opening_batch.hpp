// Kernels of sp_hyrax_prove_batch (capi_opening_batch.hip): `count` instances of HyraxPCS::prove (hyrax_pc.rs:387-478) with
// InnerProductArgumentLinear::prove (ipa.rs:125-170) inside, on ONE commitment key, every device stage ONE launch with the instance on blockIdx.y:
//   k_ob_mask     d_k = from_uniform(blocks_k) (ipa.rs:139-145) written once, and the block sums of <R_k, d_k>, R_k = eq(column point k) (:148)
//   k_ob_dvec     k_ob_mask's first half, d_k alone: a batch opened ahead draws the mask vectors before the evaluation point exists
//   k_ob_ip       its second half, the block sums of <R_k, d_k> from the stored d_k once the point is known (the same sums, block by block)
//   k_ob_rowmat   LZ_k = L_k^T W_k (bind_with_delayed, hyrax_pc.rs:38-54), L_k = eq(row point k) formed in LDS from the point
//   k_ob_walk     the table walk over one key's window tables for 2 count scalar vectors: delta_k = <d_k, ck> + r_delta_k h (ipa.rs:147), reduced
//                 from the uniform blocks as k_multi_mul_wide's raw64 form does, and comm_LZ_k = <LZ_k, ck> + r_LZ_k h (hyrax_pc.rs:454-455)
//   k_ob_z        z_vec_k = r_k LZ_k + d_k (ipa.rs:160-163)
// k_ob_walk takes a vector base, so that one launch covers the delta vectors alone (base 0) or the comm_LZ vectors alone (base count): a batch opened
// ahead (sp_hyrax_prove_batch_begin / _rows / _finish) walks them at different times.
// The walk is k_multi_mul_wide (kernels_msm.hpp) with the per-block item layout, CoopAdd / xyzz_add_block4 and the last-block join unchanged; what is
// new is the indexing: vector v = blockIdx.y has its own scalars, block-sum area, ticket and result, and the result is a plain store into device
// memory that the host fetches with one copy for all vectors. Results are group elements compared as canonical affine points and exact field
// elements, so neither the addition order nor the launch shape shows in a proof.
#pragma once
#include "coop_add.hpp"

namespace spk {
typedef FqP SF;  // scalar field

constexpr int OB_MAX = 64;                // instances per call (SP_LOCKSTEP_MAX)
constexpr int OB_WALK_ITEMS = 1024;       // (scalar, digit) items per block of the walk: MULTI_MUL_WIDE_ITEMS
constexpr int OB_WALK_MAX_BLOCKS = 128;   // block sums the last block of a vector joins in one pass: 4096 scalars
constexpr int OB_ROW_BITS_MAX = 10;       // row variables whose eq table fits the block's LDS copy
constexpr int OB_RMV_COLS = 8, OB_RMV_THREADS = 512, OB_RMV_ROWS_PER_PASS = OB_RMV_THREADS / OB_RMV_COLS;
constexpr int OB_STREAM_THREADS = 256;    // k_ob_mask / k_ob_dvec / k_ob_ip / k_ob_z: one element a thread

// one instance, as the kernels see it (a small device array, uploaded once per call; the two blinds make it mask material: wiped with the blocks)
struct ObInst {
  const uint8_t* blocks;  // cols uniform blocks of 64 bytes: the mask vector's draws
  const fe_t* poly;       // rows x cols
  const fe_t* lz;         // LZ_k: k_ob_rowmat's output, or the polynomial itself when it has one row (hyrax_pc.rs:417-423)
  const fe_t* point;      // npt elements, row variables first
  fe_t r_delta, r_lz;     // scalar of h in the two walks
};
struct ObChallenges {
  fe_t r[OB_MAX];
};

// eq(p_0 .. p_(k-1), i) with p_0 on the index MSB (EqPolynomial::evals_from_points, src/polys/eq.rs:59-93), one product per variable
__device__ __forceinline__ fe_t ob_eq_at(const fe_t* __restrict__ p, int k, unsigned i) {
  fe_t w = fe_one<SF>();
  for (int j = 0; j < k; ++j) {
    const fe_t pj = p[j];
    w = fe_mul<SF>(w, ((i >> (k - 1 - j)) & 1u) ? pj : fe_sub<SF>(fe_one<SF>(), pj));
  }
  return w;
}

// ip_part[instance][block] = the sum of the block's 256 terms: an LDS tree over halves 128, 64 .. 1 (exact field sums: the order shows in no result)
__device__ __forceinline__ void ob_block_sum(fe_t term, fe_t* __restrict__ ip_part) {
  __shared__ fe_t s[OB_STREAM_THREADS];
  s[threadIdx.x] = term;
  __syncthreads();
  for (int off = OB_STREAM_THREADS / 2; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] = fe_add<SF>(s[threadIdx.x], s[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) ip_part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s[0];
}

// grid (ceil(cols / 256), count): d[k][i] and ip_part[k][block] = sum over the block's columns of R_k[i] d_k[i]; the host adds the <= 16 block sums
__global__ void __launch_bounds__(OB_STREAM_THREADS) k_ob_mask(const ObInst* __restrict__ inst, unsigned cols, int nvr, int ncv, fe_t* __restrict__ d,
                                                               fe_t* __restrict__ ip_part) {
  const ObInst& I = inst[blockIdx.y];
  const unsigned i = blockIdx.x * OB_STREAM_THREADS + threadIdx.x;
  fe_t term = fe_zero();
  if (i < cols) {
    const fe_t di = fe_from_uniform<SF>(I.blocks + 64 * (size_t)i);
    d[(size_t)blockIdx.y * cols + i] = di;
    term = fe_mul<SF>(ob_eq_at(I.point + nvr, ncv, i), di);
  }
  ob_block_sum(term, ip_part);
}

// grid (ceil(cols / 256), count): d[k][i] alone, for a caller that does not know R yet
__global__ void __launch_bounds__(OB_STREAM_THREADS) k_ob_dvec(const ObInst* __restrict__ inst, unsigned cols, fe_t* __restrict__ d) {
  const unsigned i = blockIdx.x * OB_STREAM_THREADS + threadIdx.x;
  if (i >= cols) return;
  d[(size_t)blockIdx.y * cols + i] = fe_from_uniform<SF>(inst[blockIdx.y].blocks + 64 * (size_t)i);
}

// grid (ceil(cols / 256), count): ip_part[k][block] as k_ob_mask forms it, d as k_ob_dvec left it
__global__ void __launch_bounds__(OB_STREAM_THREADS) k_ob_ip(const ObInst* __restrict__ inst, unsigned cols, int nvr, int ncv, const fe_t* __restrict__ d,
                                                             fe_t* __restrict__ ip_part) {
  const ObInst& I = inst[blockIdx.y];
  const unsigned i = blockIdx.x * OB_STREAM_THREADS + threadIdx.x;
  fe_t term = fe_zero();
  if (i < cols) term = fe_mul<SF>(ob_eq_at(I.point + nvr, ncv, i), d[(size_t)blockIdx.y * cols + i]);
  ob_block_sum(term, ip_part);
}

// grid (ceil(cols / 8), count), 512 threads: k_rowmat_vec_tall's shape (kernels_bulk.hpp) - lane = (row-lane 0..7, column 0..7), a wave reads eight
// 256-byte row segments per pass, the 8 waves cover 64 rows - for any row count 2 .. 1024, with the row weights formed here from the row point
__global__ void __launch_bounds__(OB_RMV_THREADS) k_ob_rowmat(const ObInst* __restrict__ inst, unsigned rows, unsigned cols, int nvr, fe_t* __restrict__ lz) {
  __shared__ lazy9_t sm[OB_RMV_THREADS / 64][OB_RMV_COLS];
  __shared__ fe_t sL[1 << OB_ROW_BITS_MAX];
  const ObInst& I = inst[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & (OB_RMV_COLS - 1), rl = lane >> 3;
  const unsigned col = blockIdx.x * OB_RMV_COLS + c;
  for (unsigned r = threadIdx.x; r < rows; r += OB_RMV_THREADS) sL[r] = ob_eq_at(I.point, nvr, r);
  __syncthreads();
  const fe_t* __restrict__ poly = I.poly;
  fe_t acc = fe_zero();
  if (col < cols) {
    constexpr unsigned P = OB_RMV_ROWS_PER_PASS;
    unsigned r = (unsigned)wave * 8 + rl;
    for (; r + P < rows; r += 2 * P) {  // two loads in flight per lane
      const fe_t a0 = poly[(size_t)r * cols + col], a1 = poly[(size_t)(r + P) * cols + col];
      acc = fe_add<SF>(acc, fe_mul<SF>(sL[r], a0));
      acc = fe_add<SF>(acc, fe_mul<SF>(sL[r + P], a1));
    }
    for (; r < rows; r += P) acc = fe_add<SF>(acc, fe_mul<SF>(sL[r], poly[(size_t)r * cols + col]));
  }
  lazy9_t t = lazy_from(acc);
#pragma unroll
  for (int m = 32; m >= 8; m >>= 1) {
    lazy9_t o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.v[i] = __shfl_xor(t.v[i], m, 64);
    t = lazy_add(t, o);
  }
  if (rl == 0) sm[wave][c] = t;
  __syncthreads();
  if (threadIdx.x < OB_RMV_COLS && col < cols) {
    lazy9_t sum = sm[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < OB_RMV_THREADS / 64; ++w) sum = lazy_add(sum, sm[w][threadIdx.x]);
    lz[(size_t)blockIdx.y * cols + col] = lazy_reduce(sum);
  }
}

// grid (ceil(32 n / 1024) <= 128, vectors), 512 threads, vector v = vbase + blockIdx.y (vbase = 0 and 2 count vectors: all of them; count vectors from
// base 0 / from base count: the delta / the comm_LZ vectors alone). Vector v < count: delta of instance v - scalar idx < nraw is from_uniform(block idx); vector
// v >= count: comm_LZ of instance v - count - scalar idx < nraw is lz[idx]. Scalars nraw .. n - 2 are zero (a polynomial narrower than the key) and
// scalar n - 1, h's, is the instance's blind. partial: OB_WALK_MAX_BLOCKS block sums a vector; ticket: one counter a vector, zero at entry and at
// exit; out[v]: the Jacobian sum.
__global__ void __launch_bounds__(4 * 128) k_ob_walk(const ObInst* __restrict__ inst, unsigned count, unsigned vbase, size_t n, size_t nraw, const aff_t* __restrict__ tables,
                                                     xyzz_t* __restrict__ partial, unsigned* __restrict__ ticket, jac_t* __restrict__ out) {
  __shared__ CoopAdd<128> L;
  __shared__ xyzz_t s[256];
  __shared__ unsigned s_last;
  const unsigned v = vbase + blockIdx.y;
  const bool raw64 = v < count;
  const ObInst& I = inst[raw64 ? v : v - count];
  partial += (size_t)v * OB_WALK_MAX_BLOCKS;
  ticket += v;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, blk = wave >> 2;
  {
    const size_t e0 = (size_t)blockIdx.x * OB_WALK_ITEMS + 2 * (size_t)threadIdx.x, idx = e0 >> 5;
    const int j = (int)(e0 & 31);
    xyzz_t acc = xyzz_identity();
    if (idx < nraw || idx == n - 1) {
      fe_t sc;
      if (idx == n - 1) sc = raw64 ? I.r_delta : I.r_lz;
      else if (raw64) sc = fe_from_uniform<SF>(I.blocks + 64 * idx);
      else sc = I.lz[idx];
      const fe_t c = fe_to_canonical<SF>(sc);
      const unsigned d0 = (c.v[j >> 2] >> (8 * (j & 3))) & 0xffu, d1 = (c.v[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xffu;
      const aff_t* tab = tables + idx * (32 * 255);
      if (d0) acc = xyzz_from_affine(tab[(size_t)j * 255 + d0 - 1]);
      if (d1) acc = xyzz_add_mixed(acc, tab[(size_t)(j + 1) * 255 + d1 - 1]);
    }
    const xyzz_t other = shfl_down_xyzz(acc, 32);
    if (lane < 32) s[wave * 32 + lane] = xyzz_add(acc, other);
  }
  __syncthreads();
  const int role = (wave + 2 * blk) & 3, k = blk * 64 + lane;  // roles of an item block on four different SIMDs (see k_msm_window_reduce_coop)
  xyzz_add_block4<128>(L, &s[k], &s[k + 128], s, role, k, true);
  for (int off = 64; off >= 1; off >>= 1) {
    const bool active = k < off;
    xyzz_add_block4<128>(L, &s[k], &s[active ? k + off : k], s, role, k, active);
  }
  if (gridDim.x > 1) {
    if (threadIdx.x == 0) {
      partial[blockIdx.x] = s[0];
      __threadfence();  // the block sum is visible device-wide before the ticket is taken
      s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (role == 0) {
      xyzz_t acc = xyzz_identity();
      if (k < (int)gridDim.x) {  // other blocks' sums: loads that cannot be served from a stale line of this XCD's caches
        const unsigned* pw = reinterpret_cast<const unsigned*>(&partial[k]);
        unsigned* aw = reinterpret_cast<unsigned*>(&acc);
#pragma unroll
        for (int w = 0; w < (int)(sizeof(xyzz_t) / 4); ++w) aw[w] = __hip_atomic_load(pw + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      s[k] = acc;
    }
    __syncthreads();
    int top = 1;
    const int live = (int)gridDim.x < 128 ? (int)gridDim.x : 128;  // (the launcher keeps gridDim.x within OB_WALK_MAX_BLOCKS)
    while (2 * top < live) top <<= 1;
    for (int off = top; off >= 1; off >>= 1) {
      const bool active = k < off;
      xyzz_add_block4<128>(L, &s[k], &s[active ? k + off : k], s, role, k, active);
    }
    if (threadIdx.x == 0) atomicExch(ticket, 0u);  // ready for the next launch (stream order makes it visible)
  }
  if (threadIdx.x == 0) out[v] = xyzz_to_jac(s[0]);
}

// grid (ceil(cols / 256), count): z[k][i] = r_k lz_k[i] + d[k][i]
__global__ void __launch_bounds__(OB_STREAM_THREADS) k_ob_z(const ObInst* __restrict__ inst, ObChallenges ch, unsigned cols, const fe_t* __restrict__ d,
                                                            fe_t* __restrict__ z) {
  const unsigned i = blockIdx.x * OB_STREAM_THREADS + threadIdx.x;
  if (i >= cols) return;
  const size_t at = (size_t)blockIdx.y * cols + i;
  z[at] = fe_add<SF>(fe_mul<SF>(ch.r[blockIdx.y], inst[blockIdx.y].lz[i]), d[at]);
}

}  // namespace spk
