// sp_shape_from_wire's device decode (capi_sparse.hip): the row-major split structure row[m] (sptr / sidx / scode, gptr / gidx / gval) of A, B, C built
// from the bincode bytes of SparseMatrix { data, indices, indptr } (src/r1cs/sparse.rs:383-394) as they were uploaded - 32 canonical little-endian bytes a
// coefficient, 8 bytes an index, 8 bytes a row pointer. Five plain launches, blockIdx.y = the matrix, nothing waits for another block inside a launch:
//   k_wire_entries      one lane an entry: coefficient below the modulus, index below `cols` (the first offender of each kind goes into a status word with
//                       an atomic minimum), the class code as Classifier::code gives it (+-k for the canonical value k or q - k, k = 1 .. 7, else 0), the
//                       index narrowed to 32 bits
//   k_wire_row_counts   one lane a row: its small and general entry counts; the longest row (max_len picks k_spmv3's form)
//   k_wire_scan_reduce / k_wire_scan_blocks / k_wire_scan_add   exclusive scan of both counts over all rows: per-tile sums, one block scans the sums, per-tile
//                       scan plus the tile's offset - in place, counts in, row pointers out
//   k_wire_scatter      one lane a row: its entries in their own order into sidx / scode and gidx / gval; a general coefficient becomes Montgomery limbs here
// The host has checked, before the first launch, everything a kernel dereferences through: indptr has rows + 1 entries, starts at 0, never decreases and
// ends at nnz < 2^32; data and indices hold nnz elements each. A kernel reads entries [indptr[r], indptr[r + 1]) of arrays that long and nothing else.
#pragma once

namespace spk {

constexpr unsigned WIRE_BLOCK = 256;      // threads of every kernel here; the entry, row and scatter kernels stride a capped grid of such blocks
constexpr unsigned WIRE_SCAN_ITEMS = 4;   // rows a thread of the scan kernels owns
constexpr unsigned WIRE_SCAN_TILE = 1024; // rows a block of the scan kernels owns (WIRE_BLOCK * WIRE_SCAN_ITEMS)
static_assert(WIRE_SCAN_TILE == WIRE_BLOCK * WIRE_SCAN_ITEMS, "a scan tile is one block's rows");
constexpr unsigned long long WIRE_STATUS_OK = ~0ull;

struct WireMat {
  const uint4* data;                 // [2 nnz]: 32 bytes a coefficient (16-byte aligned: the upload places it)
  const unsigned long long* idx;     // [nnz]
  const unsigned long long* indptr;  // [rows + 1], checked by the host
  unsigned long long nnz;
  signed char* code;                 // [nnz] out of k_wire_entries
  unsigned* idx32;                   // [nnz] out of k_wire_entries
  unsigned* sptr;                    // [rows + 1]: counts, then (in place) offsets
  unsigned* gptr;
};
struct WireArgs {
  WireMat m[3];
  unsigned long long cols;
  unsigned long long* status;  // [3][2]: first non-canonical coefficient, first index out of range (WIRE_STATUS_OK = none)
  unsigned* max_len;           // [3]
  unsigned* block_sums;        // [3][2][nblk]
  unsigned* totals;            // [3][2]
  unsigned nblk;               // scan tiles: ceil(rows / WIRE_SCAN_TILE)
};
struct WireOut {
  unsigned* sidx;
  signed char* scode;
  unsigned* gidx;
  fe_t* gval;
};
struct WireOutArgs {
  WireOut o[3];
};

__device__ __forceinline__ fe_t wire_load_coeff(const uint4* data, size_t e) {
  const uint4 lo = data[2 * e], hi = data[2 * e + 1];
  fe_t c;
  c.v[0] = lo.x, c.v[1] = lo.y, c.v[2] = lo.z, c.v[3] = lo.w;
  c.v[4] = hi.x, c.v[5] = hi.y, c.v[6] = hi.z, c.v[7] = hi.w;
  return c;
}
__device__ __forceinline__ bool wire_below_modulus(const fe_t& c) {
  bool below = false, decided = false;
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    const unsigned p = S::P(i);
    if (!decided && c.v[i] != p) {
      below = c.v[i] < p;
      decided = true;
    }
  }
  return below;  // (equal to the modulus: not canonical)
}
// Classifier::code on the canonical value: k or q - k for k = 1 .. 7
__device__ __forceinline__ int wire_code(const fe_t& c) {
  unsigned hi = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i) hi |= c.v[i];
  if (hi == 0) return c.v[0] >= 1 && c.v[0] <= 7 ? (int)c.v[0] : 0;
  // d = q - c (c is below q): -k exactly when d = k
  unsigned borrow = 0, dhi = 0, d0 = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned long long t = (unsigned long long)S::P(i) - c.v[i] - borrow;
    borrow = (unsigned)(t >> 63);
    if (i == 0) d0 = (unsigned)t;
    else dhi |= (unsigned)t;
  }
  return dhi == 0 && d0 >= 1 && d0 <= 7 ? -(int)d0 : 0;
}

__global__ void __launch_bounds__(WIRE_BLOCK) k_wire_entries(WireArgs a) {
  const int which = blockIdx.y;
  const WireMat m = a.m[which];
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < m.nnz; e += (size_t)gridDim.x * blockDim.x) {
    const fe_t c = wire_load_coeff(m.data, e);
    const unsigned long long col = m.idx[e];
    int code = 0;
    if (!wire_below_modulus(c)) atomicMin(a.status + 2 * which, (unsigned long long)e);
    else code = wire_code(c);
    if (col >= a.cols) atomicMin(a.status + 2 * which + 1, (unsigned long long)e);
    m.code[e] = (signed char)code;
    m.idx32[e] = col < a.cols ? (unsigned)col : 0u;
  }
}

__global__ void __launch_bounds__(WIRE_BLOCK) k_wire_row_counts(WireArgs a, size_t rows) {
  const int which = blockIdx.y;
  const WireMat m = a.m[which];
  unsigned longest = 0;
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long lo = m.indptr[r], hi = m.indptr[r + 1];
    unsigned small = 0;
    for (unsigned long long e = lo; e < hi; ++e) small += m.code[e] != 0 ? 1u : 0u;
    m.sptr[r] = small;
    m.gptr[r] = (unsigned)(hi - lo) - small;
    longest = max(longest, (unsigned)(hi - lo));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) longest = max(longest, (unsigned)__shfl_xor((int)longest, o));
  if ((threadIdx.x & 63u) == 0 && longest) atomicMax(a.max_len + which, longest);
}

// exclusive scan of one value a thread over the block (Hillis-Steele in LDS); *total = the block's sum
__device__ __forceinline__ unsigned wire_block_scan(unsigned v, unsigned* smem, unsigned* total) {
  const unsigned t = threadIdx.x;
  smem[t] = v;
  __syncthreads();
  for (unsigned off = 1; off < WIRE_BLOCK; off <<= 1) {
    const unsigned add = t >= off ? smem[t - off] : 0u;
    __syncthreads();
    smem[t] += add;
    __syncthreads();
  }
  const unsigned incl = smem[t];
  *total = smem[WIRE_BLOCK - 1];
  __syncthreads();  // smem is reused by the caller's next scan
  return incl - v;
}

__global__ void __launch_bounds__(WIRE_BLOCK) k_wire_scan_reduce(WireArgs a, size_t rows) {
  __shared__ unsigned smem[WIRE_BLOCK];
  const int which = blockIdx.y;
  const WireMat m = a.m[which];
  const size_t r0 = (size_t)blockIdx.x * WIRE_SCAN_TILE + (size_t)threadIdx.x * WIRE_SCAN_ITEMS;
  unsigned s = 0, g = 0;
#pragma unroll
  for (unsigned j = 0; j < WIRE_SCAN_ITEMS; ++j)
    if (r0 + j < rows) s += m.sptr[r0 + j], g += m.gptr[r0 + j];
  unsigned total;
  wire_block_scan(s, smem, &total);
  if (threadIdx.x == 0) a.block_sums[(size_t)(2 * which) * a.nblk + blockIdx.x] = total;
  wire_block_scan(g, smem, &total);
  if (threadIdx.x == 0) a.block_sums[(size_t)(2 * which + 1) * a.nblk + blockIdx.x] = total;
}

// one block a matrix: the tile sums become tile offsets, the grand totals go to a.totals
__global__ void __launch_bounds__(WIRE_BLOCK) k_wire_scan_blocks(WireArgs a) {
  __shared__ unsigned smem[WIRE_BLOCK];
  const int which = blockIdx.y;
  for (int cls = 0; cls < 2; ++cls) {
    unsigned* bs = a.block_sums + (size_t)(2 * which + cls) * a.nblk;
    unsigned carry = 0;
    for (unsigned base = 0; base < a.nblk; base += WIRE_BLOCK) {  // (uniform over the block)
      const unsigned i = base + threadIdx.x;
      const unsigned v = i < a.nblk ? bs[i] : 0u;
      unsigned total;
      const unsigned excl = wire_block_scan(v, smem, &total);
      if (i < a.nblk) bs[i] = carry + excl;
      carry += total;
    }
    if (threadIdx.x == 0) a.totals[2 * which + cls] = carry;
  }
}

__global__ void __launch_bounds__(WIRE_BLOCK) k_wire_scan_add(WireArgs a, size_t rows) {
  __shared__ unsigned smem[WIRE_BLOCK];
  const int which = blockIdx.y;
  const WireMat m = a.m[which];
  const size_t r0 = (size_t)blockIdx.x * WIRE_SCAN_TILE + (size_t)threadIdx.x * WIRE_SCAN_ITEMS;
  for (int cls = 0; cls < 2; ++cls) {
    unsigned* ptr = cls ? m.gptr : m.sptr;
    unsigned v[WIRE_SCAN_ITEMS], sum = 0;
#pragma unroll
    for (unsigned j = 0; j < WIRE_SCAN_ITEMS; ++j) {
      v[j] = r0 + j < rows ? ptr[r0 + j] : 0u;
      sum += v[j];
    }
    unsigned total;
    unsigned at = a.block_sums[(size_t)(2 * which + cls) * a.nblk + blockIdx.x] + wire_block_scan(sum, smem, &total);
#pragma unroll
    for (unsigned j = 0; j < WIRE_SCAN_ITEMS; ++j)
      if (r0 + j < rows) {
        ptr[r0 + j] = at;
        at += v[j];
      }
    if (blockIdx.x == 0 && threadIdx.x == 0) ptr[rows] = a.totals[2 * which + cls];
  }
}

__global__ void __launch_bounds__(WIRE_BLOCK) k_wire_scatter(WireArgs a, WireOutArgs out, size_t rows) {
  const int which = blockIdx.y;
  const WireMat m = a.m[which];
  const WireOut o = out.o[which];
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (size_t)gridDim.x * blockDim.x) {
    unsigned ps = m.sptr[r], pg = m.gptr[r];
    for (unsigned long long e = m.indptr[r], hi = m.indptr[r + 1]; e < hi; ++e) {
      const int code = m.code[e];
      const unsigned col = m.idx32[e];
      if (code) {
        o.sidx[ps] = col;
        o.scode[ps++] = (signed char)code;
      } else {
        o.gidx[pg] = col;
        o.gval[pg++] = fe_from_canonical<S>(wire_load_coeff(m.data, e));
      }
    }
  }
}

}  // namespace spk
