// sp_shape_from_wire's FULL device decode (capi_sparse.hip, SP_SHAPE_WIRE_FULL_DEVICE): filtered[m] and the column-major col[m] of sp_shape_from_csr built from
// what the row decode (kernels_wire_decode.hpp) left on the device - the class code and the narrowed column of every entry, the row pointers, the raw
// coefficients. Plain launches on the context's stream, blockIdx.y = the matrix, no block waits for another inside a launch; the three scan kernels of the
// row decode are used as they are (a WireArgs whose sptr / gptr point at the arrays to scan).
//   k_full_filt_counts   one lane a row: the row number of each of its entries (row32), and its small / general counts among the entries the filter keeps
//                        (row < row_limit, column >= col_min); the longest filtered row
//   k_full_filt_scatter  one lane a row: the kept entries in their own order (k_wire_scatter with the predicate)
//   k_full_col_counts    one lane an entry of the rows below row_limit: one integer atomic add on its column's counter of its class (a sum: the result
//                        does not depend on the order of arrival). The host reads the six counters a column back and decides the walk order (O(columns)).
//   k_full_col_place     one lane a column: its counts to its WALK POSITION pos[column] in the column pointer arrays, which the scan kernels then sum
//   k_full_sort_hist / k_full_sort_scatter   a stable least-significant-digit radix sort of the entry numbers by walk position, FULL_SORT_BITS bits a pass,
//                        the two classes as two sequences (small entries in [0, n_small), general ones behind them). A tile of FULL_SORT_TILE elements a block,
//                        a contiguous run of it a wave, 64 consecutive elements a round: an element's rank among the equal digits of its tile is the count of
//                        its wave's earlier rounds (an LDS counter only that wave touches) plus the equal digits in lower lanes of its round (nine __ballot
//                        over the 64 lanes), plus the totals of the waves before it; the tile's offset comes from the scanned per-tile histograms. So equal
//                        keys keep the order of the input: inside a column the entries stay in ascending entry number, as build_split leaves them.
//   k_full_col_scatter   one lane a SORTED element: its index in the sorted sequence is its index in sidx / scode (or, less n_small, in gidx / gval) - a
//                        column with hundreds of thousands of entries is written by as many lanes
// Bounds: indptr, data and idx are the arrays wire_parse_shape checked; code, idx32 and row32 hold nnz elements; n_used = indptr[row_limit] <= nnz; every
// column read from idx32 is below cols (k_wire_entries clamps an offender to 0 and the call is refused before these kernels run); pos[] is a permutation of
// [0, cols) made by the host; a sort destination is below n_used because histogram and scatter classify the same elements the same way.
#pragma once

namespace spk {

constexpr unsigned FULL_SORT_BITS = 8;     // digit width of the radix sort
constexpr unsigned FULL_SORT_BINS = 256;   // 1 << FULL_SORT_BITS
constexpr unsigned FULL_SORT_ITEMS = 8;    // elements a lane owns in a tile = rounds of its wave
constexpr unsigned FULL_SORT_TILE = 2048;  // elements a block owns (WIRE_BLOCK * FULL_SORT_ITEMS)
constexpr unsigned FULL_SORT_WAVES = WIRE_BLOCK / 64;
static_assert(FULL_SORT_BINS == 1u << FULL_SORT_BITS && FULL_SORT_TILE == WIRE_BLOCK * FULL_SORT_ITEMS, "a sort tile is one block's elements");
static_assert(2 * FULL_SORT_BINS == 2 * WIRE_BLOCK, "k_full_sort_scatter: a thread owns one bin of each class");

struct FullArgs {
  unsigned* row32[3];        // [nnz] out of k_full_filt_counts
  unsigned n_used[3];        // entries of the rows below row_limit: indptr[row_limit]
  unsigned* col_cnt;         // [3][2][cols]: small / general entries of each column among them
  const unsigned* pos;       // [cols]: walk position of each column
  unsigned long long row_limit, col_min, cols;
};

__global__ void __launch_bounds__(WIRE_BLOCK) k_full_filt_counts(WireArgs a, WireArgs f, FullArgs x, size_t rows) {
  const int which = blockIdx.y;
  const WireMat m = a.m[which];
  unsigned* row32 = x.row32[which];
  unsigned longest = 0;
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long lo = m.indptr[r], hi = m.indptr[r + 1];
    const bool used = r < x.row_limit;
    unsigned small = 0, general = 0;
    for (unsigned long long e = lo; e < hi; ++e) {
      row32[e] = (unsigned)r;
      if (used && m.idx32[e] >= x.col_min) {
        if (m.code[e] != 0) ++small;
        else ++general;
      }
    }
    f.m[which].sptr[r] = small;
    f.m[which].gptr[r] = general;
    longest = max(longest, small + general);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) longest = max(longest, (unsigned)__shfl_xor((int)longest, o));
  if ((threadIdx.x & 63u) == 0 && longest) atomicMax(f.max_len + which, longest);
}

__global__ void __launch_bounds__(WIRE_BLOCK) k_full_filt_scatter(WireArgs a, WireArgs f, WireOutArgs out, FullArgs x, size_t rows) {
  const int which = blockIdx.y;
  const WireMat m = a.m[which];
  const WireOut o = out.o[which];
  const size_t limit = x.row_limit < rows ? (size_t)x.row_limit : rows;
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < limit; r += (size_t)gridDim.x * blockDim.x) {
    unsigned ps = f.m[which].sptr[r], pg = f.m[which].gptr[r];
    for (unsigned long long e = m.indptr[r], hi = m.indptr[r + 1]; e < hi; ++e) {
      const unsigned col = m.idx32[e];
      if (col < x.col_min) continue;
      const int code = m.code[e];
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

__global__ void __launch_bounds__(WIRE_BLOCK) k_full_col_counts(WireArgs a, FullArgs x) {
  const int which = blockIdx.y;
  const WireMat m = a.m[which];
  const size_t n = x.n_used[which];
  unsigned* cnt = x.col_cnt + (size_t)(2 * which) * x.cols;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x)
    atomicAdd(cnt + (m.code[e] != 0 ? 0 : x.cols) + m.idx32[e], 1u);
}

__global__ void __launch_bounds__(WIRE_BLOCK) k_full_col_place(FullArgs x, WireArgs cp) {
  const int which = blockIdx.y;
  const unsigned* cnt = x.col_cnt + (size_t)(2 * which) * x.cols;
  for (size_t col = (size_t)blockIdx.x * blockDim.x + threadIdx.x; col < x.cols; col += (size_t)gridDim.x * blockDim.x) {
    const unsigned at = x.pos[col];
    cp.m[which].sptr[at] = cnt[col];
    cp.m[which].gptr[at] = cnt[x.cols + col];
  }
}

struct SortMat {
  const unsigned *keys_in, *vals_in;  // [n] (passes after the first)
  unsigned *keys_out, *vals_out;      // [n]
  unsigned* hist_s;                   // [FULL_SORT_BINS][ntiles] (+ 1): counts, then (scanned in place) offsets inside the small sequence
  unsigned* hist_g;                   // the same for the general sequence, which starts at n_small
  unsigned n, n_small;
};
struct SortArgs {
  SortMat m[3];
  unsigned ntiles;  // of the longest of the three sequences: the histograms of all three have this many columns
};

// element i of the pass's input: its key (walk position of its column), its value (entry number) and its bin = class * FULL_SORT_BINS + digit
template <bool FIRST>
__device__ __forceinline__ void full_sort_load(const WireMat& w, const SortMat& m, const unsigned* pos, unsigned i, unsigned shift, unsigned* key, unsigned* val,
                                               unsigned* bin) {
  unsigned cls;
  if (FIRST) {
    *key = pos[w.idx32[i]];
    *val = i;
    cls = w.code[i] != 0 ? 0u : 1u;
  } else {
    *key = m.keys_in[i];
    *val = m.vals_in[i];
    cls = i >= m.n_small ? 1u : 0u;
  }
  *bin = cls * FULL_SORT_BINS + ((*key >> shift) & (FULL_SORT_BINS - 1));
}

template <bool FIRST>
__global__ void __launch_bounds__(WIRE_BLOCK) k_full_sort_hist(WireArgs a, FullArgs x, SortArgs s, unsigned shift) {
  __shared__ unsigned hist[2 * FULL_SORT_BINS];
  const int which = blockIdx.y;
  const SortMat m = s.m[which];
  hist[threadIdx.x] = 0;
  hist[threadIdx.x + WIRE_BLOCK] = 0;
  __syncthreads();
  const unsigned long long base = (unsigned long long)blockIdx.x * FULL_SORT_TILE;  // (64 bits: a tile may end past 2^32)
#pragma unroll
  for (unsigned j = 0; j < FULL_SORT_ITEMS; ++j) {
    const unsigned long long i = base + j * WIRE_BLOCK + threadIdx.x;
    if (i < m.n) {
      unsigned key, val, bin;
      full_sort_load<FIRST>(a.m[which], m, x.pos, (unsigned)i, shift, &key, &val, &bin);
      atomicAdd(&hist[bin], 1u);
    }
  }
  __syncthreads();
  m.hist_s[(size_t)threadIdx.x * s.ntiles + blockIdx.x] = hist[threadIdx.x];
  m.hist_g[(size_t)threadIdx.x * s.ntiles + blockIdx.x] = hist[FULL_SORT_BINS + threadIdx.x];
}

template <bool FIRST>
__global__ void __launch_bounds__(WIRE_BLOCK) k_full_sort_scatter(WireArgs a, FullArgs x, SortArgs s, unsigned shift) {
  __shared__ unsigned cnt[FULL_SORT_WAVES][2 * FULL_SORT_BINS];
  const int which = blockIdx.y;
  const SortMat m = s.m[which];
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
  for (unsigned w = 0; w < FULL_SORT_WAVES; ++w) {
    cnt[w][threadIdx.x] = 0;
    cnt[w][threadIdx.x + WIRE_BLOCK] = 0;
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long base = (unsigned long long)blockIdx.x * FULL_SORT_TILE + wave * (FULL_SORT_ITEMS * 64u);
  unsigned key[FULL_SORT_ITEMS], val[FULL_SORT_ITEMS], bin[FULL_SORT_ITEMS], rank[FULL_SORT_ITEMS];
#pragma unroll
  for (unsigned j = 0; j < FULL_SORT_ITEMS; ++j) {  // (every lane of the wave runs every round: the ballots and the shuffle need all 64)
    const unsigned long long i = base + j * 64u + lane;
    const bool valid = i < m.n;
    key[j] = val[j] = bin[j] = 0;
    if (valid) full_sort_load<FIRST>(a.m[which], m, x.pos, (unsigned)i, shift, &key[j], &val[j], &bin[j]);
    unsigned long long same = __ballot(valid);  // the valid lanes of this round whose bin is this lane's
#pragma unroll
    for (unsigned b = 0; b <= FULL_SORT_BITS; ++b) {
      const bool bit = (bin[j] >> b) & 1u;
      const unsigned long long with = __ballot(valid && bit);
      same &= bit ? with : ~with;
    }
    const unsigned leader = valid ? (unsigned)(__ffsll((long long)same) - 1) : lane;
    unsigned before = 0;
    if (valid && leader == lane) before = atomicAdd(&cnt[wave][bin[j]], (unsigned)__popcll(same));  // (only this wave adds to its row: the sum of its earlier rounds)
    before = (unsigned)__shfl((int)before, (int)leader);
    rank[j] = before + (unsigned)__popcll(same & below);
  }
  __syncthreads();
  // the waves' totals of a bin become each wave's first destination of that bin: the tile's offset, then the waves before it
#pragma unroll
  for (unsigned cls = 0; cls < 2; ++cls) {
    const unsigned b = cls * FULL_SORT_BINS + threadIdx.x;
    unsigned at = (cls ? m.n_small + m.hist_g[(size_t)threadIdx.x * s.ntiles + blockIdx.x] : m.hist_s[(size_t)threadIdx.x * s.ntiles + blockIdx.x]);
#pragma unroll
    for (unsigned w = 0; w < FULL_SORT_WAVES; ++w) {
      const unsigned t = cnt[w][b];
      cnt[w][b] = at;
      at += t;
    }
  }
  __syncthreads();
#pragma unroll
  for (unsigned j = 0; j < FULL_SORT_ITEMS; ++j) {
    if (base + j * 64u + lane < m.n) {
      const unsigned dst = cnt[wave][bin[j]] + rank[j];
      if (dst < m.n) {  // (always: see the header; a store never leaves the buffer)
        m.keys_out[dst] = key[j];
        m.vals_out[dst] = val[j];
      }
    }
  }
}

struct ColOutArgs {
  WireOut o[3];
  const unsigned* sorted[3];  // [n_used]: entry numbers, small sequence then general, each by walk position and entry number
  unsigned n_small[3];
};
__global__ void __launch_bounds__(WIRE_BLOCK) k_full_col_scatter(WireArgs a, FullArgs x, ColOutArgs c) {
  const int which = blockIdx.y;
  const WireMat m = a.m[which];
  const WireOut o = c.o[which];
  const unsigned* row32 = x.row32[which];
  const size_t n = x.n_used[which], ns = c.n_small[which];
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
    const unsigned e = c.sorted[which][k];
    if (e >= n) continue;  // (never: the values are a permutation of [0, n))
    if (k < ns) {
      o.sidx[k] = row32[e];
      o.scode[k] = m.code[e];
    } else {
      o.gidx[k - ns] = row32[e];
      o.gval[k - ns] = fe_from_canonical<S>(wire_load_coeff(m.data, e));
    }
  }
}

}  // namespace spk
