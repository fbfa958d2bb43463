// libspartan_hip.so — R1CS sparse kernels and entry points of include/spartan_hip.h.
//   k_spmv3     K5/K6  PrecomputedSparseMatrix::multiply_vec (src/r1cs/sparse.rs:194-233) for A, B, C in one launch, and
//                      multiply_vec_incremental_into (src/r1cs/mod.rs:1170-1211) = cached + filtered rows (sparse.rs:305-380)
//   k_polyabc*  K7     bind_and_prepare_poly_ABC / accumulate_rows (src/r1cs/mod.rs:1235-1398) as a column-major GATHER
//                      (no 256-bit atomics): short columns one lane each, long columns (the constant-1 column of the
//                      booleanity rows) one block each.
//   k_matrix_evals_batched  evaluate_with_tables_fast (src/r1cs/mod.rs:1216-1226) for a chunk of (T_x, T_y) pairs in one walk (kernels_mateval.hpp)
//   k_spmv3_multi      multiply_vec_batched (sparse.rs:237-302) for a chunk of vectors in one walk (kernels_spmv_multi.hpp)
//   k_nifs_layers      cached_step_matvec (src/neutronnova_zk.rs:1520-1600): (A, B, C) [W | 1 | X] of every instance of every state into its NIFS
//                      layers in one launch, z never assembled (kernels_nifs_layers.hpp; the entry is sp_nifs_layers_batch, capi_nifs.hip)
//   k_pab_*            evals_rx + poly_ABC (src/polys/eq.rs:59-117, src/r1cs/mod.rs:1235-1321) for a chunk of proofs in one walk over interleaved eq tables (kernels_polyabc_batch.hpp)
//   k_full_*           sp_shape_from_wire's full device decode: filtered[] and the column-major col[] of sp_shape_from_csr from the uploaded bytes - column counters, a stable
//                      radix sort of the entry numbers by walk position, one lane a sorted entry (kernels_wire_full.hpp)
//   k_r1cs_residual    R1CSShape::is_sat / is_sat_relaxed (src/r1cs/mod.rs:358-394, :430-471): the row check behind multiply_vec (kernels_sat.hpp)
// Entries keep the reference's classes: +-1 and |k| in 2..7 as an int8 code (add / sub / double-add chains, sparse.rs:137-155),
// everything else as a full field coefficient.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "core.hpp"
#include "device_utils.hpp"
#include "kernels_sat.hpp"

using sp::fail;
typedef FqP S;

namespace spk {

struct SplitDev {          // major-ordered sparse structure, entries split by coefficient class
  const unsigned* sptr;    // [n_major + 1] small-class offsets
  const unsigned* sidx;    // minor index of each small-class entry
  const signed char* scode;  // +-1 .. +-7
  const unsigned* gptr;    // [n_major + 1] general-class offsets
  const unsigned* gidx;
  const fe_t* gval;
};

__device__ __forceinline__ fe_t small_mul(int code, const fe_t& x) {  // sparse.rs:137-155
  const int a = code < 0 ? -code : code;
  fe_t r;
  switch (a) {
    case 1: r = x; break;
    case 2: r = fe_dbl<S>(x); break;
    case 3: r = fe_add<S>(fe_dbl<S>(x), x); break;
    case 4: r = fe_dbl<S>(fe_dbl<S>(x)); break;
    case 5: r = fe_add<S>(fe_dbl<S>(fe_dbl<S>(x)), x); break;
    case 6: { fe_t d = fe_dbl<S>(x); r = fe_add<S>(fe_dbl<S>(d), d); break; }
    default: { fe_t d = fe_dbl<S>(x); r = fe_add<S>(fe_add<S>(fe_dbl<S>(d), d), x); break; }
  }
  return r;
}
__device__ __forceinline__ fe_t acc_small(const fe_t& acc, int code, const fe_t& x) {
  if (code == 1) return fe_add<S>(acc, x);
  if (code == -1) return fe_sub<S>(acc, x);
  fe_t m = small_mul(code, x);
  return code < 0 ? fe_sub<S>(acc, m) : fe_add<S>(acc, m);
}
// sum over the entries of one major index, strided (first, step) so a block can share a long list
__device__ __forceinline__ fe_t gather_major(const SplitDev& m, size_t major, const fe_t* __restrict__ x, unsigned first, unsigned step) {
  fe_t acc = fe_zero();
  for (unsigned k = m.sptr[major] + first, e = m.sptr[major + 1]; k < e; k += step) acc = acc_small(acc, m.scode[k], x[m.sidx[k]]);
  for (unsigned k = m.gptr[major] + first, e = m.gptr[major + 1]; k < e; k += step) acc = fe_add<S>(acc, fe_mul<S>(m.gval[k], x[m.gidx[k]]));
  return acc;
}

// The same sum with FOUR entries in flight: index / code loads first, then the four gathers, then the four accumulations. One lane walking a
// column otherwise pays two dependent memory latencies (index, then x[index]) per entry, and the column kernels are bound by exactly that chain
// (k_polyabc_short: 82 us for 5 M entries at config 2, nowhere near a bandwidth limit).
__device__ __forceinline__ fe_t gather_major_x4(const SplitDev& m, size_t major, const fe_t* __restrict__ x) {
  fe_t acc = fe_zero();
  unsigned k = m.sptr[major];
  const unsigned e = m.sptr[major + 1];
  for (; k + 4 <= e; k += 4) {
    const unsigned i0 = m.sidx[k], i1 = m.sidx[k + 1], i2 = m.sidx[k + 2], i3 = m.sidx[k + 3];
    const int c0 = m.scode[k], c1 = m.scode[k + 1], c2 = m.scode[k + 2], c3 = m.scode[k + 3];
    const fe_t x0 = x[i0], x1 = x[i1], x2 = x[i2], x3 = x[i3];
    acc = acc_small(acc, c0, x0);
    acc = acc_small(acc, c1, x1);
    acc = acc_small(acc, c2, x2);
    acc = acc_small(acc, c3, x3);
  }
  if (k + 2 <= e) {
    const unsigned i0 = m.sidx[k], i1 = m.sidx[k + 1];
    const int c0 = m.scode[k], c1 = m.scode[k + 1];
    const fe_t x0 = x[i0], x1 = x[i1];
    acc = acc_small(acc, c0, x0);
    acc = acc_small(acc, c1, x1);
    k += 2;
  }
  if (k < e) acc = acc_small(acc, m.scode[k], x[m.sidx[k]]);
  for (unsigned g = m.gptr[major], ge = m.gptr[major + 1]; g < ge; ++g) acc = fe_add<S>(acc, fe_mul<S>(m.gval[g], x[m.gidx[g]]));
  return acc;
}

struct Spmv3Args {
  SplitDev m[3];
  const fe_t* base[3];  // cached products to add (nullptr for a plain multiply_vec)
  fe_t* out[3];
};
// One lane per row, four entries in flight (gather_major_x4). A row longer than SPMV_LONG_ROW entries - the 32-bit additions of a SHA-256 round: ~6000 rows of
// 33 .. 225 entries among 880 K of one to three at config 2 - would keep its wave waiting on one lane's chain of dependent (index, then element) loads
// (the per-wave longest rows of A sum to 958 K such steps against 2 M entries in all: 0.75 ms for the cached product of prep_prove): those are walked by
// the whole wave, an entry per lane, and added with a shuffle tree; the owner lane keeps the sum.
// LONG_ROWS = false (no row of any of the three structures is longer than SPMV_LONG_ROW - the filtered rows of the incremental product inside a prove): the
// plain lane-per-row walk at 64 registers; the cooperative form needs 116 and halves the waves per SIMD of what is then a streaming kernel (62 vs 42 us).
constexpr unsigned SPMV_LONG_ROW = 24;
template <bool LONG_ROWS>
__global__ void __launch_bounds__(256) k_spmv3(Spmv3Args a, const fe_t* __restrict__ z, size_t nrows) {
  const int which = blockIdx.y;
  const SplitDev m = a.m[which];
  const fe_t* base = a.base[which];
  fe_t* out = a.out[which];
  if (!LONG_ROWS) {
    for (size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x; row < nrows; row += (size_t)gridDim.x * blockDim.x) {
      fe_t acc = gather_major(m, row, z, 0, 1);
      if (base) acc = fe_add<S>(acc, base[row]);
      out[row] = acc;
    }
    return;
  }
  const unsigned lane = threadIdx.x & 63u;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t wbase = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); wbase < nrows; wbase += stride) {  // (uniform over a wave)
    const size_t row = wbase + lane;
    const bool valid = row < nrows;
    bool is_long = false;
    fe_t acc = fe_zero();
    if (valid) {
      is_long = (m.sptr[row + 1] - m.sptr[row]) + (m.gptr[row + 1] - m.gptr[row]) > SPMV_LONG_ROW;
      if (!is_long) acc = gather_major_x4(m, row, z);
    }
    unsigned long long pending = __ballot(is_long);
    while (pending) {
      const int owner = __ffsll((long long)pending) - 1;
      pending &= pending - 1;
      const size_t r = wbase + (size_t)owner;
      const fe_t part = wave_sum(gather_major(m, r, z, lane, 64));
      if ((int)lane == owner) acc = part;
    }
    if (valid) {
      if (base) acc = fe_add<S>(acc, base[row]);
      out[row] = acc;
    }
  }
}

// The tau-independent halves of the outer sum-check's FIRST evaluation (evaluation_points_cubic_with_three_inputs, src/sumcheck.rs:1041-1105), formed
// right behind the matrix-vector product while both run in the shadow of commit_zeros: P0[i] = A0 B0 - C0, P1[i] = (A1 - A0)(B1 - B0) for the pair
// (i, i + N/2) the top variable joins (src/polys/multilinear.rs:101). The first evaluation on the critical path then reads 2 x 16 MiB instead of
// 84 MiB. (A fused form — one thread computing both rows of all three products — was measured: its six row walks per thread cost more than this
// second streaming pass, 116 us against 50 + 25 us.)
__global__ void __launch_bounds__(256) k_round0_products(const fe_t* __restrict__ A, const fe_t* __restrict__ B, const fe_t* __restrict__ C, size_t half,
                                                         fe_t* __restrict__ p0, fe_t* __restrict__ p1) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += (size_t)gridDim.x * blockDim.x) {
    const fe_t a0 = A[i], a1 = A[i + half], b0 = B[i], b1 = B[i + half], c0 = C[i];
    p0[i] = fe_sub<S>(fe_mul<S>(a0, b0), c0);
    p1[i] = fe_mul<S>(fe_sub<S>(a1, a0), fe_sub<S>(b1, b0));
  }
}

struct PolyAbcArgs {
  SplitDev m[3];  // column-major A, B, C
  fe_t r, r2;
};
constexpr unsigned LONG_COLUMN = 512;
__device__ __forceinline__ unsigned col_len(const PolyAbcArgs& a, size_t col) {
  unsigned n = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) n += (a.m[i].sptr[col + 1] - a.m[i].sptr[col]) + (a.m[i].gptr[col + 1] - a.m[i].gptr[col]);
  return n;
}
// Long columns (the constant-1 column has ~one entry per booleanity row): NB blocks share a column, each striding
// over its entry lists; the column's last block to arrive adds the NB partial triples and applies (1, r, r^2).
constexpr unsigned LONG_NB_MAX = 128;
__device__ __forceinline__ unsigned long_nb(unsigned len) {
  unsigned nb = (len + 2047) / 2048;
  return nb < 1 ? 1 : (nb > LONG_NB_MAX ? LONG_NB_MAX : nb);
}
// accumulate_rows (src/r1cs/mod.rs:1324-1398) as a column-major gather in ONE launch: blocks [0, LONG_NB_MAX * n_long) are the long columns' (they are
// dispatched first and run under the short columns' blocks, off the path of the inner sum-check's first round), the next `short_blocks` walk the short
// columns — `order` lists them by decreasing entry count and, within one count, by their (A, B, C) entry counts, so the 64 columns of a wave run the same
// trip counts —, the last blocks of the grid write the output's zero tail. The last block of a long column to arrive (one counter per column, <= 128
// arrivals, partial triples stored write-through and read back past this XCD's L2) adds the column's partials and applies (1, r, r^2).
__global__ void __launch_bounds__(256) k_polyabc_short_and_long(PolyAbcArgs a, const fe_t* __restrict__ rx, const unsigned* __restrict__ order, size_t n_short,
                                                                fe_t* __restrict__ out, const unsigned* __restrict__ long_cols, unsigned n_long,
                                                                fe_t* __restrict__ partials, unsigned* __restrict__ tickets, unsigned short_blocks,
                                                                size_t zero_from, size_t zero_n, int permuted) {
  __shared__ fe_t smem[3 * 4];
  __shared__ unsigned s_last;
  const unsigned long_blocks = LONG_NB_MAX * n_long;
  if (blockIdx.x >= long_blocks + short_blocks) {
    // the zero tail of the output (out_len > num_cols: 32 MB at config 2, a 7 us fill launch in front of this kernel until round 3): the last blocks
    // of the grid stream it out under the column walks
    uint4* z = reinterpret_cast<uint4*>(out + zero_from);
    const size_t n16 = zero_n * 2, nb = gridDim.x - long_blocks - short_blocks;
    for (size_t i = (size_t)(blockIdx.x - long_blocks - short_blocks) * blockDim.x + threadIdx.x; i < n16; i += nb * blockDim.x) z[i] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  if (blockIdx.x < long_blocks) {
    const unsigned by = blockIdx.x / LONG_NB_MAX, bx = blockIdx.x % LONG_NB_MAX;
    const size_t col = long_cols[by];                       // the column's number: where its sum goes
    const size_t at = permuted ? n_short + by : col;        // ... and where the structure keeps it (walk order: the long columns behind the short ones)
    const unsigned nb = long_nb(col_len(a, at));
    if (bx >= nb) return;
    fe_t acc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] = gather_major(a.m[i], at, rx, bx * blockDim.x + threadIdx.x, nb * blockDim.x);
    block_sum<3>(acc, smem);
    fe_t* trip = partials + ((size_t)by * LONG_NB_MAX) * 3;
    if (threadIdx.x == 0) {
      unsigned* dst = reinterpret_cast<unsigned*>(trip + (size_t)bx * 3);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int w = 0; w < 8; ++w) __hip_atomic_store(dst + 8 * i + w, acc[i].v[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // release / acquire at agent scope on the ticket (a few hundred long-column blocks at most, all of them under the short columns' walk: the
      // L2 write-back a release costs does not matter here as it did in a thousand-block streaming launch)
      s_last = __hip_atomic_fetch_add(tickets + by, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nb - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      acc[i] = fe_zero();
      if (threadIdx.x < nb) {
        const unsigned* src = reinterpret_cast<const unsigned*>(trip + (size_t)threadIdx.x * 3 + i);
#pragma unroll
        for (int w = 0; w < 8; ++w) acc[i].v[w] = __hip_atomic_load(src + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();  // smem reuse
    block_sum<3>(acc, smem);
    if (threadIdx.x == 0) {
      __hip_atomic_store(tickets + by, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
      out[col] = fe_add<S>(fe_add<S>(acc[0], fe_mul<S>(a.r, acc[1])), fe_mul<S>(a.r2, acc[2]));
    }
    return;
  }
  const size_t nblk = short_blocks;
  for (size_t i = (size_t)(blockIdx.x - long_blocks) * blockDim.x + threadIdx.x; i < n_short; i += nblk * blockDim.x) {
    const size_t col = order[i], at = permuted ? i : col;
    fe_t sa = gather_major_x4(a.m[0], at, rx), sb = gather_major_x4(a.m[1], at, rx), sc = gather_major_x4(a.m[2], at, rx);
    if (!fe_is_zero(sb)) sa = fe_add<S>(sa, fe_mul<S>(a.r, sb));
    if (!fe_is_zero(sc)) sa = fe_add<S>(sa, fe_mul<S>(a.r2, sc));
    out[col] = sa;
  }
}
}  // namespace spk

#include "kernels_mateval.hpp"
#include "kernels_polyabc_batch.hpp"
#include "kernels_spmv_multi.hpp"
#include "kernels_nifs_layers.hpp"
#include "kernels_wire_decode.hpp"
#include "kernels_wire_full.hpp"

// ---- host side: classification and upload ---------------------------------------------------------------------------
namespace {

struct SplitHost {
  std::vector<unsigned> sptr, sidx, gptr, gidx;
  std::vector<signed char> scode;
  std::vector<fe_t> gval;
};
struct SplitOnDevice {
  unsigned *sptr = nullptr, *sidx = nullptr, *gptr = nullptr, *gidx = nullptr;
  signed char* scode = nullptr;
  fe_t* gval = nullptr;
  unsigned max_len = 0;  // longest major (entries of both classes): picks k_spmv3's form
  spk::SplitDev view() const { return spk::SplitDev{sptr, sidx, scode, gptr, gidx, gval}; }
  void release() {
    hipFree(sptr);
    hipFree(sidx);
    hipFree(gptr);
    hipFree(gidx);
    hipFree(scode);
    hipFree(gval);
  }
};

struct Classifier {  // from_sparse (sparse.rs:49-134)
  fe_t pos[8], neg[8];
  Classifier() {
    for (int k = 1; k <= 7; ++k) {
      pos[k] = fe_from_u64<S>(k);
      neg[k] = fe_neg<S>(pos[k]);
    }
  }
  int code(const fe_t& v) const {
    for (int k = 1; k <= 7; ++k) {
      if (fe_eq(v, pos[k])) return k;
      if (fe_eq(v, neg[k])) return -k;
    }
    return 0;
  }
};

template <class T>
int upload(T** dst, const std::vector<T>& src) {
  size_t bytes = (src.empty() ? 1 : src.size()) * sizeof(T);
  hipError_t e = hipMalloc((void**)dst, bytes);
  if (e != hipSuccess) return fail(SP_ERR_NO_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
  if (!src.empty()) e = hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(SP_ERR_NO_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
  return SP_OK;
}
int upload_split(const SplitHost& h, SplitOnDevice* d) {
  int rc;
  if ((rc = upload(&d->sptr, h.sptr))) return rc;
  if ((rc = upload(&d->sidx, h.sidx))) return rc;
  if ((rc = upload(&d->scode, h.scode))) return rc;
  if ((rc = upload(&d->gptr, h.gptr))) return rc;
  if ((rc = upload(&d->gidx, h.gidx))) return rc;
  d->max_len = 0;
  for (size_t i = 0; i + 1 < h.sptr.size(); ++i) {
    const unsigned l = (h.sptr[i + 1] - h.sptr[i]) + (h.gptr[i + 1] - h.gptr[i]);
    if (l > d->max_len) d->max_len = l;
  }
  return upload(&d->gval, h.gval);
}

struct Entry {
  unsigned major, minor;
  int code;
  fe_t val;
};
// build a major-ordered split structure from (major, minor) entries already grouped by major
SplitHost build_split(size_t n_major, const std::vector<Entry>& es) {
  SplitHost h;
  h.sptr.assign(n_major + 1, 0);
  h.gptr.assign(n_major + 1, 0);
  for (const Entry& e : es) (e.code ? h.sptr : h.gptr)[e.major + 1]++;
  for (size_t i = 0; i < n_major; ++i) {
    h.sptr[i + 1] += h.sptr[i];
    h.gptr[i + 1] += h.gptr[i];
  }
  h.sidx.resize(h.sptr[n_major]);
  h.scode.resize(h.sptr[n_major]);
  h.gidx.resize(h.gptr[n_major]);
  h.gval.resize(h.gptr[n_major]);
  std::vector<unsigned> sc(h.sptr.begin(), h.sptr.end() - 1), gc(h.gptr.begin(), h.gptr.end() - 1);
  for (const Entry& e : es) {
    if (e.code) {
      unsigned p = sc[e.major]++;
      h.sidx[p] = e.minor;
      h.scode[p] = (signed char)e.code;
    } else {
      unsigned p = gc[e.major]++;
      h.gidx[p] = e.minor;
      h.gval[p] = e.val;
    }
  }
  return h;
}

}  // namespace

struct sp_shape {
  sp_dims dims;
  size_t num_vars = 0, num_cols = 0;
  SplitOnDevice row[3];       // full CSR (multiply_vec)
  SplitOnDevice filtered[3];  // FilteredSpmv rows: col >= num_shared + num_precommitted, row < num_cons_unpadded
  SplitOnDevice col[3];       // column-major, rows < num_cons_unpadded (accumulate_rows)
  unsigned* d_long_cols = nullptr;
  unsigned* d_short_order = nullptr;  // short columns by decreasing entry count (k_polyabc_short_and_long)
  size_t n_short = 0;
  size_t n_long_cols = 0;
  bool col_permuted = false;  // col[] is stored in walk order: position i = d_short_order[i] for i < n_short, then the long columns
  uint64_t nnz[3] = {0, 0, 0}, nnz_filtered[3] = {0, 0, 0};
  bool row_only = false;  // sp_shape_from_wire's verifier form: row[] alone; filtered[], col[] and the walk order are absent (null)
};
// the entry points that walk filtered[] or col[] refuse a row-only shape before they touch either
static int refuse_row_only(const sp_shape* s, const char* who) {
  if (s && s->row_only) return fail(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": row-only shape (loaded by sp_shape_from_wire without SP_SHAPE_WIRE_FULL)");
  return SP_OK;
}

// The three settings of poly_ABC's column structure, read once (the window with every shape that takes it). sp_shape_from_csr and the full device decode
// of sp_shape_from_wire build under the same three.
static int polyabc_order_mode() {
  static const int order_mode = [] {
    const char* e = getenv("SPARTAN_POLYABC_ORDER");  // "natural": column order as it is; "window": sorted inside windows of 4096 neighbouring columns (A/B runs)
    return !e ? 0 : (e[0] == 'n' ? 1 : (e[0] == 'w' ? 2 : 0));
  }();
  return order_mode;
}
static size_t polyabc_window() {
  const char* w = getenv("SPARTAN_POLYABC_WINDOW");
  return w && atol(w) > 0 ? (size_t)atol(w) : 4096;
}
static bool polyabc_permuted() {
  static const bool permuted = [] {
    const char* e = getenv("SPARTAN_POLYABC_LAYOUT");
    return !(e && e[0] == 'n');
  }();
  return permuted;
}

extern "C" {

int sp_shape_from_csr(sp_ctx* c, const sp_csr* A, const sp_csr* Bm, const sp_csr* C, const sp_dims* dims, sp_shape** out) {
  (void)c;
  sp_shape* s = new sp_shape();
  s->dims = *dims;
  s->num_vars = dims->num_shared + dims->num_precommitted + dims->num_rest;
  s->num_cols = s->num_vars + 1 + dims->num_public + dims->num_challenges;
  const size_t nrows = dims->num_cons, col_min = dims->num_shared + dims->num_precommitted, nr_used = dims->num_cons_unpadded;
  const sp_csr* M[3] = {A, Bm, C};
  Classifier cls;
  std::vector<unsigned> col_count(s->num_cols, 0);
  std::vector<SplitHost> col_host(3);
  for (int m = 0; m < 3; ++m) {
    const size_t nnz = M[m]->indptr[nrows];
    s->nnz[m] = nnz;
    std::vector<Entry> all, filt, bycol;
    all.reserve(nnz);
    for (size_t r = 0; r < nrows; ++r) {
      for (uint64_t k = M[m]->indptr[r]; k < M[m]->indptr[r + 1]; ++k) {
        Entry e;
        e.major = (unsigned)r;
        e.minor = M[m]->indices[k];
        if (e.minor >= s->num_cols) {
          delete s;
          return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_csr: column index out of range");
        }
        memcpy(&e.val, M[m]->data + 4 * k, 32);
        e.code = cls.code(e.val);
        all.push_back(e);
        if (r < nr_used && e.minor >= col_min) filt.push_back(e);
      }
    }
    s->nnz_filtered[m] = filt.size();
    // column-major copy of the rows accumulate_rows visits
    std::vector<unsigned> cptr(s->num_cols + 1, 0);
    for (const Entry& e : all)
      if (e.major < nr_used) cptr[e.minor + 1]++;
    for (size_t i = 0; i < s->num_cols; ++i) cptr[i + 1] += cptr[i];
    bycol.resize(cptr[s->num_cols]);
    {
      std::vector<unsigned> cur(cptr.begin(), cptr.end() - 1);
      for (const Entry& e : all)
        if (e.major < nr_used) {
          Entry t = e;
          t.major = e.minor;
          t.minor = e.major;
          bycol[cur[e.minor]++] = t;
        }
    }
    for (size_t i = 0; i < s->num_cols; ++i) col_count[i] += cptr[i + 1] - cptr[i];
    int rc;
    col_host[m] = build_split(s->num_cols, bycol);
    if ((rc = upload_split(build_split(nrows, all), &s->row[m])) || (rc = upload_split(build_split(nrows, filt), &s->filtered[m]))) {
      delete s;
      return rc;
    }
  }
  std::vector<unsigned> long_cols;
  for (size_t i = 0; i < s->num_cols; ++i)
    if (col_count[i] >= spk::LONG_COLUMN) long_cols.push_back((unsigned)i);
  s->n_long_cols = long_cols.size();
  int rc = upload(&s->d_long_cols, long_cols);
  if (rc) {
    sp_shape_free(s);
    return rc;
  }
  {
    std::vector<unsigned> order;
    order.reserve(s->num_cols);
    for (size_t i = 0; i < s->num_cols; ++i)
      if (col_count[i] < spk::LONG_COLUMN) order.push_back((unsigned)i);
    // Sorted by decreasing entry count; within one total the columns are grouped by their (A, B, C) entry counts, so the lanes of a wave run the same
    // trip counts in each of the three matrices. (Sorting inside windows of neighbouring columns instead — for locality of the pointer loads and of the
    // gathers from evals_rx — measured the same 115-120 us: locality is not what bounds the kernel.)
    auto cnt6 = [&](unsigned col, unsigned out6[6]) {  // small / general entry counts of A, B, C
      for (int m = 0; m < 3; ++m) {
        out6[2 * m] = col_host[m].sptr[col + 1] - col_host[m].sptr[col];
        out6[2 * m + 1] = col_host[m].gptr[col + 1] - col_host[m].gptr[col];
      }
    };
    auto by_len = [&](unsigned x, unsigned y) {
      if (col_count[x] != col_count[y]) return col_count[x] > col_count[y];
      unsigned a[6], b[6];
      cnt6(x, a);
      cnt6(y, b);
      for (int k = 0; k < 5; ++k)
        if (a[k] != b[k]) return a[k] > b[k];
      return false;
    };
    const int order_mode = polyabc_order_mode();
    if (order_mode == 0) std::stable_sort(order.begin(), order.end(), by_len);
    else if (order_mode == 2)
    {
      const size_t win = polyabc_window();
      for (size_t lo = 0; lo < order.size(); lo += win) std::stable_sort(order.begin() + lo, order.begin() + std::min(order.size(), lo + win), by_len);
    }
    s->n_short = order.size();
    if ((rc = upload(&s->d_short_order, order))) {
      sp_shape_free(s);
      return rc;
    }
    // The column-major structure is STORED in the order it is walked - the short columns in `order`, then the long ones (round 6): lane i of the walk reads
    // entry i of the pointer arrays and the index lists of neighbouring lanes are neighbours in memory, instead of a dozen scattered 4-byte loads per
    // column through the permutation. (Config 4's synthetic instance - 3.8 M columns of 1-3 entries - walked in natural order took 1.02 ms of inner
    // sum-check against 1.45 sorted, and the SHA-256 instances the other way round, 120 against 76 us: with the storage permuted the sorted walk has both.)
    // SPARTAN_POLYABC_LAYOUT=natural keeps the columns where their numbers put them (A/B runs).
    const bool permuted = polyabc_permuted();
    s->col_permuted = permuted;
    std::vector<unsigned> seq;
    if (permuted) {
      seq = order;
      seq.insert(seq.end(), long_cols.begin(), long_cols.end());
    }
    for (int m = 0; m < 3; ++m) {
      if (!permuted) {
        if ((rc = upload_split(col_host[m], &s->col[m]))) {
          sp_shape_free(s);
          return rc;
        }
        continue;
      }
      const SplitHost& h = col_host[m];
      SplitHost q;
      q.sptr.assign(seq.size() + 1, 0);
      q.gptr.assign(seq.size() + 1, 0);
      q.sidx.reserve(h.sidx.size());
      q.scode.reserve(h.scode.size());
      q.gidx.reserve(h.gidx.size());
      q.gval.reserve(h.gval.size());
      for (size_t pos = 0; pos < seq.size(); ++pos) {
        const unsigned col = seq[pos];
        q.sidx.insert(q.sidx.end(), h.sidx.begin() + h.sptr[col], h.sidx.begin() + h.sptr[col + 1]);
        q.scode.insert(q.scode.end(), h.scode.begin() + h.sptr[col], h.scode.begin() + h.sptr[col + 1]);
        q.gidx.insert(q.gidx.end(), h.gidx.begin() + h.gptr[col], h.gidx.begin() + h.gptr[col + 1]);
        q.gval.insert(q.gval.end(), h.gval.begin() + h.gptr[col], h.gval.begin() + h.gptr[col + 1]);
        q.sptr[pos + 1] = (unsigned)q.sidx.size();
        q.gptr[pos + 1] = (unsigned)q.gidx.size();
      }
      if ((rc = upload_split(q, &s->col[m]))) {
        sp_shape_free(s);
        return rc;
      }
    }
  }
  SP_HIP(hipDeviceSynchronize());
  *out = s;
  return SP_OK;
}
void sp_shape_free(sp_shape* s) {
  if (!s) return;
  for (int m = 0; m < 3; ++m) {
    s->row[m].release();
    s->filtered[m].release();
    s->col[m].release();
  }
  hipFree(s->d_long_cols);
  hipFree(s->d_short_order);
  delete s;
}

int sp_shape_info(const sp_shape* s, uint64_t out[8]) {
  if (!s || !out) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_info: null argument");
  for (int m = 0; m < 3; ++m) {
    out[m] = s->nnz[m];
    out[3 + m] = s->nnz_filtered[m];
  }
  out[6] = s->n_long_cols;
  out[7] = s->n_short;
  return SP_OK;
}

}  // extern "C"

// ---- sp_shape_from_wire: a shape from the bincode bytes of SplitR1CSShape (src/r1cs/mod.rs:742-773) ----------------------------------------------------
// The stream is what sp_wire_shape(.., digest_form = 0) writes: the ten dimensions, then per matrix data (u64 length, 32 bytes an element), indices and
// indptr (u64 length, 8 bytes an element) and cols. wire_parse_shape takes the arrays as slices of the input and checks everything a later stage
// dereferences through - that is O(rows) host work and ends a refused call before the first launch. The row-major structure is then built either on the
// device from the raw bytes (wire_decode_device, kernels_wire_decode.hpp: the host touches no per-entry array) or on the host with the code behind
// sp_shape_from_csr (wire_decode_host: sp_unwire_scalars, index narrowing, Classifier, build_split), which is also a way to a full shape (SP_SHAPE_WIRE_FULL). The other
// way (SP_SHAPE_WIRE_FULL_DEVICE) continues the device decode: wire_full_device builds filtered[], col[] and the walk order from what the row decode left on the device
// (kernels_wire_full.hpp); the host reads six counters a column back and orders the columns, and touches no per-entry array.
namespace {

struct WireSlices {  // one matrix of the stream
  const uint8_t *data = nullptr, *idx = nullptr, *indptr = nullptr;
  uint64_t nnz = 0;
};
inline uint64_t le64(const uint8_t* p) {  // (little-endian host; the input need not be aligned)
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
}
struct DevOwner {  // the device allocations of one call: freed when the call ends unless the shape took them
  std::vector<void*> held;
  ~DevOwner() {
    for (void* q : held) hipFree(q);
  }
  template <class T>
  int alloc(T** out, size_t n) {
    hipError_t e = hipMalloc((void**)out, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess) return fail(SP_ERR_NO_DEVICE, std::string("sp_shape_from_wire: hipMalloc: ") + hipGetErrorString(e));
    held.push_back(*out);
    return SP_OK;
  }
  void release(void* q) { held.erase(std::remove(held.begin(), held.end(), q), held.end()); }
};
// what the last sp_shape_from_wire on this thread spent where (ms): upload, entry kernel, counts + scan, scatter (device events, SP_SHAPE_WIRE_TIMED),
// parse + checks, the decode as a whole, the whole call (host clock), and 1 / 0 for the device / host decode
thread_local double g_wire_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
constexpr bool WIRE_DEVICE_DEFAULT = true;  // which decode a call without a forcing flag takes: measured, profiles/verifier_key.md

double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int wire_parse_shape(sp_unwire* r, sp_dims* d, uint64_t* cols_out, WireSlices W[3]) {
  static const char* const names[3] = {"A", "B", "C"};
  const uint8_t* base = r->p;
  uint64_t w[10];
  int rc = sp_unwire_u64s(r, 10, w);
  if (rc) return rc;
  for (int i = 0; i < 10; ++i)
    if (w[i] >> 32) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: a dimension is 2^32 or more");
  d->num_cons = w[0], d->num_cons_unpadded = w[1];
  d->num_shared_unpadded = w[2], d->num_precommitted_unpadded = w[3], d->num_rest_unpadded = w[4];
  d->num_shared = w[5], d->num_precommitted = w[6], d->num_rest = w[7];
  d->num_public = w[8], d->num_challenges = w[9];
  if (d->num_cons == 0) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: num_cons must be at least 1");
  if (d->num_cons_unpadded > d->num_cons) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: num_cons_unpadded exceeds num_cons");
  if (d->num_shared_unpadded > d->num_shared || d->num_precommitted_unpadded > d->num_precommitted || d->num_rest_unpadded > d->num_rest)
    return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: an unpadded variable count exceeds its padded one");
  const uint64_t cols = d->num_shared + d->num_precommitted + d->num_rest + 1 + d->num_public + d->num_challenges, rows = d->num_cons;
  if (cols >> 32) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: 2^32 columns or more");
  *cols_out = cols;
  for (int m = 0; m < 3; ++m) {
    const std::string at = std::string(" (matrix ") + names[m] + ")";
    size_t nd, ni, np;
    if ((rc = sp_unwire_len(r, 32, &nd))) return rc;
    W[m].data = r->p;
    r->p += 32 * nd;
    if ((rc = sp_unwire_len(r, 8, &ni))) return rc;
    W[m].idx = r->p;
    r->p += 8 * ni;
    if ((rc = sp_unwire_len(r, 8, &np))) return rc;
    W[m].indptr = r->p;
    r->p += 8 * np;
    uint64_t cols_m;
    if ((rc = sp_unwire_u64s(r, 1, &cols_m))) return rc;
    W[m].nnz = nd;
    if (nd != ni) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: data and indices differ in length" + at);
    if ((uint64_t)nd >> 32) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: 2^32 entries or more" + at);
    if (np != rows + 1) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: indptr must hold num_cons + 1 offsets" + at);
    if (cols_m != cols) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: cols is not num_vars + 1 + num_public + num_challenges" + at);
    // u64 prefixes, 32- and 8-byte elements: every array starts at a multiple of 8 from the start of the shape (the device loads rely on it)
    if (((W[m].data - base) | (W[m].idx - base) | (W[m].indptr - base)) & 7) return fail(SP_ERR_INTERNAL, "sp_shape_from_wire: an array is not 8-byte aligned in the stream");
    uint64_t prev = le64(W[m].indptr);
    if (prev != 0) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: indptr does not start at 0" + at);
    for (uint64_t i = 1; i <= rows; ++i) {
      const uint64_t v = le64(W[m].indptr + 8 * i);
      if (v < prev) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: indptr decreases at row " + std::to_string(i - 1) + at);
      prev = v;
    }
    if (prev != nd) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: indptr does not end at the entry count" + at);
  }
  return SP_OK;
}

// what the full part of the last SP_SHAPE_WIRE_FULL_DEVICE call on this thread spent where (ms): filtered[] (counts, scan, scatter), the column counters and
// their read-back, the walk order on the host, the sort, the column structure (pointer scan and scatter) - device events, zero without SP_SHAPE_WIRE_TIMED -,
// the whole full part (host clock), the digit passes of the sort, one spare slot
thread_local double g_wire_full_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// `cols` short columns by decreasing packed key, ties in the order they stand in (ascending column number): what std::stable_sort with sp_shape_from_csr's
// six-count comparator gives, as a stable least-significant-digit radix sort of the 54-bit keys (a pass whose digit is the same for all is skipped)
void sort_columns_by_key(unsigned* first, size_t n, const std::vector<uint64_t>& key) {
  if (n < 2) return;
  if (n < 2048) {
    std::stable_sort(first, first + n, [&](unsigned x, unsigned y) { return key[x] > key[y]; });
    return;
  }
  constexpr unsigned BITS = 11, BINS = 1u << BITS;
  std::vector<unsigned> other(n), count(BINS);
  unsigned *src = first, *dst = other.data();
  for (unsigned shift = 0; shift < 54; shift += BITS) {
    std::fill(count.begin(), count.end(), 0u);
    for (size_t i = 0; i < n; ++i) count[(~key[src[i]] >> shift) & (BINS - 1)]++;
    if (count[(~key[src[0]] >> shift) & (BINS - 1)] == n) continue;
    unsigned at = 0;
    for (unsigned b = 0; b < BINS; ++b) {
      const unsigned t = count[b];
      count[b] = at;
      at += t;
    }
    for (size_t i = 0; i < n; ++i) dst[count[(~key[src[i]] >> shift) & (BINS - 1)]++] = src[i];
    std::swap(src, dst);
  }
  if (src != first) memcpy(first, src, n * sizeof(unsigned));
}

// The full part of the device decode: filtered[], col[], the walk order. `a` holds what the row decode left on the device (codes, narrowed columns, raw
// coefficients, row pointers; row[m]'s own arrays are not read). Every allocation goes through `own`: a refused call frees them all.
int wire_full_device(sp_ctx* c, const sp_dims& d, uint64_t cols, const WireSlices W[3], const spk::WireArgs& a, DevOwner& own, bool timed, sp_shape* s) {
  const double t_begin = wall_ms();
  const size_t rows = d.num_cons, nblk_rows = a.nblk, nblk_cols = (cols + spk::WIRE_SCAN_TILE - 1) / spk::WIRE_SCAN_TILE;
  const size_t nr_used = d.num_cons_unpadded, col_min = d.num_shared + d.num_precommitted;
  int rc;
  spk::FullArgs x;
  spk::WireArgs f = a, cp = a;  // the scan kernels' view of the filtered row pointers and of the column pointers
  uint64_t max_used = 0, all_used = 0, all_nnz = 0;
  for (int m = 0; m < 3; ++m) {
    x.n_used[m] = (unsigned)le64(W[m].indptr + 8 * nr_used);  // (row-major stream: the entries of the rows below nr_used are its first indptr[nr_used])
    max_used = std::max<uint64_t>(max_used, x.n_used[m]);
    all_used += x.n_used[m];
    all_nnz += W[m].nnz;
    if ((rc = own.alloc(&x.row32[m], W[m].nnz)) || (rc = own.alloc(&f.m[m].sptr, rows + 1)) || (rc = own.alloc(&f.m[m].gptr, rows + 1)) ||
        (rc = own.alloc(&cp.m[m].sptr, cols + 1)) || (rc = own.alloc(&cp.m[m].gptr, cols + 1)))
      return rc;
  }
  unsigned *d_fwords, *d_cwords, *d_pos;  // totals [6] | max_len [3] | block_sums [6 nblk]
  if ((rc = own.alloc(&x.col_cnt, 6 * cols)) || (rc = own.alloc(&d_fwords, 9 + 6 * nblk_rows)) || (rc = own.alloc(&d_cwords, 9 + 6 * nblk_cols)) || (rc = own.alloc(&d_pos, cols)))
    return rc;
  x.pos = d_pos;
  x.row_limit = nr_used, x.col_min = col_min, x.cols = cols;
  f.totals = d_fwords, f.max_len = d_fwords + 6, f.block_sums = d_fwords + 9, f.nblk = (unsigned)nblk_rows;
  cp.totals = d_cwords, cp.max_len = d_cwords + 6, cp.block_sums = d_cwords + 9, cp.nblk = (unsigned)nblk_cols;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() {
      for (int i = 0; i < 6; ++i)
        if (e[i]) hipEventDestroy(e[i]);
    }
  } ev_guard{ev};
  auto mark = [&](int i) -> hipError_t { return timed ? hipEventRecord(ev[i], c->stream) : hipSuccess; };
  if (timed)
    for (int i = 0; i < 6; ++i) SP_HIP(hipEventCreate(&ev[i]));
  const dim3 block(spk::WIRE_BLOCK);
  auto capped = [](uint64_t n) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((n + spk::WIRE_BLOCK - 1) / spk::WIRE_BLOCK, 1), 4096); };
  const unsigned row_blocks = capped(rows), col_blocks = capped(cols), used_blocks = capped(max_used);
  auto scan = [&](const spk::WireArgs& w, size_t n) {  // exclusive scan of w.m[].sptr / gptr over n elements, in place (kernels_wire_decode.hpp)
    c->timed_kernel("wire_scan", 3 * 8ull * n, spk::k_wire_scan_reduce, dim3(w.nblk, 3), block, w, n);
    c->timed_kernel("wire_scan", 3 * 16ull * w.nblk, spk::k_wire_scan_blocks, dim3(1, 3), block, w);
    c->timed_kernel("wire_scan", 3 * 16ull * n, spk::k_wire_scan_add, dim3(w.nblk, 3), block, w, n);
  };
  // ---- filtered[]: count, scan, scatter with the predicate
  SP_HIP(mark(0));
  SP_HIP(hipMemsetAsync(d_fwords, 0, 9 * sizeof(unsigned), c->stream));
  SP_HIP(hipMemsetAsync(x.col_cnt, 0, 6 * cols * sizeof(unsigned), c->stream));
  c->timed_kernel("wire_full_filtered", 9ull * all_nnz + 3 * 24ull * rows, spk::k_full_filt_counts, dim3(row_blocks, 3), block, a, f, x, rows);
  scan(f, rows);
  unsigned fwords[9];
  SP_HIP(hipMemcpyAsync(fwords, d_fwords, sizeof fwords, hipMemcpyDeviceToHost, c->stream));
  SP_HIP(sp::stream_sync(c->stream));
  SP_HIP(hipGetLastError());
  spk::WireOutArgs fo;
  for (int m = 0; m < 3; ++m) {
    if ((uint64_t)fwords[2 * m] + fwords[2 * m + 1] > x.n_used[m]) return fail(SP_ERR_INTERNAL, "sp_shape_from_wire: more filtered entries than entries");
    if ((rc = own.alloc(&fo.o[m].sidx, fwords[2 * m])) || (rc = own.alloc(&fo.o[m].scode, fwords[2 * m])) || (rc = own.alloc(&fo.o[m].gidx, fwords[2 * m + 1])) ||
        (rc = own.alloc(&fo.o[m].gval, fwords[2 * m + 1])))
      return rc;
  }
  c->timed_kernel("wire_full_filtered", 46ull * all_used + 3 * 24ull * rows, spk::k_full_filt_scatter, dim3(row_blocks, 3), block, a, f, fo, x, rows);
  SP_HIP(mark(1));
  // ---- the six counters of every column, back to the host
  if (max_used) c->timed_kernel("wire_full_col_counts", 9ull * all_used, spk::k_full_col_counts, dim3(used_blocks, 3), block, a, x);
  std::vector<unsigned> cnt(6 * cols);
  SP_HIP(hipMemcpyAsync(cnt.data(), x.col_cnt, cnt.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  SP_HIP(mark(2));
  SP_HIP(sp::stream_sync(c->stream));
  SP_HIP(hipGetLastError());
  // ---- the walk order (O(columns) on the host): the rules of sp_shape_from_csr under the same three settings
  const double t_order = wall_ms();
  const int order_mode = polyabc_order_mode();
  const bool permuted = polyabc_permuted();
  std::vector<unsigned> order, long_cols, pos(cols);
  std::vector<uint64_t> key(cols);
  unsigned n_small[3] = {0, 0, 0}, col_max_len[3] = {0, 0, 0};
  uint64_t sums[6] = {0, 0, 0, 0, 0, 0};
  order.reserve(cols);
  for (size_t i = 0; i < cols; ++i) {
    uint64_t total = 0, k = 0;
    for (int j = 0; j < 6; ++j) {
      const unsigned v = cnt[(size_t)j * cols + i];
      total += v;
      sums[j] += v;
      if (j < 5) k = (k << 9) | (v & 511u);  // (a short column's counts are below LONG_COLUMN = 512 each: nine bits)
    }
    for (int m = 0; m < 3; ++m) col_max_len[m] = std::max(col_max_len[m], cnt[(size_t)(2 * m) * cols + i] + cnt[(size_t)(2 * m + 1) * cols + i]);
    if (total >= spk::LONG_COLUMN) long_cols.push_back((unsigned)i);
    else {
      key[i] = (total << 45) | k;
      order.push_back((unsigned)i);
    }
  }
  for (int m = 0; m < 3; ++m) {
    if (sums[2 * m] + sums[2 * m + 1] != x.n_used[m]) return fail(SP_ERR_INTERNAL, "sp_shape_from_wire: the column counts do not add up to the entry count");
    n_small[m] = (unsigned)sums[2 * m];
  }
  if (order_mode == 0) sort_columns_by_key(order.data(), order.size(), key);
  else if (order_mode == 2) {
    const size_t win = polyabc_window();
    for (size_t lo = 0; lo < order.size(); lo += win) sort_columns_by_key(order.data() + lo, std::min(order.size(), lo + win) - lo, key);
  }
  if (permuted) {  // the column-major structure is stored in walk order: the short columns in `order`, then the long ones
    for (size_t i = 0; i < order.size(); ++i) pos[order[i]] = (unsigned)i;
    for (size_t i = 0; i < long_cols.size(); ++i) pos[long_cols[i]] = (unsigned)(order.size() + i);
  } else {
    for (size_t i = 0; i < cols; ++i) pos[i] = (unsigned)i;
  }
  const double order_ms = wall_ms() - t_order;
  unsigned *d_order, *d_long;
  if ((rc = own.alloc(&d_order, order.size())) || (rc = own.alloc(&d_long, long_cols.size()))) return rc;
  SP_HIP(mark(3));
  if (!order.empty()) SP_HIP(hipMemcpyAsync(d_order, order.data(), order.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  if (!long_cols.empty()) SP_HIP(hipMemcpyAsync(d_long, long_cols.data(), long_cols.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  SP_HIP(hipMemcpyAsync(d_pos, pos.data(), cols * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  // ---- the stable sort of the entry numbers by walk position, one digit a pass
  unsigned passes = 1;
  while (passes < 4 && ((cols - 1) >> (spk::FULL_SORT_BITS * passes)) != 0) ++passes;
  spk::SortArgs sa;
  sa.ntiles = (unsigned)std::max<uint64_t>((max_used + spk::FULL_SORT_TILE - 1) / spk::FULL_SORT_TILE, 1);
  const size_t hist_n = (size_t)spk::FULL_SORT_BINS * sa.ntiles, nblk_hist = (hist_n + spk::WIRE_SCAN_TILE - 1) / spk::WIRE_SCAN_TILE;
  spk::WireArgs hs = a;  // the scan kernels' view of the histograms
  unsigned *d_hwords, *buf_k[3][2], *buf_v[3][2];
  if ((rc = own.alloc(&d_hwords, 9 + 6 * nblk_hist))) return rc;
  hs.totals = d_hwords, hs.max_len = d_hwords + 6, hs.block_sums = d_hwords + 9, hs.nblk = (unsigned)nblk_hist;
  for (int m = 0; m < 3; ++m) {
    spk::SortMat& sm = sa.m[m];
    if ((rc = own.alloc(&sm.hist_s, hist_n + 1)) || (rc = own.alloc(&sm.hist_g, hist_n + 1))) return rc;
    for (int b = 0; b < 2; ++b)
      if ((rc = own.alloc(&buf_k[m][b], x.n_used[m])) || (rc = own.alloc(&buf_v[m][b], x.n_used[m]))) return rc;
    hs.m[m].sptr = sm.hist_s, hs.m[m].gptr = sm.hist_g;
    sm.n = x.n_used[m], sm.n_small = n_small[m];
  }
  for (unsigned p = 0; p < passes; ++p) {
    for (int m = 0; m < 3; ++m) {
      sa.m[m].keys_in = buf_k[m][(p + 1) & 1], sa.m[m].vals_in = buf_v[m][(p + 1) & 1];  // (not read by the first pass: it takes the stream itself)
      sa.m[m].keys_out = buf_k[m][p & 1], sa.m[m].vals_out = buf_v[m][p & 1];
    }
    const unsigned shift = spk::FULL_SORT_BITS * p;
    const dim3 grid(sa.ntiles, 3);
    if (p == 0) c->timed_kernel("wire_full_sort", 9ull * all_used, spk::k_full_sort_hist<true>, grid, block, a, x, sa, shift);
    else c->timed_kernel("wire_full_sort", 8ull * all_used, spk::k_full_sort_hist<false>, grid, block, a, x, sa, shift);
    scan(hs, hist_n);
    if (p == 0) c->timed_kernel("wire_full_sort", 17ull * all_used, spk::k_full_sort_scatter<true>, grid, block, a, x, sa, shift);
    else c->timed_kernel("wire_full_sort", 16ull * all_used, spk::k_full_sort_scatter<false>, grid, block, a, x, sa, shift);
  }
  SP_HIP(mark(4));
  // ---- col[]: the column pointers from the counts at their walk positions, then one lane a sorted entry
  c->timed_kernel("wire_full_columns", 3 * 20ull * cols, spk::k_full_col_place, dim3(col_blocks, 3), block, x, cp);
  scan(cp, cols);
  spk::ColOutArgs co;
  for (int m = 0; m < 3; ++m) {
    const unsigned ng = x.n_used[m] - n_small[m];
    if ((rc = own.alloc(&co.o[m].sidx, n_small[m])) || (rc = own.alloc(&co.o[m].scode, n_small[m])) || (rc = own.alloc(&co.o[m].gidx, ng)) || (rc = own.alloc(&co.o[m].gval, ng)))
      return rc;
    co.sorted[m] = buf_v[m][(passes - 1) & 1];
    co.n_small[m] = n_small[m];
  }
  if (max_used) c->timed_kernel("wire_full_columns", 45ull * all_used, spk::k_full_col_scatter, dim3(used_blocks, 3), block, a, x, co);
  SP_HIP(mark(5));
  unsigned cwords[6];
  SP_HIP(hipMemcpyAsync(cwords, d_cwords, sizeof cwords, hipMemcpyDeviceToHost, c->stream));
  SP_HIP(sp::stream_sync(c->stream));
  SP_HIP(hipGetLastError());
  for (int m = 0; m < 3; ++m)
    if (cwords[2 * m] != n_small[m] || cwords[2 * m] + cwords[2 * m + 1] != x.n_used[m]) return fail(SP_ERR_INTERNAL, "sp_shape_from_wire: the column pointers do not end at the entry count");
  if (timed) {
    float ms[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 5; ++i) SP_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    g_wire_full_ms[0] = ms[0], g_wire_full_ms[1] = ms[1], g_wire_full_ms[3] = ms[3], g_wire_full_ms[4] = ms[4];
  }
  g_wire_full_ms[2] = order_ms;
  g_wire_full_ms[6] = passes;
  // ---- everything succeeded: the shape takes its structures
  for (int m = 0; m < 3; ++m) {
    SplitOnDevice& fm = s->filtered[m];
    fm.sptr = f.m[m].sptr, fm.gptr = f.m[m].gptr;
    fm.sidx = fo.o[m].sidx, fm.scode = fo.o[m].scode, fm.gidx = fo.o[m].gidx, fm.gval = fo.o[m].gval;
    fm.max_len = fwords[6 + m];
    SplitOnDevice& cm = s->col[m];
    cm.sptr = cp.m[m].sptr, cm.gptr = cp.m[m].gptr;
    cm.sidx = co.o[m].sidx, cm.scode = co.o[m].scode, cm.gidx = co.o[m].gidx, cm.gval = co.o[m].gval;
    cm.max_len = col_max_len[m];
    for (void* q : {(void*)fm.sptr, (void*)fm.gptr, (void*)fm.sidx, (void*)fm.scode, (void*)fm.gidx, (void*)fm.gval, (void*)cm.sptr, (void*)cm.gptr, (void*)cm.sidx,
                    (void*)cm.scode, (void*)cm.gidx, (void*)cm.gval})
      own.release(q);
    s->nnz_filtered[m] = (uint64_t)fwords[2 * m] + fwords[2 * m + 1];
  }
  s->d_short_order = d_order, s->d_long_cols = d_long;
  own.release(d_order);
  own.release(d_long);
  s->n_short = order.size();
  s->n_long_cols = long_cols.size();
  s->col_permuted = permuted;
  g_wire_full_ms[5] = wall_ms() - t_begin;
  return SP_OK;
}

int wire_decode_device(sp_ctx* c, const sp_dims& d, uint64_t cols, const WireSlices W[3], bool timed, bool full, sp_shape* s) {
  static const char* const names[3] = {"A", "B", "C"};
  const size_t rows = d.num_cons, nblk = (rows + spk::WIRE_SCAN_TILE - 1) / spk::WIRE_SCAN_TILE;
  DevOwner own;
  spk::WireArgs a;
  uint4* d_data[3];
  unsigned long long *d_idx[3], *d_indptr[3];
  uint64_t max_nnz = 0, all_nnz = 0;
  int rc;
  for (int m = 0; m < 3; ++m) {
    const size_t nnz = W[m].nnz;
    max_nnz = std::max<uint64_t>(max_nnz, nnz);
    all_nnz += nnz;
    spk::WireMat& wm = a.m[m];
    if ((rc = own.alloc(&d_data[m], 2 * nnz)) || (rc = own.alloc(&d_idx[m], nnz)) || (rc = own.alloc(&d_indptr[m], rows + 1)) || (rc = own.alloc(&wm.code, nnz)) ||
        (rc = own.alloc(&wm.idx32, nnz)) || (rc = own.alloc(&wm.sptr, rows + 1)) || (rc = own.alloc(&wm.gptr, rows + 1)))
      return rc;
    wm.data = d_data[m];
    wm.idx = d_idx[m];
    wm.indptr = d_indptr[m];
    wm.nnz = nnz;
  }
  unsigned* d_words;  // totals [6] | max_len [3] | block_sums [6 nblk]
  if ((rc = own.alloc(&a.status, 6)) || (rc = own.alloc(&d_words, 9 + 6 * nblk))) return rc;
  a.cols = cols;
  a.totals = d_words;
  a.max_len = d_words + 6;
  a.block_sums = d_words + 9;
  a.nblk = (unsigned)nblk;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() {
      for (int i = 0; i < 5; ++i)
        if (e[i]) hipEventDestroy(e[i]);
    }
  } ev_guard{ev};
  auto mark = [&](int i) -> hipError_t { return timed ? hipEventRecord(ev[i], c->stream) : hipSuccess; };
  if (timed)
    for (int i = 0; i < 5; ++i) SP_HIP(hipEventCreate(&ev[i]));
  SP_HIP(mark(0));
  SP_HIP(hipMemsetAsync(a.status, 0xff, 6 * sizeof(unsigned long long), c->stream));
  SP_HIP(hipMemsetAsync(d_words, 0, 9 * sizeof(unsigned), c->stream));
  for (int m = 0; m < 3; ++m) {  // the raw bytes, once: no per-entry work on the host
    const size_t nnz = W[m].nnz;
    if (nnz) SP_HIP(hipMemcpyAsync(d_data[m], W[m].data, 32 * nnz, hipMemcpyHostToDevice, c->stream));
    if (nnz) SP_HIP(hipMemcpyAsync(d_idx[m], W[m].idx, 8 * nnz, hipMemcpyHostToDevice, c->stream));
    SP_HIP(hipMemcpyAsync(d_indptr[m], W[m].indptr, 8 * (rows + 1), hipMemcpyHostToDevice, c->stream));
  }
  SP_HIP(mark(1));
  const dim3 block(spk::WIRE_BLOCK);
  const unsigned row_blocks = (unsigned)std::min<size_t>((rows + spk::WIRE_BLOCK - 1) / spk::WIRE_BLOCK, 4096);
  if (max_nnz) {
    const unsigned eb = (unsigned)std::min<uint64_t>((max_nnz + spk::WIRE_BLOCK - 1) / spk::WIRE_BLOCK, 4096);
    c->timed_kernel("wire_entries", 45ull * all_nnz, spk::k_wire_entries, dim3(eb, 3), block, a);  // 32 + 8 in, 1 + 4 out an entry
  }
  SP_HIP(mark(2));
  c->timed_kernel("wire_row_counts", all_nnz + 3 * 24ull * rows, spk::k_wire_row_counts, dim3(row_blocks, 3), block, a, rows);
  c->timed_kernel("wire_scan", 3 * 8ull * rows, spk::k_wire_scan_reduce, dim3((unsigned)nblk, 3), block, a, rows);
  c->timed_kernel("wire_scan", 3 * 16ull * nblk, spk::k_wire_scan_blocks, dim3(1, 3), block, a);
  c->timed_kernel("wire_scan", 3 * 16ull * rows, spk::k_wire_scan_add, dim3((unsigned)nblk, 3), block, a, rows);
  SP_HIP(mark(3));
  unsigned long long status[6];
  unsigned words[9];
  SP_HIP(hipMemcpyAsync(status, a.status, sizeof status, hipMemcpyDeviceToHost, c->stream));
  SP_HIP(hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, c->stream));
  SP_HIP(sp::stream_sync(c->stream));
  SP_HIP(hipGetLastError());
  for (int m = 0; m < 3; ++m) {
    if (status[2 * m] != spk::WIRE_STATUS_OK)
      return fail(SP_ERR_INVALID_INPUT_LENGTH, std::string("sp_shape_from_wire: non-canonical field element at entry ") + std::to_string(status[2 * m]) + " of matrix " + names[m]);
    if (status[2 * m + 1] != spk::WIRE_STATUS_OK)
      return fail(SP_ERR_INVALID_INPUT_LENGTH, std::string("sp_shape_from_wire: column index out of range at entry ") + std::to_string(status[2 * m + 1]) + " of matrix " + names[m]);
    if ((uint64_t)words[2 * m] + words[2 * m + 1] != W[m].nnz) return fail(SP_ERR_INTERNAL, "sp_shape_from_wire: the class counts do not add up to the entry count");
  }
  spk::WireOutArgs o;
  for (int m = 0; m < 3; ++m)
    if ((rc = own.alloc(&o.o[m].sidx, words[2 * m])) || (rc = own.alloc(&o.o[m].scode, words[2 * m])) || (rc = own.alloc(&o.o[m].gidx, words[2 * m + 1])) ||
        (rc = own.alloc(&o.o[m].gval, words[2 * m + 1])))
      return rc;
  c->timed_kernel("wire_scatter", 46ull * all_nnz + 3 * 24ull * rows, spk::k_wire_scatter, dim3(row_blocks, 3), block, a, o, rows);
  SP_HIP(mark(4));
  SP_HIP(sp::stream_sync(c->stream));
  SP_HIP(hipGetLastError());
  if (timed)
    for (int i = 0; i < 4; ++i) {
      float ms = 0;
      SP_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
      g_wire_ms[i] = ms;
    }
  if (full && (rc = wire_full_device(c, d, cols, W, a, own, timed, s))) return rc;  // (it hands its structures over last: a refusal leaves `s` owning nothing)
  for (int m = 0; m < 3; ++m) {
    SplitOnDevice& r = s->row[m];
    r.sptr = a.m[m].sptr, r.gptr = a.m[m].gptr;
    r.sidx = o.o[m].sidx, r.scode = o.o[m].scode, r.gidx = o.o[m].gidx, r.gval = o.o[m].gval;
    r.max_len = words[6 + m];
    for (void* q : {(void*)r.sptr, (void*)r.gptr, (void*)r.sidx, (void*)r.scode, (void*)r.gidx, (void*)r.gval}) own.release(q);
    s->nnz[m] = W[m].nnz;
  }
  return SP_OK;  // (the raw bytes, the codes and the narrowed indices go with `own`)
}

int wire_decode_host(sp_ctx* c, const sp_dims& d, uint64_t cols, const WireSlices W[3], bool full, sp_shape** out) {
  const size_t rows = d.num_cons;
  std::vector<fe_t> data[3];
  std::vector<uint32_t> idx[3];
  std::vector<uint64_t> ptr[3];
  for (int m = 0; m < 3; ++m) {
    const size_t nnz = W[m].nnz;
    data[m].resize(nnz);
    idx[m].resize(nnz);
    ptr[m].resize(rows + 1);
    sp_unwire src{W[m].data, W[m].data + 32 * nnz};
    int rc = sp_unwire_scalars(&src, nnz, reinterpret_cast<uint64_t*>(data[m].data()));
    if (rc) return rc;
    for (size_t k = 0; k < nnz; ++k) {
      const uint64_t v = le64(W[m].idx + 8 * k);
      if (v >= cols) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: column index out of range at entry " + std::to_string(k));
      idx[m][k] = (uint32_t)v;
    }
    memcpy(ptr[m].data(), W[m].indptr, 8 * (rows + 1));
  }
  if (full) {
    sp_csr cs[3];
    for (int m = 0; m < 3; ++m) cs[m] = sp_csr{reinterpret_cast<const uint64_t*>(data[m].data()), idx[m].data(), ptr[m].data()};
    return sp_shape_from_csr(c, &cs[0], &cs[1], &cs[2], &d, out);
  }
  sp_shape* s = new sp_shape();
  s->dims = d;
  s->num_vars = d.num_shared + d.num_precommitted + d.num_rest;
  s->num_cols = cols;
  s->row_only = true;
  Classifier cls;
  for (int m = 0; m < 3; ++m) {
    std::vector<Entry> all(W[m].nnz);
    for (size_t r = 0; r < rows; ++r)
      for (uint64_t k = ptr[m][r]; k < ptr[m][r + 1]; ++k) {
        Entry& e = all[k];
        e.major = (unsigned)r;
        e.minor = idx[m][k];
        e.val = data[m][k];
        e.code = cls.code(e.val);
      }
    s->nnz[m] = W[m].nnz;
    int rc = upload_split(build_split(rows, all), &s->row[m]);
    if (rc) {
      sp_shape_free(s);
      return rc;
    }
  }
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    sp_shape_free(s);
    return fail(SP_ERR_NO_DEVICE, std::string("sp_shape_from_wire: ") + hipGetErrorString(e));
  }
  *out = s;
  return SP_OK;
}

}  // namespace

extern "C" {

size_t sp_shape_wire_block(void) { return (size_t)spk::WIRE_BLOCK; }
size_t sp_shape_wire_scan_tile(void) { return (size_t)spk::WIRE_SCAN_TILE; }
int sp_shape_wire_device_default(void) { return WIRE_DEVICE_DEFAULT ? 1 : 0; }
void sp_shape_from_wire_stages(double out[8]) {
  if (out) memcpy(out, g_wire_ms, sizeof g_wire_ms);
}
size_t sp_shape_wire_sort_tile(void) { return (size_t)spk::FULL_SORT_TILE; }
size_t sp_shape_wire_sort_digit_bits(void) { return (size_t)spk::FULL_SORT_BITS; }
void sp_shape_from_wire_full_stages(double out[8]) {
  if (out) memcpy(out, g_wire_full_ms, sizeof g_wire_full_ms);
}

// A checking tool: every device array of both shapes copied back and compared on the host. `where` names the first difference by structure, matrix, array
// and index ("col[1].sidx[37]: 5 != 6"); it is empty when there is none.
int sp_shape_compare(sp_ctx* c, const sp_shape* a, const sp_shape* b, char* where, size_t cap) {
  if (!c || !a || !b || !where || !cap) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_compare: null argument");
  where[0] = 0;
  std::string diff;
  auto differ = [&](const std::string& what) {
    diff = what;
    snprintf(where, cap, "%s", diff.c_str());
    return SP_OK;
  };
  auto scalar = [&](const char* name, uint64_t x, uint64_t y) {
    if (diff.empty() && x != y) diff = std::string(name) + ": " + std::to_string(x) + " != " + std::to_string(y);
  };
  SP_HIP(sp::stream_sync(c->stream));
  static const char* const dim_names[10] = {"num_cons", "num_cons_unpadded", "num_shared", "num_precommitted", "num_rest", "num_shared_unpadded", "num_precommitted_unpadded",
                                            "num_rest_unpadded", "num_public", "num_challenges"};
  const uint64_t *da = reinterpret_cast<const uint64_t*>(&a->dims), *db = reinterpret_cast<const uint64_t*>(&b->dims);
  static_assert(sizeof(sp_dims) == 10 * sizeof(uint64_t), "sp_dims is ten words");
  for (int i = 0; i < 10; ++i) scalar((std::string("dims.") + dim_names[i]).c_str(), da[i], db[i]);
  scalar("num_cols", a->num_cols, b->num_cols);
  scalar("row_only", a->row_only, b->row_only);
  if (!diff.empty()) return differ(diff);
  int rc = SP_OK;
  auto arrays = [&](const std::string& name, const void* x, const void* y, size_t n, size_t elem) {  // elem: bytes an element
    if (!diff.empty() || rc || !n) return;
    std::vector<uint8_t> hx(n * elem), hy(n * elem);
    if (hipMemcpy(hx.data(), x, n * elem, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hy.data(), y, n * elem, hipMemcpyDeviceToHost) != hipSuccess) {
      rc = fail(SP_ERR_NO_DEVICE, "sp_shape_compare: hipMemcpy of " + name);
      return;
    }
    if (!memcmp(hx.data(), hy.data(), n * elem)) return;
    size_t i = 0;
    while (!memcmp(hx.data() + i * elem, hy.data() + i * elem, elem)) ++i;
    diff = name + "[" + std::to_string(i) + "]";
    if (elem <= 4) {
      uint32_t vx = 0, vy = 0;
      memcpy(&vx, hx.data() + i * elem, elem);
      memcpy(&vy, hy.data() + i * elem, elem);
      diff += ": " + std::to_string(vx) + " != " + std::to_string(vy);
    }
  };
  auto split = [&](const char* structure, int m, const SplitOnDevice& x, const SplitOnDevice& y, size_t n_major) {
    const std::string at = std::string(structure) + "[" + std::to_string(m) + "].";
    scalar((at + "max_len").c_str(), x.max_len, y.max_len);
    arrays(at + "sptr", x.sptr, y.sptr, n_major + 1, 4);
    arrays(at + "gptr", x.gptr, y.gptr, n_major + 1, 4);
    if (!diff.empty() || rc) return;
    unsigned ns = 0, ng = 0;  // (equal in both by now)
    if (hipMemcpy(&ns, x.sptr + n_major, 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&ng, x.gptr + n_major, 4, hipMemcpyDeviceToHost) != hipSuccess) {
      rc = fail(SP_ERR_NO_DEVICE, "sp_shape_compare: hipMemcpy of " + at + "sptr");
      return;
    }
    arrays(at + "sidx", x.sidx, y.sidx, ns, 4);
    arrays(at + "scode", x.scode, y.scode, ns, 1);
    arrays(at + "gidx", x.gidx, y.gidx, ng, 4);
    arrays(at + "gval", x.gval, y.gval, ng, sizeof(fe_t));
  };
  for (int m = 0; m < 3; ++m) scalar(("nnz[" + std::to_string(m) + "]").c_str(), a->nnz[m], b->nnz[m]);
  for (int m = 0; m < 3; ++m) split("row", m, a->row[m], b->row[m], a->dims.num_cons);
  if (!a->row_only) {
    for (int m = 0; m < 3; ++m) scalar(("nnz_filtered[" + std::to_string(m) + "]").c_str(), a->nnz_filtered[m], b->nnz_filtered[m]);
    scalar("n_short", a->n_short, b->n_short);
    scalar("n_long_cols", a->n_long_cols, b->n_long_cols);
    scalar("col_permuted", a->col_permuted, b->col_permuted);
    for (int m = 0; m < 3; ++m) split("filtered", m, a->filtered[m], b->filtered[m], a->dims.num_cons);
    arrays("short_order", a->d_short_order, b->d_short_order, a->n_short, 4);
    arrays("long_cols", a->d_long_cols, b->d_long_cols, a->n_long_cols, 4);
    for (int m = 0; m < 3; ++m) split("col", m, a->col[m], b->col[m], a->num_cols);
  }
  if (rc) return rc;
  return diff.empty() ? SP_OK : differ(diff);
}

int sp_shape_from_wire(sp_ctx* c, sp_unwire* r, unsigned flags, sp_dims* dims_out, sp_shape** out) {
  if (!c || !r || !dims_out || !out) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: null argument");
  const bool want_dev = flags & SP_SHAPE_WIRE_DEVICE, want_host = flags & SP_SHAPE_WIRE_HOST, full = flags & SP_SHAPE_WIRE_FULL;
  const bool full_dev = flags & SP_SHAPE_WIRE_FULL_DEVICE;
  if ((flags & ~(unsigned)(SP_SHAPE_WIRE_DEVICE | SP_SHAPE_WIRE_HOST | SP_SHAPE_WIRE_FULL | SP_SHAPE_WIRE_TIMED | SP_SHAPE_WIRE_FULL_DEVICE)) || (want_dev && (want_host || full)))
    return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: flags that exclude each other (the device decode builds the row-only shape; the full shape takes the host decode)");
  if (full_dev && (want_dev || want_host || full))
    return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_shape_from_wire: flags that exclude each other (SP_SHAPE_WIRE_FULL_DEVICE builds the full shape on the device and takes no other form)");
  for (double& x : g_wire_ms) x = 0;
  for (double& x : g_wire_full_ms) x = 0;
  const double t0 = wall_ms();
  sp_dims d;
  uint64_t cols = 0;
  WireSlices W[3];
  int rc = wire_parse_shape(r, &d, &cols, W);
  if (rc) return rc;
  const double t1 = wall_ms();
  const bool device = full_dev || want_dev || (!want_host && !full && WIRE_DEVICE_DEFAULT);
  sp_shape* s = nullptr;
  if (device) {
    s = new sp_shape();
    s->dims = d;
    s->num_vars = d.num_shared + d.num_precommitted + d.num_rest;
    s->num_cols = cols;
    s->row_only = !full_dev;
    if ((rc = wire_decode_device(c, d, cols, W, (flags & SP_SHAPE_WIRE_TIMED) != 0, full_dev, s))) {
      delete s;  // (it owns nothing yet: the structures are handed over at the very end of a decode that succeeded)
      return rc;
    }
  } else if ((rc = wire_decode_host(c, d, cols, W, full, &s))) {
    return rc;
  }
  const double t2 = wall_ms();
  g_wire_ms[4] = t1 - t0;
  g_wire_ms[5] = t2 - t1;
  g_wire_ms[6] = t2 - t0;
  g_wire_ms[7] = device ? 1 : 0;
  *dims_out = d;
  *out = s;
  return SP_OK;
}

static int spmv3(sp_ctx* c, const sp_shape* s, const SplitOnDevice* mats, const uint64_t* nnz, const sp_table* z, const sp_table* const* base,
                 sp_table** outs, const char* what) {
  const size_t nrows = s->dims.num_cons;
  if (z->len != s->num_cols) return fail(SP_ERR_INVALID_WITNESS_LENGTH, "multiply_vec: z has the wrong length");
  spk::Spmv3Args a;
  for (int m = 0; m < 3; ++m) {
    if (outs[m]->cap < nrows) return fail(SP_ERR_INVALID_INPUT_LENGTH, "multiply_vec: output table too short");
    if (base && base[m]->cap < nrows) return fail(SP_ERR_INVALID_INPUT_LENGTH, "multiply_vec_incremental: cached table too short");
    a.m[m] = mats[m].view();
    a.base[m] = base ? base[m]->d : nullptr;
    a.out[m] = outs[m]->d;
    outs[m]->len = nrows;
    outs[m]->lo_eff = outs[m]->hi_eff = (size_t)-1;
  }
  size_t blocks = (nrows + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  // sum_nnz (4 + 32) [+32 per general coefficient, ignored] + 3*32*N outputs (+ cached reads when incremental)
  uint64_t bytes = 36ull * (nnz[0] + nnz[1] + nnz[2]) + 96ull * nrows * (base ? 2 : 1);
  const bool long_rows = mats[0].max_len > spk::SPMV_LONG_ROW || mats[1].max_len > spk::SPMV_LONG_ROW || mats[2].max_len > spk::SPMV_LONG_ROW;
  c->timed(what, bytes, [&] {
    if (long_rows) hipLaunchKernelGGL(spk::k_spmv3<true>, dim3((unsigned)blocks, 3), dim3(256), 0, c->stream, a, z->d, nrows);
    else hipLaunchKernelGGL(spk::k_spmv3<false>, dim3((unsigned)blocks, 3), dim3(256), 0, c->stream, a, z->d, nrows);
  });
  return SP_OK;
}

int sp_multiply_vec(sp_ctx* c, const sp_shape* s, const sp_table* z, sp_table* az, sp_table* bz, sp_table* cz) {
  sp_table* outs[3] = {az, bz, cz};
  return spmv3(c, s, s->row, s->nnz, z, nullptr, outs, "spmv");
}
int sp_multiply_vec_batched(sp_ctx* c, const sp_shape* s, const sp_table* const* zs, size_t count, sp_table* const* az, sp_table* const* bz, sp_table* const* cz) {
  if (count && (!zs || !az || !bz || !cz)) return fail(SP_ERR_INVALID_INPUT_LENGTH, "multiply_vec_batched: null argument");
  // one launch per vector: the matrices (a few MB of indices) stay in the L2s between launches, which is what the reference's single pass over the
  // matrix for all vectors buys on a CPU
  for (size_t k = 0; k < count; ++k) {
    sp_table* outs[3] = {az[k], bz[k], cz[k]};
    int rc = spmv3(c, s, s->row, s->nnz, zs[k], nullptr, outs, "spmv");
    if (rc) return rc;
  }
  return SP_OK;
}
// multiply_vec_batched (sparse.rs:237-302) with the reference's ONE pass over the matrices for several vectors: chunks of SPMV_KC vectors, one launch
// of k_spmv3_multi each. Every argument is checked before the first launch, so a refused call has written nothing.
size_t sp_multiply_vec_chunk(void) { return (size_t)spk::SPMV_KC; }
int sp_multiply_vec_chunked(sp_ctx* c, const sp_shape* s, const sp_table* const* zs, size_t count, sp_table* const* az, sp_table* const* bz, sp_table* const* cz) {
  if (!c || !s || (count && (!zs || !az || !bz || !cz))) return fail(SP_ERR_INVALID_INPUT_LENGTH, "multiply_vec_chunked: null argument");
  const size_t nrows = s->dims.num_cons;
  for (size_t k = 0; k < count; ++k) {
    const std::string at = ", vector " + std::to_string(k);
    if (!zs[k] || !az[k] || !bz[k] || !cz[k]) return fail(SP_ERR_INVALID_INPUT_LENGTH, "multiply_vec_chunked: null table" + at);
    if (zs[k]->len != s->num_cols) return fail(SP_ERR_INVALID_WITNESS_LENGTH, "multiply_vec_chunked: z has the wrong length" + at);
    if (az[k]->cap < nrows || bz[k]->cap < nrows || cz[k]->cap < nrows) return fail(SP_ERR_INVALID_INPUT_LENGTH, "multiply_vec_chunked: output table too short" + at);
  }
  size_t blocks = (nrows + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks == 0) blocks = 1;
  const uint64_t nnz = s->nnz[0] + s->nnz[1] + s->nnz[2];
  for (size_t k0 = 0; k0 < count; k0 += spk::SPMV_KC) {
    const size_t kc = std::min<size_t>(spk::SPMV_KC, count - k0);
    spk::SpmvMultiArgs a;
    for (int m = 0; m < 3; ++m) a.m[m] = s->row[m].view();
    for (size_t j = 0; j < (size_t)spk::SPMV_KC; ++j) {  // (the unused slots of a ragged chunk are never dereferenced)
      const size_t k = k0 + (j < kc ? j : 0);
      a.z[j] = zs[k]->d;
      sp_table* outs[3] = {az[k], bz[k], cz[k]};
      for (int m = 0; m < 3; ++m) {
        a.out[m][j] = outs[m]->d;
        outs[m]->len = nrows;
        outs[m]->lo_eff = outs[m]->hi_eff = (size_t)-1;
      }
    }
    a.kc = (int)kc;
    // structure once per chunk (4-byte index + code, row pointers of both classes) + one 32-byte gather per entry and vector + the 3 outputs per vector
    const uint64_t bytes = 5ull * nnz + 24ull * nrows + kc * (32ull * nnz + 96ull * nrows);
    c->timed_kernel("spmv_multi", bytes, spk::k_spmv3_multi, dim3((unsigned)blocks, 3), dim3(256), a, nrows);
  }
  return SP_OK;
}
int sp_multiply_vec_incremental(sp_ctx* c, const sp_shape* s, const sp_table* z, const sp_table* caz, const sp_table* cbz, const sp_table* ccz,
                                sp_table* az, sp_table* bz, sp_table* cz) {
  if (int rc = refuse_row_only(s, "multiply_vec_incremental")) return rc;
  sp_table* outs[3] = {az, bz, cz};
  const sp_table* base[3] = {caz, cbz, ccz};
  return spmv3(c, s, s->filtered, s->nnz_filtered, z, base, outs, "spmv_incremental");
}

int sp_multiply_vec_incremental_round0(sp_ctx* c, const sp_shape* s, const sp_table* z, const sp_table* caz, const sp_table* cbz, const sp_table* ccz, sp_table* az,
                                       sp_table* bz, sp_table* cz, sp_table* p0, sp_table* p1) {
  if (int rc = refuse_row_only(s, "multiply_vec_incremental_round0")) return rc;
  const size_t nrows = s->dims.num_cons, half = nrows / 2;
  if (nrows < 2) return fail(SP_ERR_INVALID_INPUT_LENGTH, "multiply_vec_incremental_round0: needs at least two rows");
  if (p0->cap < half || p1->cap < half) return fail(SP_ERR_INVALID_INPUT_LENGTH, "multiply_vec_incremental_round0: product tables too short");
  int rc = sp_multiply_vec_incremental(c, s, z, caz, cbz, ccz, az, bz, cz);
  if (rc) return rc;
  p0->len = p1->len = half;
  p0->lo_eff = p0->hi_eff = p1->lo_eff = p1->hi_eff = (size_t)-1;
  size_t blocks = (half + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  c->timed("round0_products", 224ull * half, [&] { hipLaunchKernelGGL(spk::k_round0_products, dim3((unsigned)blocks), dim3(256), 0, c->stream, az->d, bz->d, cz->d, half, p0->d, p1->d); });
  return SP_OK;
}

int sp_poly_abc(sp_ctx* c, const sp_shape* s, const sp_table* rx, const uint64_t r_[4], size_t out_len, sp_table* out) {
  if (int rc = refuse_row_only(s, "poly_ABC")) return rc;
  if (rx->len != s->dims.num_cons) return fail(SP_ERR_INVALID_INPUT_LENGTH, "poly_ABC: rx must have num_cons elements");
  if (out_len < s->num_cols || out->cap < out_len) return fail(SP_ERR_INVALID_INPUT_LENGTH, "poly_ABC: output too short");
  spk::PolyAbcArgs a;
  for (int m = 0; m < 3; ++m) a.m[m] = s->col[m].view();
  memcpy(&a.r, r_, 32);
  a.r2 = fe_mul<S>(a.r, a.r);
  // the long columns' partial triples and arrival counters belong to the CONTEXT (a shape is shared by every context that proves with its key): the
  // counters are zeroed when the buffer is (re)allocated and each column's last block leaves its counter at zero again
  const size_t ticket_bytes = (s->n_long_cols + 1) * sizeof(unsigned);
  const bool fresh = c->ws_bytes[sp_ctx::WS_POLYABC_TICKETS] < ticket_bytes;
  fe_t* partials = (fe_t*)c->workspace(sp_ctx::WS_POLYABC_PARTIALS, (s->n_long_cols + 1) * spk::LONG_NB_MAX * 3 * sizeof(fe_t));
  unsigned* tickets = (unsigned*)c->workspace(sp_ctx::WS_POLYABC_TICKETS, ticket_bytes);
  if (!partials || !tickets) return SP_ERR_NO_DEVICE;
  if (fresh) SP_HIP(hipMemsetAsync(tickets, 0, c->ws_bytes[sp_ctx::WS_POLYABC_TICKETS], c->stream));
  size_t blocks = (s->n_short + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks == 0) blocks = 1;
  const uint64_t bytes = 36ull * (s->nnz[0] + s->nnz[1] + s->nnz[2]) + 32ull * out_len;
  const size_t zero_n = out_len - s->num_cols;
  size_t zblocks = (2 * zero_n + 256 * 16 - 1) / (256 * 16);  // 16 stores of 16 bytes per thread
  if (zblocks > 2048) zblocks = 2048;
  c->timed("poly_abc", bytes, [&] {
    hipLaunchKernelGGL(spk::k_polyabc_short_and_long, dim3((unsigned)(blocks + spk::LONG_NB_MAX * s->n_long_cols + zblocks)), dim3(256), 0, c->stream, a, rx->d, s->d_short_order,
                       s->n_short, out->d, s->d_long_cols, (unsigned)s->n_long_cols, partials, tickets, (unsigned)blocks, (size_t)s->num_cols, zero_n, s->col_permuted ? 1 : 0);
  });
  return SP_OK;
}

// evals_rx + poly_ABC of `count` proofs of one shape: chunks of PAB_KC proofs, per chunk the pyramids of its points, the outer product that writes the
// chunk's eq tables interleaved (the context's workspace, reused by every chunk: the stream orders them) and one walk (kernels_polyabc_batch.hpp). Every
// argument is checked before the first launch, so a refused call has written nothing. The points and challenges travel by value: nothing of the
// caller's is read after the call returns. The arrival counters are this entry point's own (not sp_poly_abc's).
size_t sp_poly_abc_batch_chunk(void) { return (size_t)spk::PAB_KC; }
int sp_poly_abc_batch(sp_ctx* c, const sp_shape* s, size_t count, const uint64_t* r_x, size_t ell, const uint64_t* r_, size_t out_len, sp_table* const* out) {
  if (!c || !s || (count && ((ell && !r_x) || !r_ || !out))) return fail(SP_ERR_INVALID_INPUT_LENGTH, "poly_abc_batch: null argument");
  if (int rc = refuse_row_only(s, "poly_abc_batch")) return rc;
  if (count == 0) return SP_OK;
  const size_t nrows = s->dims.num_cons;
  if (ell > (size_t)spk::PAB_MAX_ELL || ((size_t)1 << ell) != nrows) return fail(SP_ERR_INVALID_INPUT_LENGTH, "poly_abc_batch: r_x must have log2(num_cons) coordinates");
  if (out_len < s->num_cols) return fail(SP_ERR_INVALID_INPUT_LENGTH, "poly_abc_batch: out_len is shorter than z");
  for (size_t k = 0; k < count; ++k) {
    const std::string at = ", proof " + std::to_string(k);
    if (!out[k]) return fail(SP_ERR_INVALID_INPUT_LENGTH, "poly_abc_batch: null table" + at);
    if (out[k]->cap < out_len) return fail(SP_ERR_INVALID_INPUT_LENGTH, "poly_abc_batch: output table too short" + at);
    for (size_t j = 0; j < k; ++j)
      if (out[j] == out[k] || out[j]->d == out[k]->d) return fail(SP_ERR_INVALID_INPUT_LENGTH, "poly_abc_batch: the same table as the output of proof " + std::to_string(j) + at);
  }
  constexpr size_t KC = (size_t)spk::PAB_KC;
  const int hi_bits = (int)(ell / 2), lo_bits = (int)ell - hi_bits;  // both <= 10 up to 2^20 rows: every level of both pyramids stays in LDS
  const size_t pyr_hi = (size_t)2 << hi_bits, pyr_stride = pyr_hi + ((size_t)2 << lo_bits);
  const size_t ticket_bytes = (s->n_long_cols + 1) * sizeof(unsigned);
  const bool fresh = c->ws_bytes[sp_ctx::WS_POLYABC_BATCH_TICKETS] < ticket_bytes;
  unsigned* tickets = (unsigned*)c->workspace(sp_ctx::WS_POLYABC_BATCH_TICKETS, ticket_bytes);
  if (!tickets) return SP_ERR_NO_DEVICE;
  if (fresh) SP_HIP(hipMemsetAsync(tickets, 0, c->ws_bytes[sp_ctx::WS_POLYABC_BATCH_TICKETS], c->stream));
  fe_t* partials = (fe_t*)c->workspace(sp_ctx::WS_POLYABC_BATCH_PARTIALS, (s->n_long_cols + 1) * spk::LONG_NB_MAX * 3 * KC * sizeof(fe_t));
  fe_t* pyr = (fe_t*)c->workspace(sp_ctx::WS_POLYABC_BATCH_PYRAMIDS, KC * pyr_stride * sizeof(fe_t));
  fe_t* E = (fe_t*)c->workspace(sp_ctx::WS_POLYABC_BATCH_EQ, KC * nrows * sizeof(fe_t));
  if (!partials || !pyr || !E) return SP_ERR_NO_DEVICE;
  size_t blocks = (s->n_short + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks == 0) blocks = 1;
  const size_t zero_n = out_len - s->num_cols;
  size_t zblocks = (2 * zero_n + 256 * 16 - 1) / (256 * 16);  // 16 stores of 16 bytes per thread and table
  if (zblocks > 2048) zblocks = 2048;
  size_t eblocks = (KC * nrows + 255) / 256;
  if (eblocks > 8192) eblocks = 8192;
  const uint64_t nnz = s->nnz[0] + s->nnz[1] + s->nnz[2];
  const dim3 grid((unsigned)(blocks + spk::LONG_NB_MAX * s->n_long_cols + zblocks));
  for (size_t k0 = 0; k0 < count; k0 += KC) {
    const size_t kc = std::min<size_t>(KC, count - k0);
    spk::PabPoints pts;
    spk::PabArgs a;
    for (int m = 0; m < 3; ++m) a.m[m] = s->col[m].view();
    for (size_t j = 0; j < KC; ++j) {  // (the unused slots of a ragged chunk are never dereferenced)
      const size_t k = k0 + (j < kc ? j : 0);
      if (ell) memcpy(pts.v[j], r_x + 4 * ell * k, ell * sizeof(fe_t));
      memcpy(&a.r[j], r_ + 4 * k, sizeof(fe_t));
      a.r2[j] = fe_mul<S>(a.r[j], a.r[j]);
      a.out[j] = out[k]->d;
    }
    a.kc = (int)kc;
    c->timed_kernel("eq_levels_batch", (uint64_t)kc * pyr_stride * sizeof(fe_t), spk::k_pab_eq_levels, dim3(2, (unsigned)kc), dim3(1024), pts, (int)ell, hi_bits, pyr,
                    (unsigned long long)pyr_stride, (unsigned long long)pyr_hi);
    c->timed_kernel("eq_table_batch", 32ull * nrows * kc, spk::k_pab_eq_outer, dim3((unsigned)eblocks), dim3(256), (const fe_t*)pyr, (unsigned long long)pyr_stride,
                    (unsigned long long)spk::eq_level_offset(hi_bits), (unsigned long long)(pyr_hi + spk::eq_level_offset(lo_bits)), lo_bits, nrows, (int)kc, E);
    // structure once per chunk (4-byte index + code, column pointers of both classes) + one 32-byte gather per entry and proof + the output per proof
    const uint64_t bytes = 5ull * nnz + 24ull * s->num_cols + kc * (32ull * nnz + 32ull * out_len);
    if (kc == KC)
      c->timed_kernel("poly_abc_batch", bytes, spk::k_pab_walk<true>, grid, dim3(256), a, (const fe_t*)E, (const unsigned*)s->d_short_order, s->n_short,
                      (const unsigned*)s->d_long_cols, (unsigned)s->n_long_cols, partials, tickets, (unsigned)blocks, (size_t)s->num_cols, zero_n, s->col_permuted ? 1 : 0);
    else
      c->timed_kernel("poly_abc_batch", bytes, spk::k_pab_walk<false>, grid, dim3(256), a, (const fe_t*)E, (const unsigned*)s->d_short_order, s->n_short,
                      (const unsigned*)s->d_long_cols, (unsigned)s->n_long_cols, partials, tickets, (unsigned)blocks, (size_t)s->num_cols, zero_n, s->col_permuted ? 1 : 0);
  }
  return SP_OK;
}

// evaluate_with_tables_fast (src/r1cs/mod.rs:1216-1226; call site src/spartan.rs:540-548) for `count` pairs of tables: chunks of MATEVAL_KC pairs, one
// launch each (the structure is read once per chunk), the 3 results of every pair collected on the device and copied out once at the end.
size_t sp_shape_matrix_evals_chunk(void) { return (size_t)spk::MATEVAL_KC; }
int sp_shape_matrix_evals_batched(sp_ctx* c, const sp_shape* s, const sp_table* const* tx, const sp_table* const* ty, size_t count, uint64_t* out) {
  if (!s || (count && (!tx || !ty || !out))) return fail(SP_ERR_INVALID_INPUT_LENGTH, "matrix_evals_batched: null argument");
  const size_t nrows = s->dims.num_cons;
  for (size_t k = 0; k < count; ++k) {
    if (!tx[k] || !ty[k]) return fail(SP_ERR_INVALID_INPUT_LENGTH, "matrix_evals_batched: null table");
    if (tx[k]->len < nrows) return fail(SP_ERR_INVALID_WITNESS_LENGTH, "matrix_evals_batched: a T_x table has fewer than num_cons elements");
    if (ty[k]->len < s->num_cols) return fail(SP_ERR_INVALID_WITNESS_LENGTH, "matrix_evals_batched: a T_y table is shorter than z");
  }
  if (count == 0) return SP_OK;
  size_t blocks = (nrows + 255) / 256;
  if (blocks > spk::MATEVAL_MAX_BLOCKS) blocks = spk::MATEVAL_MAX_BLOCKS;
  if (blocks == 0) blocks = 1;
  // the arrival counters first, zeroed in the same breath as they are allocated (every launch leaves them at zero again): a later allocation that fails
  // must not leave a ticket buffer behind that the next call takes for a used one
  const bool fresh = c->ws_bytes[sp_ctx::WS_MATEVAL_TICKETS] < 3 * sizeof(unsigned);
  unsigned* tickets = (unsigned*)c->workspace(sp_ctx::WS_MATEVAL_TICKETS, 3 * sizeof(unsigned));
  if (!tickets) return SP_ERR_NO_DEVICE;
  if (fresh) SP_HIP(hipMemsetAsync(tickets, 0, c->ws_bytes[sp_ctx::WS_MATEVAL_TICKETS], c->stream));
  fe_t* partials = (fe_t*)c->workspace(sp_ctx::WS_MATEVAL_PARTIALS, 3 * (size_t)spk::MATEVAL_MAX_BLOCKS * spk::MATEVAL_KC * sizeof(fe_t));
  fe_t* d_out = (fe_t*)c->workspace(sp_ctx::WS_MATEVAL_OUT, count * 3 * sizeof(fe_t));
  if (!partials || !d_out) return SP_ERR_NO_DEVICE;
  const uint64_t nnz = s->nnz[0] + s->nnz[1] + s->nnz[2];
  for (size_t k0 = 0; k0 < count; k0 += spk::MATEVAL_KC) {
    const size_t kc = std::min<size_t>(spk::MATEVAL_KC, count - k0);
    spk::MatEvalArgs a;
    for (int m = 0; m < 3; ++m) a.m[m] = s->row[m].view();
    for (size_t j = 0; j < (size_t)spk::MATEVAL_KC; ++j) {  // (the unused slots of a ragged chunk are never dereferenced)
      a.tx[j] = tx[k0 + (j < kc ? j : 0)]->d;
      a.ty[j] = ty[k0 + (j < kc ? j : 0)]->d;
    }
    a.partials = partials;
    a.tickets = tickets;
    a.out = d_out + 3 * k0;
    a.kc = (int)kc;
    // structure once per chunk (4-byte index + code, row pointers of both classes) + one 32-byte gather per entry and pair + T_x once per matrix and pair
    const uint64_t bytes = 5ull * nnz + 24ull * nrows + kc * (32ull * nnz + 96ull * nrows);
    c->timed_kernel("matrix_evals_batched", bytes, spk::k_matrix_evals_batched, dim3((unsigned)blocks, 3), dim3(256), a, nrows);
  }
  SP_HIP(hipMemcpyAsync(out, d_out, count * 3 * sizeof(fe_t), hipMemcpyDeviceToHost, c->stream));
  SP_HIP(sp::stream_sync(c->stream));
  return SP_OK;
}

// ---- is_sat / is_sat_relaxed (src/r1cs/mod.rs:358-394, :430-471) -----------------------------------------------------------------------------------
// The residual pass over `count` instances of n rows each: bitmaps and (count, first) pairs in the context's workspaces, one launch per SAT_BATCH
// instances, then an ordinary copy of the pairs; a bitmap is fetched only for an instance with failing rows, from the word of its first one on.
static int residual_run(sp_ctx* c, const sp_table* const* az, const sp_table* const* bz, const sp_table* const* cz, const uint64_t* u, const sp_table* const* E,
                        size_t count, size_t n, sp_sat_report* out) {
  if (!out || (count && (!az || !bz || !cz))) return fail(SP_ERR_INVALID_INPUT_LENGTH, "r1cs_residual: null argument");
  if (n < 1) return fail(SP_ERR_INVALID_INPUT_LENGTH, "r1cs_residual: n must be at least 1");
  for (size_t k = 0; k < count; ++k) {
    if (!az[k] || !bz[k] || !cz[k] || (E && !E[k])) return fail(SP_ERR_INVALID_INPUT_LENGTH, "r1cs_residual: null table");
    if (az[k]->len < n || bz[k]->len < n || cz[k]->len < n || (E && E[k]->len < n)) return fail(SP_ERR_INVALID_INPUT_LENGTH, "r1cs_residual: a table is shorter than n");
  }
  if (count == 0) return SP_OK;
  const size_t words = (n + 63) / 64;
  unsigned long long* bitmap = (unsigned long long*)c->workspace(sp_ctx::WS_SAT_BITMAP, count * words * 8);
  unsigned long long* summary = (unsigned long long*)c->workspace(sp_ctx::WS_SAT_SUMMARY, 2 * count * 8);  // counts, then first indices
  if (!bitmap || !summary) return SP_ERR_NO_DEVICE;
  SP_HIP(hipMemsetAsync(summary, 0, count * 8, c->stream));
  SP_HIP(hipMemsetAsync(summary + count, 0xff, count * 8, c->stream));
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  for (size_t k0 = 0; k0 < count; k0 += spk::SAT_BATCH) {
    const size_t nb = std::min<size_t>(spk::SAT_BATCH, count - k0);
    spk::SatArgs a;
    memset(&a, 0, sizeof a);
    for (size_t j = 0; j < nb; ++j) {
      const size_t k = k0 + j;
      spk::SatInst& in = a.inst[j];
      in.az = az[k]->d;
      in.bz = bz[k]->d;
      in.cz = cz[k]->d;
      in.E = E ? E[k]->d : nullptr;
      if (u) memcpy(&in.u, u + 4 * k, 32);
      in.bitmap = bitmap + k * words;
      in.count = summary + k;
      in.first = summary + count + k;
    }
    const uint64_t bytes = (uint64_t)nb * ((E ? 128ull : 96ull) * n + 8ull * words);
    const dim3 grid((unsigned)blocks, (unsigned)nb), block(256);
    if (u && E) c->timed_kernel("r1cs_residual", bytes, spk::k_r1cs_residual<true, true>, grid, block, a, n);
    else if (u) c->timed_kernel("r1cs_residual", bytes, spk::k_r1cs_residual<true, false>, grid, block, a, n);
    else if (E) c->timed_kernel("r1cs_residual", bytes, spk::k_r1cs_residual<false, true>, grid, block, a, n);
    else c->timed_kernel("r1cs_residual", bytes, spk::k_r1cs_residual<false, false>, grid, block, a, n);
  }
  std::vector<unsigned long long> sum(2 * count);
  SP_HIP(hipMemcpyAsync(sum.data(), summary, 2 * count * 8, hipMemcpyDeviceToHost, c->stream));
  SP_HIP(sp::stream_sync(c->stream));
  std::vector<unsigned long long> chunk;
  for (size_t k = 0; k < count; ++k) {
    sp_sat_report& r = out[k];
    memset(&r, 0, sizeof r);
    r.num_failing = sum[k];
    if (!r.num_failing) continue;
    const uint64_t want = r.num_failing < 16 ? r.num_failing : 16;
    for (size_t w = (size_t)(sum[count + k] >> 6); w < words && r.num_listed < want;) {
      const size_t take = std::min<size_t>(4096, words - w);
      chunk.resize(take);
      SP_HIP(hipMemcpy(chunk.data(), bitmap + k * words + w, take * 8, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < take && r.num_listed < want; ++i)
        for (unsigned long long m = chunk[i]; m && r.num_listed < want; m &= m - 1) r.first[r.num_listed++] = 64 * (uint64_t)(w + i) + (uint64_t)(__builtin_ffsll((long long)m) - 1);
      w += take;
    }
  }
  return SP_OK;
}

int sp_r1cs_residual(sp_ctx* c, const sp_table* az, const sp_table* bz, const sp_table* cz, const uint64_t* u, const sp_table* E, size_t n, sp_sat_report* out) {
  return residual_run(c, &az, &bz, &cz, u, E ? &E : nullptr, 1, n, out);
}
int sp_r1cs_residual_batched(sp_ctx* c, const sp_table* const* az, const sp_table* const* bz, const sp_table* const* cz, const uint64_t* u, const sp_table* const* E,
                             size_t count, size_t n, sp_sat_report* out) {
  return residual_run(c, az, bz, cz, u, E, count, n, out);
}
int sp_shape_is_sat(sp_ctx* c, const sp_shape* s, const sp_table* z, const uint64_t* u, const sp_table* E, sp_sat_report* out) {
  if (!s || !z || !out) return fail(SP_ERR_INVALID_INPUT_LENGTH, "shape_is_sat: null argument");
  const size_t nrows = s->dims.num_cons;
  if (z->len != s->num_cols) return fail(SP_ERR_INVALID_WITNESS_LENGTH, "shape_is_sat: z has the wrong length");
  fe_t* prod = (fe_t*)c->workspace(sp_ctx::WS_SAT_PRODUCTS, 3 * nrows * sizeof(fe_t));
  if (!prod) return SP_ERR_NO_DEVICE;
  sp_table t[3];
  for (int m = 0; m < 3; ++m) {
    t[m].ctx = c;
    t[m].d = prod + (size_t)m * nrows;
    t[m].cap = t[m].len = nrows;
    t[m].view = true;
  }
  int rc = sp_multiply_vec(c, s, z, &t[0], &t[1], &t[2]);
  if (rc) return rc;
  return sp_r1cs_residual(c, &t[0], &t[1], &t[2], u, E, nrows, out);
}

}  // extern "C"

// ---- sp_nifs_layers_batch's half on this side of the shape (core.hpp) ----------------------------------------------------------------------------------
size_t sp_nifs_layers_chunk(void) { return (size_t)spk::NIFS_LAYERS_KC; }
namespace sp {
const sp_dims& shape_dims(const sp_shape* s) { return s->dims; }
int nifs_layers_launch(sp_ctx* c, const sp_shape* s, std::vector<NifsLayerVec>& vecs, const std::vector<fe_t>& tails, size_t tail_len) {
  const size_t nvec = vecs.size(), nrows = s->dims.num_cons, KC = (size_t)spk::NIFS_LAYERS_KC;
  if (nvec == 0 || nrows == 0) return SP_OK;
  if (nvec > 0xffffffffull - KC || s->num_vars > 0xffffffffull) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_nifs_layers_batch: too many vectors / variables for 32-bit indices");
  const size_t tail_bytes = tails.size() * sizeof(fe_t), bytes_all = tail_bytes + nvec * sizeof(NifsLayerVec);
  char* d = (char*)c->workspace(sp_ctx::WS_NIFS_LAYERS, bytes_all);
  if (!d) return SP_ERR_NO_DEVICE;
  const fe_t* d_tails = (const fe_t*)d;
  for (NifsLayerVec& v : vecs) v.tail = d_tails + (size_t)(uintptr_t)v.tail * tail_len;
  if (tail_bytes) SP_HIP(hipMemcpyAsync(d, tails.data(), tail_bytes, hipMemcpyHostToDevice, c->stream));
  SP_HIP(hipMemcpyAsync(d + tail_bytes, vecs.data(), nvec * sizeof(NifsLayerVec), hipMemcpyHostToDevice, c->stream));
  SP_HIP(sp::stream_sync(c->stream));  // the host arrays are only borrowed for the duration of the call
  spk::NifsLayersArgs a;
  for (int m = 0; m < 3; ++m) a.m[m] = s->row[m].view();
  a.vecs = (const NifsLayerVec*)(d + tail_bytes);
  a.nvec = (unsigned)nvec;
  a.num_vars = (unsigned)s->num_vars;
  size_t blocks = (nrows + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const uint64_t nnz = s->nnz[0] + s->nnz[1] + s->nnz[2];
  const size_t chunks = (nvec + KC - 1) / KC;
  for (size_t c0 = 0; c0 < chunks; c0 += 65535) {  // (gridDim.z is 16 bits wide)
    const size_t nz = std::min<size_t>(65535, chunks - c0), nv = std::min(nvec - c0 * KC, nz * KC);
    a.chunk0 = (unsigned)c0;
    // per chunk the structure once (4-byte index + code, row pointers of both classes); per vector one 32-byte gather per entry and the 3 outputs
    const uint64_t bytes = nz * (5ull * nnz + 24ull * nrows) + nv * (32ull * nnz + 96ull * nrows);
    c->timed_kernel("nifs_layers", bytes, spk::k_nifs_layers, dim3((unsigned)blocks, 3, (unsigned)nz), dim3(256), a, nrows);
  }
  return SP_OK;
}
}  // namespace sp
