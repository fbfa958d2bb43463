// An evaluator for the field arithmetic of field.hpp and the reductions of device_utils.hpp: it reads records, computes, writes results, and compares
// nothing - the judge is tests/test_field_host.py with Python integers. Built and run by that file.
//
//   fq_check host IN OUT     the 32-bit-limb algorithms on the host (no GPU is touched): fe_mul_limb32, fe_add, fe_sub, fe_neg, fe_dbl, both fields
//   fq_check device IN OUT   the same ops on the device plus the device-only ones, in a lone wave first and in full 256-thread blocks after it
//
// IN is a sequence of records {u32 op; u32 a[8]; u32 b[8]} (68 bytes), OUT one 8 x u32 result per record, in order; in device mode the lone wave's results
// for the first min(n, LONE) records follow (element-wise ops only; the other slots are zero). Ops:
//   element-wise      MUL_FQ fe_mul<FqP>, MUL_FP fe_mul_rowwise<FpP> (host: fe_mul_limb32 of that field), CHAIN_FQ a 64-deep dependent chain of fe_mul<FqP>
//                     (device only), ADD / SUB / NEG / DBL of both fields, UNIFORM_FQ fe_from_uniform<FqP> of the 64 bytes a || b (device only),
//                     LAZY_REDUCE lazy_reduce of the 9-word value a + b[0] 2^256 (device only)
//   per wave          LAZY_WAVE lazy_reduce(lazy_wave_sum(lazy_from(a))) and WAVE_SUM_T wave_sum(a) in blocks of T threads: every record gets the sum of
//                     the 64 records of its wave
//   per block         BLOCK_SUM_T block_sum<3> of (a, b, a - b) over groups of T records in one block of T threads: the group's first three records get
//                     the three sums, the others zero
// Runs of records with one per-wave / per-block op must be a multiple of 64 / T long. Every device step is followed by hipDeviceSynchronize; at the first
// error the program exits non-zero and launches nothing more.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../spartan2_amd/csrc/device_utils.hpp"

enum Op : uint32_t {
  MUL_FQ = 1, MUL_FP, CHAIN_FQ, ADD_FQ, SUB_FQ, NEG_FQ, DBL_FQ, ADD_FP, SUB_FP, NEG_FP, DBL_FP, UNIFORM_FQ, LAZY_REDUCE,  // element-wise
  LAZY_WAVE, WAVE_SUM_64, WAVE_SUM_128, WAVE_SUM_256,                                                                    // per wave
  BLOCK_SUM_64, BLOCK_SUM_128, BLOCK_SUM_256,                                                                            // per block
  OP_END
};
struct rec_t {
  uint32_t op;
  uint32_t a[8], b[8];
};
struct out_t {
  uint32_t v[8];
};
static_assert(sizeof(rec_t) == 68 && sizeof(out_t) == 32, "record layout");

__host__ __device__ inline fe_t load_fe(const uint32_t w[8]) {
  fe_t r;
  for (int i = 0; i < 8; ++i) r.v[i] = w[i];
  return r;
}
__host__ __device__ inline void store_fe(out_t* o, const fe_t& x) {
  for (int i = 0; i < 8; ++i) o->v[i] = x.v[i];
}
// the ops both modes share; false when `op` is not one of them
__host__ __device__ inline bool eval_shared(uint32_t op, const fe_t& a, const fe_t& b, fe_t* r) {
  switch (op) {
    case ADD_FQ: *r = fe_add<FqP>(a, b); return true;
    case SUB_FQ: *r = fe_sub<FqP>(a, b); return true;
    case NEG_FQ: *r = fe_neg<FqP>(a); return true;
    case DBL_FQ: *r = fe_dbl<FqP>(a); return true;
    case ADD_FP: *r = fe_add<FpP>(a, b); return true;
    case SUB_FP: *r = fe_sub<FpP>(a, b); return true;
    case NEG_FP: *r = fe_neg<FpP>(a); return true;
    case DBL_FP: *r = fe_dbl<FpP>(a); return true;
    default: return false;
  }
}

// element-wise ops, grid-stride over records [0, n); records of other ops get zero
__global__ void k_elem(const rec_t* __restrict__ in, out_t* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t op = in[i].op;
    const fe_t a = load_fe(in[i].a), b = load_fe(in[i].b);
    fe_t r = fe_zero();
    if (!eval_shared(op, a, b, &r)) {
      if (op == MUL_FQ) {
        r = fe_mul<FqP>(a, b);
      } else if (op == MUL_FP) {
        r = fe_mul_rowwise<FpP>(a, b);
      } else if (op == CHAIN_FQ) {
        r = a;
        for (int k = 0; k < 64; ++k) r = fe_mul<FqP>(r, (k & 1) ? b : r);
      } else if (op == UNIFORM_FQ) {
        uint8_t bytes[64];
        for (int w = 0; w < 8; ++w)
          for (int j = 0; j < 4; ++j) {
            bytes[4 * w + j] = (uint8_t)(a.v[w] >> (8 * j));
            bytes[32 + 4 * w + j] = (uint8_t)(b.v[w] >> (8 * j));
          }
        r = fe_from_uniform<FqP>(bytes);
      } else if (op == LAZY_REDUCE) {
        spk::lazy9_t l;
        for (int w = 0; w < 8; ++w) l.v[w] = a.v[w];
        l.v[8] = b.v[0];
        r = spk::lazy_reduce(l);
      }
    }
    store_fe(&out[i], r);
  }
}
// per-wave ops on records [first, first + cnt), cnt a multiple of 64: a wave past the end leaves as a whole
__global__ void k_wave(const rec_t* __restrict__ in, out_t* __restrict__ out, size_t first, size_t cnt, int lazy) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const fe_t a = load_fe(in[first + i].a);
  store_fe(&out[first + i], lazy ? spk::lazy_reduce(spk::lazy_wave_sum(spk::lazy_from(a))) : spk::wave_sum(a));
}
// block_sum<3> on groups of blockDim.x records starting at `first`; one block per group
__global__ void k_block(const rec_t* __restrict__ in, out_t* __restrict__ out, size_t first) {
  __shared__ fe_t smem[3 * 4];
  const size_t i = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const fe_t a = load_fe(in[i].a), b = load_fe(in[i].b);
  fe_t acc[3] = {a, b, fe_sub<FqP>(a, b)};
  spk::block_sum<3>(acc, smem);
  if (threadIdx.x == 0) {
    for (int k = 0; k < 3; ++k) store_fe(&out[i + k], acc[k]);
  } else if (threadIdx.x >= 3) {
    store_fe(&out[i], fe_zero());
  }
}

#if !defined(__HIP_DEVICE_COMPILE__)
static const size_t LONE = 4096;  // records the lone wave walks

static int fail(const char* what) {
  fprintf(stderr, "fq_check: %s\n", what);
  return 2;
}
static bool sync_ok(const char* what) {
  const hipError_t e1 = hipGetLastError(), e2 = hipDeviceSynchronize();
  if (e1 == hipSuccess && e2 == hipSuccess) return true;
  fprintf(stderr, "fq_check: %s: %s\n", what, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
  return false;
}
static int group_of(uint32_t op) {  // records per launch group of a per-wave / per-block op, 0 for element-wise ops
  switch (op) {
    case LAZY_WAVE: case WAVE_SUM_64: case BLOCK_SUM_64: return 64;
    case WAVE_SUM_128: case BLOCK_SUM_128: return 128;
    case WAVE_SUM_256: case BLOCK_SUM_256: return 256;
    default: return 0;
  }
}
#endif

int main(int argc, char** argv) {
#if !defined(__HIP_DEVICE_COMPILE__)
  if (argc != 4 || (strcmp(argv[1], "host") && strcmp(argv[1], "device"))) return fail("usage: fq_check host|device IN OUT");
  const bool device = !strcmp(argv[1], "device");
  FILE* f = fopen(argv[2], "rb");
  if (!f) return fail("cannot open IN");
  fseek(f, 0, SEEK_END);
  const long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (sz <= 0 || sz % (long)sizeof(rec_t)) return fail("IN is not a whole number of records");
  const size_t n = (size_t)sz / sizeof(rec_t);
  std::vector<rec_t> rec(n);
  if (fread(rec.data(), sizeof(rec_t), n, f) != n) return fail("short read");
  fclose(f);
  for (size_t i = 0; i < n; ++i)
    if (rec[i].op == 0 || rec[i].op >= OP_END) return fail("unknown op");
  std::vector<out_t> out(n), lone;
  memset(out.data(), 0, n * sizeof(out_t));

  if (!device) {
    for (size_t i = 0; i < n; ++i) {
      const fe_t a = load_fe(rec[i].a), b = load_fe(rec[i].b);
      fe_t r;
      if (rec[i].op == MUL_FQ) r = fe_mul_limb32<FqP>(a, b);
      else if (rec[i].op == MUL_FP) r = fe_mul_limb32<FpP>(a, b);
      else if (!eval_shared(rec[i].op, a, b, &r)) return fail("op is device-only");
      store_fe(&out[i], r);
    }
  } else {
    // every run of a grouped op must fill its groups: checked before anything is launched
    for (size_t i = 0; i < n;) {
      size_t j = i;
      while (j < n && rec[j].op == rec[i].op) ++j;
      const int g = group_of(rec[i].op);
      if (g && (j - i) % g) return fail("a run of a per-wave / per-block op is not a whole number of groups");
      i = j;
    }
    rec_t* d_in;
    out_t* d_out;
    if (hipMalloc((void**)&d_in, n * sizeof(rec_t)) != hipSuccess || hipMalloc((void**)&d_out, n * sizeof(out_t)) != hipSuccess) return fail("hipMalloc");
    if (hipMemcpy(d_in, rec.data(), n * sizeof(rec_t), hipMemcpyHostToDevice) != hipSuccess) return fail("copy in");
    // a lone wave over the first records, then everything in full blocks
    const size_t nl = n < LONE ? n : LONE;
    lone.resize(nl);
    if (hipMemset(d_out, 0, n * sizeof(out_t)) != hipSuccess) return fail("memset");
    hipLaunchKernelGGL(k_elem, dim3(1), dim3(64), 0, 0, d_in, d_out, nl);
    if (!sync_ok("k_elem, lone wave")) return 2;
    if (hipMemcpy(lone.data(), d_out, nl * sizeof(out_t), hipMemcpyDeviceToHost) != hipSuccess) return fail("copy out");
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_elem, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, 0, d_in, d_out, n);
    if (!sync_ok("k_elem, full blocks")) return 2;
    for (size_t i = 0; i < n;) {
      size_t j = i;
      while (j < n && rec[j].op == rec[i].op) ++j;
      const uint32_t op = rec[i].op;
      const int g = group_of(op);
      const size_t cnt = j - i;
      if (op == LAZY_WAVE) {
        hipLaunchKernelGGL(k_wave, dim3(1), dim3(64), 0, 0, d_in, d_out, i, (size_t)64, 1);  // its first wave alone
        if (!sync_ok("k_wave lazy, lone wave")) return 2;
        hipLaunchKernelGGL(k_wave, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0, d_in, d_out, i, cnt, 1);
        if (!sync_ok("k_wave lazy")) return 2;
      } else if (op == WAVE_SUM_64 || op == WAVE_SUM_128 || op == WAVE_SUM_256) {
        hipLaunchKernelGGL(k_wave, dim3((unsigned)(cnt / g)), dim3(g), 0, 0, d_in, d_out, i, cnt, 0);
        if (!sync_ok("k_wave")) return 2;
      } else if (g) {
        hipLaunchKernelGGL(k_block, dim3((unsigned)(cnt / g)), dim3(g), 0, 0, d_in, d_out, i);
        if (!sync_ok("k_block")) return 2;
      }
      i = j;
    }
    if (hipMemcpy(out.data(), d_out, n * sizeof(out_t), hipMemcpyDeviceToHost) != hipSuccess) return fail("copy out");
    hipFree(d_in);
    hipFree(d_out);
  }
  FILE* o = fopen(argv[3], "wb");
  if (!o) return fail("cannot open OUT");
  if (fwrite(out.data(), sizeof(out_t), n, o) != n || (lone.size() && fwrite(lone.data(), sizeof(out_t), lone.size(), o) != lone.size())) return fail("short write");
  fclose(o);
  printf("%s: %zu records\n", argv[1], n);
  return 0;
#else
  return 0;
#endif
}
