// An evaluator for the point-addition routines of curve.hpp and coop_add.hpp: it reads records, computes, writes results, and compares nothing - the
// judge is tests/test_group_host.py, which normalises every result in Python integers and compares it with (a + b) H from the oracle. Built and run by
// that file.
//
//   group_check host IN OUT     xyzz_add, xyzz_add_mixed, xyzz_dbl, jac_add, jac_add_mixed, jac_dbl as the host compiles them (no GPU is touched)
//   group_check device IN OUT   the same ops in 256-thread blocks, and xyzz_add_block4<64> as ONE block of 256 threads per 64 records
//
// IN is a sequence of records {u32 op; u32 p[32]; u32 q[32]} (260 bytes), OUT 32 words per record, in order. An operand is four base-field elements
// in Montgomery form: (X, Y, ZZ, ZZZ) for the xyzz ops, (X, Y, Z, -) for the Jacobian ops, (x, y, -, -) for the affine second operand of the mixed ops;
// a result has the layout of its op's return type, unused words zero. Bit 31 of `op` on a BLOCK4 record: the item does not take part (`active` false),
// its result is the untouched first operand - the full-EXEC products still run on it. A run of BLOCK4 records must be a multiple of 64 long. Every
// device step is followed by hipDeviceSynchronize; at the first error the program exits non-zero and launches nothing more.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../spartan2_amd/csrc/coop_add.hpp"

enum Op : uint32_t { XYZZ_ADD = 1, XYZZ_ADD_MIXED, XYZZ_DBL, JAC_ADD, JAC_ADD_MIXED, JAC_DBL, BLOCK4, OP_END };
constexpr uint32_t INACTIVE = 0x80000000u;
struct rec_t {
  uint32_t op;
  uint32_t p[32], q[32];
};
struct out_t {
  uint32_t v[32];
};
static_assert(sizeof(rec_t) == 260 && sizeof(out_t) == 128 && sizeof(xyzz_t) == 128 && sizeof(jac_t) == 96 && sizeof(aff_t) == 64, "record layout");

__host__ __device__ inline fe_t load_fe(const uint32_t* w) {
  fe_t r;
  for (int i = 0; i < 8; ++i) r.v[i] = w[i];
  return r;
}
__host__ __device__ inline xyzz_t load_xyzz(const uint32_t* w) {
  xyzz_t r;
  r.x = load_fe(w), r.y = load_fe(w + 8), r.zz = load_fe(w + 16), r.zzz = load_fe(w + 24);
  return r;
}
__host__ __device__ inline jac_t load_jac(const uint32_t* w) {
  jac_t r;
  r.x = load_fe(w), r.y = load_fe(w + 8), r.z = load_fe(w + 16);
  return r;
}
__host__ __device__ inline aff_t load_aff(const uint32_t* w) {
  aff_t r;
  r.x = load_fe(w), r.y = load_fe(w + 8);
  return r;
}
__host__ __device__ inline void store_fe(uint32_t* w, const fe_t& x) {
  for (int i = 0; i < 8; ++i) w[i] = x.v[i];
}
__host__ __device__ inline void store_xyzz(out_t* o, const xyzz_t& r) {
  store_fe(o->v, r.x), store_fe(o->v + 8, r.y), store_fe(o->v + 16, r.zz), store_fe(o->v + 24, r.zzz);
}
__host__ __device__ inline void store_jac(out_t* o, const jac_t& r) {
  store_fe(o->v, r.x), store_fe(o->v + 8, r.y), store_fe(o->v + 16, r.z);
  for (int i = 24; i < 32; ++i) o->v[i] = 0;
}
// the lane-private ops; false when `op` is not one of them
__host__ __device__ inline bool eval_one(const rec_t& r, out_t* o) {
  switch (r.op) {
    case XYZZ_ADD: store_xyzz(o, xyzz_add(load_xyzz(r.p), load_xyzz(r.q))); return true;
    case XYZZ_ADD_MIXED: store_xyzz(o, xyzz_add_mixed(load_xyzz(r.p), load_aff(r.q))); return true;
    case XYZZ_DBL: store_xyzz(o, xyzz_dbl(load_xyzz(r.p))); return true;
    case JAC_ADD: store_jac(o, jac_add(load_jac(r.p), load_jac(r.q))); return true;
    case JAC_ADD_MIXED: store_jac(o, jac_add_mixed(load_jac(r.p), load_aff(r.q))); return true;
    case JAC_DBL: store_jac(o, jac_dbl(load_jac(r.p))); return true;
    default: return false;
  }
}

// lane-private ops, grid-stride over records [0, n); BLOCK4 records are left alone
__global__ void __launch_bounds__(256) k_elem(const rec_t* __restrict__ in, out_t* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    out_t o;
    if (eval_one(in[i], &o)) out[i] = o;
  }
}
// xyzz_add_block4<64> on records [first + 64 b, first + 64 b + 64) by block b: 256 threads, role = thread / 64, item = thread % 64, the sum written over
// the first operand as the kernels do (dst aliases P)
__global__ void __launch_bounds__(256) k_block4(const rec_t* __restrict__ in, out_t* __restrict__ out, size_t first) {
  __shared__ spk::CoopAdd<64> L;
  __shared__ xyzz_t P[64], Q[64];
  const int role = threadIdx.x >> 6, i = threadIdx.x & 63;
  const size_t r = first + (size_t)blockIdx.x * 64 + i;
  const bool active = !(in[r].op & INACTIVE);
  if (role == 0) {
    P[i] = load_xyzz(in[r].p);
    Q[i] = load_xyzz(in[r].q);
  }
  __syncthreads();
  spk::xyzz_add_block4<64>(L, &P[i], &Q[i], P, role, i, active);
  if (role == 0) store_xyzz(&out[r], P[i]);
}

#if !defined(__HIP_DEVICE_COMPILE__)
static int fail(const char* what) {
  fprintf(stderr, "group_check: %s\n", what);
  return 2;
}
static bool sync_ok(const char* what) {
  const hipError_t e1 = hipGetLastError(), e2 = hipDeviceSynchronize();
  if (e1 == hipSuccess && e2 == hipSuccess) return true;
  fprintf(stderr, "group_check: %s: %s\n", what, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
  return false;
}
#endif

int main(int argc, char** argv) {
#if !defined(__HIP_DEVICE_COMPILE__)
  if (argc != 4 || (strcmp(argv[1], "host") && strcmp(argv[1], "device"))) return fail("usage: group_check host|device IN OUT");
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
  for (size_t i = 0; i < n; ++i) {
    const uint32_t op = rec[i].op & ~INACTIVE;
    if (op == 0 || op >= OP_END || ((rec[i].op & INACTIVE) && op != BLOCK4)) return fail("unknown op");
  }
  std::vector<out_t> out(n);
  memset(out.data(), 0, n * sizeof(out_t));

  if (!device) {
    for (size_t i = 0; i < n; ++i)
      if (!eval_one(rec[i], &out[i])) return fail("op is device-only");
  } else {
    // every run of BLOCK4 records must fill its blocks: checked before anything is launched
    for (size_t i = 0; i < n;) {
      size_t j = i;
      const bool b4 = (rec[i].op & ~INACTIVE) == BLOCK4;
      while (j < n && ((rec[j].op & ~INACTIVE) == BLOCK4) == b4) ++j;
      if (b4 && (j - i) % 64) return fail("a run of BLOCK4 records is not a whole number of blocks");
      i = j;
    }
    rec_t* d_in;
    out_t* d_out;
    if (hipMalloc((void**)&d_in, n * sizeof(rec_t)) != hipSuccess || hipMalloc((void**)&d_out, n * sizeof(out_t)) != hipSuccess) return fail("hipMalloc");
    if (hipMemcpy(d_in, rec.data(), n * sizeof(rec_t), hipMemcpyHostToDevice) != hipSuccess) return fail("copy in");
    if (hipMemset(d_out, 0, n * sizeof(out_t)) != hipSuccess) return fail("memset");
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_elem, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, 0, d_in, d_out, n);
    if (!sync_ok("k_elem")) return 2;
    for (size_t i = 0; i < n;) {
      size_t j = i;
      const bool b4 = (rec[i].op & ~INACTIVE) == BLOCK4;
      while (j < n && ((rec[j].op & ~INACTIVE) == BLOCK4) == b4) ++j;
      if (b4) {
        hipLaunchKernelGGL(k_block4, dim3((unsigned)((j - i) / 64)), dim3(256), 0, 0, d_in, d_out, i);
        if (!sync_ok("k_block4")) return 2;
      }
      i = j;
    }
    if (hipMemcpy(out.data(), d_out, n * sizeof(out_t), hipMemcpyDeviceToHost) != hipSuccess) return fail("copy out");
    hipFree(d_in);
    hipFree(d_out);
  }
  FILE* o = fopen(argv[3], "wb");
  if (!o) return fail("cannot open OUT");
  if (fwrite(out.data(), sizeof(out_t), n, o) != n) return fail("short write");
  fclose(o);
  printf("%s: %zu records\n", argv[1], n);
  return 0;
#else
  return 0;
#endif
}
