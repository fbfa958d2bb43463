// R1CSShape::is_sat / is_sat_relaxed (src/r1cs/mod.rs:358-394, :430-471): the residual pass behind the matrix-vector product.
//   k_r1cs_residual   row i fails when Az[i] Bz[i] - u Cz[i] - E[i] != 0 (Montgomery form; u absent = 1, E absent = 0: the plain check of :375, both present:
//                     the relaxed one of :444). Streaming: one row a lane, a wave reads 2 KiB contiguous per table like the bind kernels; 96 - 128 bytes a row.
// Outputs per instance (grid y = instance, all of equal n):
//   bitmap   ceil(n / 64) words, one per wave: the wave's 64-bit ballot, stored by lane 0 (0 for a wave without a failing row)
//   summary  count = number of failing rows, first = smallest failing index: one atomicAdd and one atomicMin per wave, from waves with a non-zero mask only -
//            a satisfied instance issues no atomics. The host presets count = 0, first = ~0.
#pragma once
#include "device_utils.hpp"

namespace spk {

constexpr unsigned SAT_BATCH = 16;  // instances a launch (the pointers travel as kernel arguments)
struct SatInst {
  const fe_t *az, *bz, *cz, *E;
  fe_t u;
  unsigned long long* bitmap;
  unsigned long long* count;
  unsigned long long* first;
};
struct SatArgs {
  SatInst inst[SAT_BATCH];
};

template <bool HAS_U, bool HAS_E>
__global__ void __launch_bounds__(256) k_r1cs_residual(SatArgs a, size_t n) {
  typedef FqP S;
  const SatInst& in = a.inst[blockIdx.y];
  const fe_t* __restrict__ az = in.az;
  const fe_t* __restrict__ bz = in.bz;
  const fe_t* __restrict__ cz = in.cz;
  const fe_t* __restrict__ E = in.E;
  const unsigned lane = threadIdx.x & 63u;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t wbase = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); wbase < n; wbase += stride) {  // (uniform over a wave)
    const size_t row = wbase + lane;
    bool bad = false;
    if (row < n) {
      const fe_t x = az[row], y = bz[row];
      fe_t c = cz[row];
      if (HAS_U) c = fe_mul<S>(in.u, c);
      fe_t r = fe_sub<S>(fe_mul<S>(x, y), c);
      if (HAS_E) r = fe_sub<S>(r, E[row]);
      bad = !fe_is_zero(r);
    }
    const unsigned long long mask = __ballot(bad);
    if (lane == 0) {
      in.bitmap[wbase >> 6] = mask;
      if (mask) {
        atomicAdd(in.count, (unsigned long long)__popcll(mask));
        atomicMin(in.first, (unsigned long long)wbase + (unsigned long long)(__ffsll((long long)mask) - 1));
      }
    }
  }
}

}  // namespace spk
