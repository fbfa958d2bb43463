// The pieces of the table kernels that more than one kernel header uses (kernels_poly.hpp, kernels_lockstep.hpp): the self-validating result slot of the
// mapped pinned buffer and the one-block eq pyramid. Inline device code only - every translation unit may include it.
#pragma once
#include "device_utils.hpp"

namespace spk {

// Block partials of an evaluation launch. Up to HOST_SUM_MAX_BLOCKS blocks: every block writes its NACC sums and the sequence number into its own
// 128-byte slot of the mapped pinned buffer and the HOST adds them (a few dozen 256-bit additions) — no second-stage launch on the per-round
// critical path. Larger grids store to device memory for k_sum_partials.
constexpr int HOST_SUM_MAX_BLOCKS = 64;
constexpr int SLOT_BASE_ELEM = 64;  // element index of slot 0 in the mapped buffer; slot b = 4 elements: sums[0..3), word 0 of the 4th = sequence
// A slot is self-validating: element 3 carries the sequence number TWICE (words 0 and 3) and two independent check words over the data
// (word 1 = sequence + plain sum, word 2 = sequence * K + position-weighted sum), so the host accepts a slot only when all of it has landed,
// whatever order the stores reach host memory in, and the producer needs no fence for it. A torn read would have to match both 32-bit
// checks (2^-64 for unrelated stale words) and both copies of the sequence number.
struct slot_chk {
  unsigned a, b;
};
constexpr unsigned SLOT_CHK_K = 0x9E3779B1u;
// the same arithmetic on the host side of capi_core.hip (wait_slot / reduce_partials_wait)
__host__ __device__ __forceinline__ void slot_chk_add(slot_chk& c, const fe_t& v, int k) {
  // c.b += sum_i (8k + i + 1) v_i, written as (8k + 1) sum_i v_i + sum_i i v_i (the same value mod 2^32): with a run-time k the weights are ONE per-lane
  // value instead of eight - the resident tail's compiler hoisted the eight out of its round loop and spilled them (tools/spill_report.py)
  unsigned plain = 0, ramp = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    plain += v.v[i];
    ramp += (unsigned)i * v.v[i];
  }
  c.a += plain;
  c.b += (unsigned)(8 * k + 1) * plain + ramp;
}
// (mapped host memory is uncached on the device side: plain stores go straight out, as two 16-byte writes per element and two 8-byte tag halves)
__device__ __forceinline__ void slot_store_elem(fe_t* dst, const fe_t& v) { *dst = v; }
__device__ __forceinline__ void slot_store_tag(fe_t* slot, unsigned seq, const slot_chk& c) {
  const unsigned long long hi = ((unsigned long long)seq << 32) | (seq * SLOT_CHK_K + c.b);  // words 2, 3
  const unsigned long long lo = ((unsigned long long)(seq + c.a) << 32) | seq;               // words 0, 1 (word 0 is what the host polls)
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(&slot[3].v[2]), hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(&slot[3].v[0]), lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- K8: eq pyramids ---------------------------------------------------------------------------------------------
// level k of a pyramid (2^k entries) sits at out + 2^k - 1
__host__ __device__ __forceinline__ size_t eq_level_offset(int k) { return ((size_t)1 << k) - 1; }
// One level of the pyramid per barrier. The levels of up to 1024 entries are kept in LDS as well (in place: entry i of level k becomes entries i and
// 2^k + i of level k + 1), so a level costs an LDS round trip + one product instead of a store to and a load from the L2 (1.5 -> 0.7 us per level; the
// pyramids of tau and of r_x stand in front of the first evaluation of the outer and of the inner sum-check); the global stores are fire-and-forget.
constexpr int EQ_LDS_ENTRIES = 1024;
__device__ __forceinline__ void eq_levels_block(const fe_t* v_rev /* v_rev[k] = the challenge of level k */, int m, fe_t* __restrict__ out, fe_t* lv) {
  if (threadIdx.x == 0) {
    out[0] = fe_one<S>();
    lv[0] = fe_one<S>();
  }
  __syncthreads();
  for (int k = 0; k < m; ++k) {
    const fe_t r = v_rev[-k];
    fe_t* next = out + eq_level_offset(k + 1);
    const size_t size = (size_t)1 << k;
    if (2 * size <= (size_t)EQ_LDS_ENTRIES) {
      for (size_t i = threadIdx.x; i < size; i += blockDim.x) {
        const fe_t e = lv[i];
        const fe_t y = fe_mul<S>(e, r), x = fe_sub<S>(e, y);
        lv[size + i] = y;
        lv[i] = x;
        next[size + i] = y;
        next[i] = x;
      }
    } else {
      const fe_t* prev = out + eq_level_offset(k);
      for (size_t i = threadIdx.x; i < size; i += blockDim.x) {
        const fe_t e = prev[i];
        const fe_t y = fe_mul<S>(e, r);
        next[size + i] = y;
        next[i] = fe_sub<S>(e, y);
      }
    }
    __syncthreads();
  }
}

}  // namespace spk
