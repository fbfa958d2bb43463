// Witness generation for the SHA-256 circuits on the device (sp_sha256_witness): the kernel form of sp_frontend::sha256_plan_eval
// (frontend/sha256_witness_plan.hpp), which is its specification.
//
// One workgroup per (message, block, split). The host has hashed the message and uploads, per block, the chaining value the block starts from and its 16
// message words (B dependent compressions are microseconds on the host and would be one lane's serial walk here). The workgroup
//   (a) fills the block's trace (frontend/sha256_trace_layout.h: 841 slots of 8 bytes, 6.6 KiB of LDS) - the schedule and the 64 rounds' two running
//       sums are one lane's serial work (every block of every message in parallel), the per-round and per-schedule-word XOR / ch / maj words are then
//       derived by 112 lanes from the stored sums -, and
//   (b) streams its share of the block's descriptors (coalesced 4-byte loads), picks each variable's bit from LDS and stores the element: 0 or the
//       field's ONE in Montgomery form, 32 contiguous bytes a lane, 2 KiB a wave.
// `splits` workgroups share a block's descriptors (each fills the trace for itself: ~7 KiB of LDS writes against ~26 k elements of stores), so a
// 33-block message still covers the device.
#pragma once
#include "../frontend/sha256_trace_layout.h"
#include "device_utils.hpp"

namespace spk {

__constant__ uint32_t SHA256_ROUND_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
    0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
    0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
    0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
    0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
    0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

constexpr unsigned SHA_WIT_THREADS = 256;
constexpr unsigned SHA_WIT_BLOCK_WORDS = 24;  // per (message, block) in `blocks`: 8 chaining words, 16 message words

__device__ __forceinline__ uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// desc: n_aux descriptors; block_starts: n_blocks + 1; the first n_pre variables are preimage bits, 512 a block.
// blocks: n_msgs * n_blocks * SHA_WIT_BLOCK_WORDS words; tables[m] + off: where message m's n_aux elements go.
// grid = (n_msgs * n_blocks, splits)
__global__ void __launch_bounds__(SHA_WIT_THREADS) k_sha256_witness(const uint32_t* __restrict__ desc, const uint32_t* __restrict__ block_starts, uint32_t n_pre,
                                                                    uint32_t n_blocks, const uint32_t* __restrict__ blocks, fe_t* const* __restrict__ tables, size_t off) {
  namespace L = sha256_trace;
  __shared__ uint64_t T[L::SLOTS + 7];
  __shared__ uint32_t Hs[8];
  const unsigned t = threadIdx.x;
  const uint32_t m = blockIdx.x / n_blocks, b = blockIdx.x - m * n_blocks;
  const uint32_t* in = blocks + (size_t)blockIdx.x * SHA_WIT_BLOCK_WORDS;
  if (t < 8) Hs[t] = in[t];
  if (t >= 8 && t < 24) T[L::W + (t - 8)] = in[t];
  __syncthreads();
  if (t == 0) {
    // the serial spine: w[16..63] with their full sums and, per round, the two running sums. Both loops are one, fully unrolled, with the schedule in a
    // 16-word ring of registers: the chain of dependent operations then never waits for an LDS read (stores only), and the schedule's work fills the
    // gaps of the rounds' chain.
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = in[8 + i];
    uint32_t bb = Hs[1], c = Hs[2], d = Hs[3], f = Hs[5], g = Hs[6], h = Hs[7];
    uint64_t A = Hs[0], E = Hs[4];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      if (i >= 16) {
        const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
        const uint32_t s0 = sha_rotr(x, 7) ^ sha_rotr(x, 18) ^ (x >> 3), s1 = sha_rotr(y, 17) ^ sha_rotr(y, 19) ^ (y >> 10);
        const uint64_t sum = (uint64_t)w[i & 15] + s0 + (uint64_t)w[(i + 9) & 15] + s1;
        T[L::W + i] = sum;
        w[i & 15] = (uint32_t)sum;
      }
      const uint32_t e = (uint32_t)E, a = (uint32_t)A;
      T[L::ROUND + 9 * i + 0] = E;
      T[L::ROUND + 9 * i + 4] = A;
      const uint32_t S1 = sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25), ch = (e & f) ^ (~e & g);
      const uint32_t S0 = sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22), mj = (a & bb) ^ (a & c) ^ (bb & c);
      const uint64_t temp1 = (uint64_t)h + S1 + ch + SHA256_ROUND_K[i] + (uint64_t)w[i & 15];
      E = (uint64_t)d + temp1;
      A = temp1 + S0 + mj;
      h = g, g = f, f = e, d = c, c = bb, bb = a;
    }
    T[L::OUT + 0] = A + Hs[0];
    T[L::OUT + 1] = (uint64_t)Hs[1] + bb;
    T[L::OUT + 2] = (uint64_t)Hs[2] + c;
    T[L::OUT + 3] = (uint64_t)Hs[3] + d;
    T[L::OUT + 4] = E + Hs[4];
    T[L::OUT + 5] = (uint64_t)Hs[5] + f;
    T[L::OUT + 6] = (uint64_t)Hs[6] + g;
    T[L::OUT + 7] = (uint64_t)Hs[7] + h;
    T[L::ZERO] = 0;
  }
  __syncthreads();
  if (t < 64) {
    // round t's derived words from the stored sums: the working variable that is j rounds old at the start of round t is a_(t-j) (e_(t-j)), or, before
    // round 0, the chaining word H[j - t] (H[4 + j - t])
    const int i = (int)t;
    auto a_at = [&](int j) { return i >= j ? (uint32_t)T[L::ROUND + 9 * (i - j) + 4] : Hs[j - i]; };
    auto e_at = [&](int j) { return i >= j ? (uint32_t)T[L::ROUND + 9 * (i - j) + 0] : Hs[4 + j - i]; };
    const uint32_t a = a_at(0), bb = a_at(1), c = a_at(2), e = e_at(0), f = e_at(1), g = e_at(2);
    uint64_t* r = T + L::ROUND + 9 * i;
    const uint32_t s1a = sha_rotr(e, 6) ^ sha_rotr(e, 11), s0a = sha_rotr(a, 2) ^ sha_rotr(a, 13);
    r[1] = s1a;
    r[2] = s1a ^ sha_rotr(e, 25);
    r[3] = (e & f) ^ (~e & g);
    r[5] = s0a;
    r[6] = s0a ^ sha_rotr(a, 22);
    r[7] = bb & c;
    r[8] = (a & bb) ^ (a & c) ^ (bb & c);
  } else if (t < 64 + 48) {
    const int i = (int)t - 64 + 16;
    const uint32_t x = (uint32_t)T[L::W + i - 15], y = (uint32_t)T[L::W + i - 2];
    uint64_t* s = T + L::SCHED + 4 * (i - 16);
    const uint32_t s0a = sha_rotr(x, 7) ^ sha_rotr(x, 18), s1a = sha_rotr(y, 17) ^ sha_rotr(y, 19);
    s[0] = s0a;
    s[1] = s0a ^ (x >> 3);
    s[2] = s1a;
    s[3] = s1a ^ (y >> 10);
  }
  __syncthreads();

  // this workgroup's share of the block's variables: its preimage bits [p0, p1), then the compression's [c0, c1)
  const uint32_t p0 = min(n_pre, b * L::BITS_PER_BLOCK), p1 = min(n_pre, (b + 1) * L::BITS_PER_BLOCK), npre = p1 - p0;
  const uint32_t c0 = block_starts[b], c1 = block_starts[b + 1];
  const uint32_t n = npre + (c1 - c0);
  const uint32_t chunk = ((n + gridDim.y - 1) / gridDim.y + SHA_WIT_THREADS - 1) / SHA_WIT_THREADS * SHA_WIT_THREADS;
  const uint32_t lo = min(n, blockIdx.y * chunk), hi = min(n, lo + chunk);
  const uint32_t* T32 = (const uint32_t*)T;  // little-endian halves of the slots
  fe_t* out = tables[m] + off;
  const fe_t one = fe_one<S>();
  for (uint32_t k = lo + t; k < hi; k += SHA_WIT_THREADS) {
    const uint32_t v = k < npre ? p0 + k : c0 + (k - npre);
    const uint32_t dsc = desc[v];
    const uint32_t bit = (dsc >> L::DESC_BIT_SHIFT) & 63u;
    const uint32_t word = T32[2 * (dsc & L::DESC_SLOT_MASK) + (bit >> 5)];
    const uint32_t mask = 0u - (((word >> (bit & 31u)) ^ (dsc >> L::DESC_INVERT_SHIFT)) & 1u);
    fe_t el;
#pragma unroll
    for (int q = 0; q < 8; ++q) el.v[q] = one.v[q] & mask;
    out[v] = el;
  }
}

}  // namespace spk
