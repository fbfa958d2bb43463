// Witness plans for the SHA-256 circuits: witness generation without re-synthesising the circuit.
//
// The structure of sha256_spartan_circuit depends only on the message LENGTH (constant folding only ever sees the IV, the round constants and the
// padding) and the step circuit is the same for every block; every aux variable is a bit, and each of them is a fixed bit of a word that a native
// SHA-256 compression computes on the way (sha256_trace_layout.h). A plan is that correspondence, recorded once per structure by running the
// generator with a PlanRecorder attached (r1cs_builder.hpp): for every aux variable, in allocation order, a 32-bit descriptor
// (trace slot, bit, invert). The block a descriptor refers to is implied by the variable's position: the first n_pre variables are the preimage
// bits, 512 per block; the variables allocated by compression b are [block_starts[b], block_starts[b + 1]) (the last range also takes the step
// circuit's trailing x = 0).
//
// sha256_plan_eval is the plain C++ evaluation - native compressions -> trace -> bits - and the specification of the device kernel
// (csrc/kernels_witness.hpp k_sha256_witness), which does the same per (message, block) workgroup.
//
// Replaces, for these circuits, the witness synthesis inside the reference's prep_prove (src/bellpepper/r1cs.rs:359-409 precommitted_witness;
// src/neutronnova_zk.rs:1487-1518 for the steps).
#pragma once
#include <cstring>

#include "r1cs_builder.hpp"

namespace sp_frontend {

struct Sha256WitnessPlan {
  size_t msg_len = 0;    // bytes of a message this plan serves
  bool padded = true;    // true: sha256_spartan_circuit (the message is padded, n_blocks = padded length / 64); false: the step circuit (one raw 64-byte block)
  size_t n_aux = 0, n_pre = 0, n_blocks = 0;
  std::vector<uint32_t> desc;          // n_aux descriptors
  std::vector<uint32_t> block_starts;  // n_blocks + 1
};

inline void sha256_plan_check(Sha256WitnessPlan& P, PlanRecorder& rec, size_t n_aux) {
  namespace T = sha256_trace;
  P.n_aux = n_aux;
  P.n_blocks = rec.block_starts.size();
  P.desc = std::move(rec.desc);
  P.block_starts = std::move(rec.block_starts);
  P.block_starts.push_back((uint32_t)n_aux);
  if (P.desc.size() != n_aux) throw std::runtime_error("sha256 witness plan: a variable was allocated without a trace bit");
  for (uint32_t d : P.desc)
    if (d == T::DESC_UNSET || (d & T::DESC_SLOT_MASK) >= T::SLOTS) throw std::runtime_error("sha256 witness plan: a variable was allocated without a trace bit");
  if (P.n_blocks == 0 || P.block_starts[0] != P.n_pre || (P.n_pre + T::BITS_PER_BLOCK - 1) / T::BITS_PER_BLOCK > P.n_blocks)
    throw std::runtime_error("sha256 witness plan: unexpected allocation order");
  for (size_t b = 0; b < P.n_blocks; ++b)
    if (P.block_starts[b] > P.block_starts[b + 1]) throw std::runtime_error("sha256 witness plan: unexpected allocation order");
}

// the sha256_spartan_circuit layout for messages of msg_len >= 1 bytes (length 0 has no witness variable to place)
inline Sha256WitnessPlan sha256_witness_plan(size_t msg_len) {
  if (msg_len == 0) throw std::runtime_error("sha256 witness plan: the empty message has no preimage witness");
  Sha256WitnessPlan P;
  PlanRecorder rec;
  R1CSInstanceInt R = sha256_spartan_circuit(std::vector<uint8_t>(msg_len, 0), &rec);
  P.msg_len = msg_len;
  P.padded = true;
  P.n_pre = 8 * msg_len;
  sha256_plan_check(P, rec, R.witness.size());
  return P;
}

// the step / core circuit (sha256_step_circuit): 512 block bits, constant IV, one compression, x = 0
inline Sha256WitnessPlan sha256_step_witness_plan() {
  Sha256WitnessPlan P;
  PlanRecorder rec;
  const uint8_t zero[64] = {0};
  R1CSInstanceInt R = sha256_step_circuit(zero, &rec);
  P.msg_len = 64;
  P.padded = false;
  P.n_pre = 512;
  sha256_plan_check(P, rec, R.witness.size());
  return P;
}

// One block's trace from the chaining value it starts from and its 16 message words; Hout = the next chaining value.
inline void sha256_fill_trace(const uint32_t H[8], const uint32_t m[16], uint64_t* T, uint32_t Hout[8]) {
  namespace L = sha256_trace;
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  for (int i = 0; i < 16; ++i) T[L::W + i] = m[i];
  for (int i = 16; i < 64; ++i) {
    const uint32_t x = (uint32_t)T[L::W + i - 15], y = (uint32_t)T[L::W + i - 2];
    uint64_t* s = T + L::SCHED + 4 * (i - 16);
    s[0] = rotr(x, 7) ^ rotr(x, 18);
    s[1] = (uint32_t)s[0] ^ (x >> 3);
    s[2] = rotr(y, 17) ^ rotr(y, 19);
    s[3] = (uint32_t)s[2] ^ (y >> 10);
    T[L::W + i] = (uint64_t)(uint32_t)T[L::W + i - 16] + s[1] + (uint64_t)(uint32_t)T[L::W + i - 7] + s[3];
  }
  uint32_t b = H[1], c = H[2], d = H[3], f = H[5], g = H[6], h = H[7];
  uint64_t A = H[0], E = H[4];
  for (int i = 0; i < 64; ++i) {
    uint64_t* r = T + L::ROUND + 9 * i;
    const uint32_t e = (uint32_t)E, a = (uint32_t)A;
    r[0] = E;
    r[1] = rotr(e, 6) ^ rotr(e, 11);
    r[2] = (uint32_t)r[1] ^ rotr(e, 25);
    r[3] = (e & f) ^ (~e & g);
    r[4] = A;
    r[5] = rotr(a, 2) ^ rotr(a, 13);
    r[6] = (uint32_t)r[5] ^ rotr(a, 22);
    r[7] = b & c;
    r[8] = (a & b) ^ (a & c) ^ (b & c);
    const uint64_t temp1 = (uint64_t)h + r[2] + r[3] + SHA256_K[i] + (uint64_t)(uint32_t)T[L::W + i];
    E = (uint64_t)d + temp1;
    A = temp1 + r[6] + r[8];
    h = g, g = f, f = e, d = c, c = b, b = a;
  }
  T[L::OUT + 0] = A + H[0];
  T[L::OUT + 1] = (uint64_t)H[1] + b;
  T[L::OUT + 2] = (uint64_t)H[2] + c;
  T[L::OUT + 3] = (uint64_t)H[3] + d;
  T[L::OUT + 4] = E + H[4];
  T[L::OUT + 5] = (uint64_t)H[5] + f;
  T[L::OUT + 6] = (uint64_t)H[6] + g;
  T[L::OUT + 7] = (uint64_t)H[7] + h;
  T[L::ZERO] = 0;
  for (int j = 0; j < 8; ++j) Hout[j] = (uint32_t)T[L::OUT + j];
}

// the blocks a plan's message is hashed as: padded (FIPS 180-4 5.1.1) or the raw block
inline std::vector<uint8_t> sha256_plan_blocks(const Sha256WitnessPlan& P, const uint8_t* msg) {
  std::vector<uint8_t> m(msg, msg + P.msg_len);
  if (P.padded) {
    m.push_back(0x80);
    while ((m.size() + 8) % 64) m.push_back(0);
    const uint64_t bits = (uint64_t)P.msg_len * 8;
    for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(bits >> (8 * i)));
  }
  if (m.size() != 64 * P.n_blocks) throw std::runtime_error("sha256 witness plan: block count does not match the message length");
  return m;
}

// witness of the plan's circuit for `msg` (P.msg_len bytes): out[v] in {0, 1} for every aux variable v; digest_out (optional) = the last chaining value
inline void sha256_plan_eval(const Sha256WitnessPlan& P, const uint8_t* msg, uint64_t* out, uint32_t* digest_out = nullptr) {
  namespace L = sha256_trace;
  const std::vector<uint8_t> m = sha256_plan_blocks(P, msg);
  std::vector<uint64_t> T(L::SLOTS);
  uint32_t H[8];
  for (int i = 0; i < 8; ++i) H[i] = SHA256_IV[i];
  auto bit_of = [&T](uint32_t d) { return ((T[d & L::DESC_SLOT_MASK] >> ((d >> L::DESC_BIT_SHIFT) & 63u)) ^ (d >> L::DESC_INVERT_SHIFT)) & 1u; };
  for (size_t b = 0; b < P.n_blocks; ++b) {
    uint32_t w[16], Hn[8];
    for (int i = 0; i < 16; ++i) {
      const uint8_t* p = m.data() + 64 * b + 4 * i;
      w[i] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
    }
    sha256_fill_trace(H, w, T.data(), Hn);
    const size_t p0 = std::min(P.n_pre, b * L::BITS_PER_BLOCK), p1 = std::min(P.n_pre, (b + 1) * L::BITS_PER_BLOCK);
    for (size_t v = p0; v < p1; ++v) out[v] = bit_of(P.desc[v]);
    for (size_t v = P.block_starts[b]; v < P.block_starts[b + 1]; ++v) out[v] = bit_of(P.desc[v]);
    memcpy(H, Hn, sizeof H);
  }
  if (digest_out) memcpy(digest_out, H, sizeof H);
}

}  // namespace sp_frontend
