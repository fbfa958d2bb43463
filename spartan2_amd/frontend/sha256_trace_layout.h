// Per-block trace of one SHA-256 compression: the fixed list of 64-bit slots that a native compression fills on the way and that every witness
// bit of the SHA-256 circuits (r1cs_builder.hpp sha256_compression) is a bit of. Shared by the circuit generator (which notes, per allocated variable,
// the slot and bit it equals), the CPU evaluation of a witness plan (sha256_witness_plan.hpp) and the device kernel (csrc/kernels_witness.hpp).
// Constants only: no code lives here.
//
// With H[0..8) the chaining value the block starts from, m[0..16) its big-endian message words, lo(x) the low 32 bits of a slot, and
// a_i .. h_i the working variables at the START of round i (a_0 .. h_0 = H):
//   W + i            i < 16: m[i];  i >= 16: the full sum lo(W[i-16]) + s0 + lo(W[i-7]) + s1 (up to 34 bits), w[i] = lo(W[i])
//   SCHED + 4(i-16)  i in 16..63:  +0 rotr7(x) ^ rotr18(x)   +1 that ^ (x >> 3)  = s0,   x = w[i-15]
//                                  +2 rotr17(y) ^ rotr19(y)  +3 that ^ (y >> 10) = s1,   y = w[i-2]
//   ROUND + 9 i      i in 0..63:   +0 E_i: H[4] for i = 0, else the full sum d + h + S1 + ch + K + w of round i-1 (6 operands), e_i = lo(E_i)
//                                  +1 rotr6(e_i) ^ rotr11(e_i)   +2 that ^ rotr25(e_i) = S1   +3 ch(e_i, f_i, g_i)
//                                  +4 A_i: H[0] for i = 0, else the full sum h + S1 + ch + K + w + S0 + maj of round i-1 (7 operands), a_i = lo(A_i)
//                                  +5 rotr2(a_i) ^ rotr13(a_i)   +6 that ^ rotr22(a_i) = S0   +7 b_i & c_i   +8 maj(a_i, b_i, c_i)
//   OUT + j          j in 0..7:    the full sums of the final additions: OUT+0 = (round 63's sum for a) + H[0] (8 operands), OUT+4 = (round 63's
//                                  sum for e) + H[4] (7 operands), the others H[j] + the working variable; the next chaining value is lo(OUT + j)
//   ZERO             the constant 0 (the step circuit's x = 0)
//
// A descriptor names one bit of one slot, optionally inverted: slot | bit << 11 | invert << 17. The XOR gadget allocates the XOR of its operands'
// underlying variables, which is the logical value inverted when exactly one operand is a negated variable: that is what `invert` carries.
#pragma once
#include <stdint.h>

namespace sha256_trace {
constexpr uint32_t W = 0, SCHED = 64, ROUND = 256, OUT = 832, ZERO = 840, SLOTS = 841;
constexpr uint32_t DESC_BIT_SHIFT = 11, DESC_INVERT_SHIFT = 17, DESC_SLOT_MASK = (1u << DESC_BIT_SHIFT) - 1u, DESC_UNSET = 0xffffffffu;
constexpr uint32_t BITS_PER_BLOCK = 512;
constexpr uint32_t desc_pack(uint32_t slot, uint32_t bit, bool invert) { return slot | bit << DESC_BIT_SHIFT | (invert ? 1u : 0u) << DESC_INVERT_SHIFT; }
}  // namespace sha256_trace
