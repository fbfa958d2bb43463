// libspartan_hip.so - SHA-256 witness generation on the device (include/spartan_hip.h: sp_sha256_plan_*, sp_sha256_witness). The plan comes from the
// frontend (frontend/sha256_witness_plan.hpp); the kernel is kernels_witness.hpp. The host part here hashes the messages with the library's own
// SHA-256 to get the chaining value every block starts from: B dependent compressions are microseconds on the host.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "core.hpp"
#include "kernels_witness.hpp"
#include "sha256.hpp"

using sp::fail;

struct sp_sha256_plan {
  sp_ctx* ctx = nullptr;
  uint32_t* d_desc = nullptr;    // n_aux descriptors, then n_blocks + 1 block starts (one allocation)
  uint32_t* d_starts = nullptr;
  size_t n_aux = 0, n_blocks = 0, n_pre = 0, msg_len = 0;
  bool padded = true;
};

extern "C" {

int sp_sha256_plan_create(sp_ctx* c, const uint32_t* descriptors, size_t n_aux, const uint32_t* block_starts, size_t n_blocks, size_t n_pre, size_t msg_len, int padded,
                          sp_sha256_plan** out) {
  namespace L = sha256_trace;
  if (!c || !descriptors || !block_starts || !out) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_plan_create: null argument");
  if (n_aux == 0 || n_aux >= ((size_t)1 << 31) || n_blocks == 0 || n_blocks >= ((size_t)1 << 20) || msg_len == 0)
    return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_plan_create: empty or oversized plan");
  // the blocks the message is hashed as must be the plan's
  if (padded ? (msg_len + 9 + 63) / 64 != n_blocks : (msg_len != 64 || n_blocks != 1))
    return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_plan_create: block count does not match the message length");
  // everything the kernel indexes with is checked here, once: the preimage bits have a block each, the compressions' ranges are ordered and end at n_aux,
  // and every descriptor names a slot of the trace
  if (n_pre > n_aux || (n_pre + L::BITS_PER_BLOCK - 1) / L::BITS_PER_BLOCK > n_blocks || block_starts[0] < n_pre || block_starts[n_blocks] != n_aux)
    return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_plan_create: block offsets do not cover the variables");
  for (size_t b = 0; b < n_blocks; ++b)
    if (block_starts[b] > block_starts[b + 1]) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_plan_create: block offsets are not ascending");
  for (size_t v = 0; v < n_aux; ++v)
    if ((descriptors[v] & L::DESC_SLOT_MASK) >= L::SLOTS || (descriptors[v] >> (L::DESC_INVERT_SHIFT + 1)) != 0)
      return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_plan_create: a descriptor names no trace slot");
  SP_HIP(hipSetDevice(c->device));
  auto* p = new sp_sha256_plan();
  p->ctx = c;
  p->n_aux = n_aux, p->n_blocks = n_blocks, p->n_pre = n_pre, p->msg_len = msg_len, p->padded = padded != 0;
  const size_t words = n_aux + n_blocks + 1;
  hipError_t e = hipMalloc((void**)&p->d_desc, words * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(p->d_desc, descriptors, n_aux * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->d_desc + n_aux, block_starts, (n_blocks + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (p->d_desc) (void)hipFree(p->d_desc);
    delete p;
    return fail(SP_ERR_NO_DEVICE, std::string("sp_sha256_plan_create: ") + hipGetErrorString(e));
  }
  p->d_starts = p->d_desc + n_aux;
  *out = p;
  return SP_OK;
}

void sp_sha256_plan_free(sp_sha256_plan* p) {
  if (!p) return;
  if (p->d_desc) (void)hipFree(p->d_desc);
  delete p;
}

int sp_sha256_plan_info(const sp_sha256_plan* p, uint64_t out[5]) {
  if (!p || !out) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_plan_info: null argument");
  out[0] = p->n_aux, out[1] = p->n_blocks, out[2] = p->n_pre, out[3] = p->msg_len, out[4] = p->padded ? 1 : 0;
  return SP_OK;
}

int sp_sha256_witness(sp_ctx* c, const sp_sha256_plan* p, const uint8_t* msgs, size_t msg_len, size_t n_msgs, sp_table* const* tables, size_t off, uint8_t* digests) {
  if (!c || !p || !tables) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_witness: null argument");
  if (p->ctx != c) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_witness: the plan belongs to another context");
  if (msg_len != p->msg_len) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_witness: the plan serves another message length");
  if (n_msgs == 0) return SP_OK;
  if (!msgs) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_witness: null messages");
  if (n_msgs * p->n_blocks >= ((size_t)1 << 24)) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_witness: too many blocks for one launch");
  for (size_t m = 0; m < n_msgs; ++m) {
    const sp_table* t = tables[m];
    if (!t || off > t->cap || p->n_aux > t->cap - off) return fail(SP_ERR_INVALID_WITNESS_LENGTH, "sp_sha256_witness: the witness does not fit the table at this offset");
    for (size_t k = 0; k < m; ++k)
      if (tables[k] == t) return fail(SP_ERR_INVALID_INPUT_LENGTH, "sp_sha256_witness: one table given for two messages");
  }
  // staging: n_msgs table addresses, then per (message, block) the chaining value and the 16 message words
  const size_t nb = p->n_blocks, ptr_bytes = n_msgs * sizeof(fe_t*), words = n_msgs * nb * spk::SHA_WIT_BLOCK_WORDS;
  std::vector<uint64_t> stage((ptr_bytes + words * sizeof(uint32_t) + 7) / 8);
  fe_t** h_ptrs = (fe_t**)stage.data();
  uint32_t* h_words = (uint32_t*)((char*)stage.data() + ptr_bytes);
  std::vector<uint8_t> padded(64 * nb);
  for (size_t m = 0; m < n_msgs; ++m) {
    h_ptrs[m] = tables[m]->d;
    memset(padded.data(), 0, padded.size());
    memcpy(padded.data(), msgs + m * msg_len, msg_len);
    if (p->padded) {  // FIPS 180-4 5.1.1
      padded[msg_len] = 0x80;
      const uint64_t bits = (uint64_t)msg_len * 8;
      for (int i = 0; i < 8; ++i) padded[64 * nb - 1 - i] = (uint8_t)(bits >> (8 * i));
    }
    uint32_t H[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    for (size_t b = 0; b < nb; ++b) {
      uint32_t* w = h_words + (m * nb + b) * spk::SHA_WIT_BLOCK_WORDS;
      memcpy(w, H, sizeof H);
      for (int i = 0; i < 16; ++i) {
        uint32_t x;
        memcpy(&x, padded.data() + 64 * b + 4 * i, 4);
        w[8 + i] = __builtin_bswap32(x);
      }
      sp::Sha256::compress(H, padded.data() + 64 * b, 1);
    }
    if (digests)
      for (int i = 0; i < 8; ++i) {
        const uint32_t x = __builtin_bswap32(H[i]);
        memcpy(digests + 32 * m + 4 * i, &x, 4);
      }
  }
  const size_t bytes = stage.size() * 8;
  void* d_stage = c->workspace(sp_ctx::WS_SCALARS_RAW, bytes);
  if (!d_stage) return SP_ERR_NO_DEVICE;
  SP_HIP(hipMemcpyAsync(d_stage, stage.data(), bytes, hipMemcpyHostToDevice, c->stream));
  // enough workgroups to cover the device: the descriptors of a block are shared out over `splits` of them
  const size_t groups = n_msgs * nb;
  size_t splits = 1024 / groups;
  splits = splits < 1 ? 1 : (splits > 16 ? 16 : splits);
  c->timed_kernel("sha256_witness", (uint64_t)n_msgs * p->n_aux * (sizeof(fe_t) + sizeof(uint32_t)), spk::k_sha256_witness, dim3((unsigned)groups, (unsigned)splits),
                  dim3(spk::SHA_WIT_THREADS), (const uint32_t*)p->d_desc, (const uint32_t*)p->d_starts, (uint32_t)p->n_pre, (uint32_t)nb,
                  (const uint32_t*)((const char*)d_stage + ptr_bytes), (fe_t* const*)d_stage, off);
  SP_HIP(hipGetLastError());
  SP_HIP(sp::stream_sync(c->stream));  // the staging workspace is shared with the other upload entry points
  return SP_OK;
}

}  // extern "C"
