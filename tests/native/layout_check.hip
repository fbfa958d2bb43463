// Host-only check of spartan2_amd/host/proof_layout.hpp against proofs of the oracle (tests/test_proof_layout_cpu.py writes the case files):
// word count, wire length, bytes in both directions, the view's pointers against hand-written offsets, refusal of malformed bytes.
// A case file is uint64 values: kind (0 NeutronNova, 1 Spartan) | step dims (10) | core dims (10) | num_steps nb nx ny | vc_vars vc_cons vc_public |
// golden proof_words, wire_len (0 = none) | nwords nbytes | the words | the bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../spartan2_amd/host/proof_layout.hpp"

using namespace spartan2;

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("  FAILED line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

struct Count {
  size_t coords = 0, scalars_ = 0;
  void points(const aff_t*, size_t n) { coords += 2 * n; }
  void scalars(const fe_t*, size_t n) { scalars_ += n; }
};

static std::string refusal_text;
static int refusal(const NNLayout& L, const std::vector<uint8_t>& b) {  // the code from_bytes throws (its message in refusal_text), SP_OK when it accepts
  refusal_text.clear();
  try {
    L.from_bytes(b.data(), b.size());
  } catch (const Error& e) {
    refusal_text = e.what();
    return e.code;
  }
  return SP_OK;
}
static bool refused_as(const NNLayout& L, const std::vector<uint8_t>& b, const char* why) {
  return refusal(L, b) == SP_ERR_INVALID_INPUT_LENGTH && refusal_text.find(why) != std::string::npos;
}
// The Vec length at byte `at` is read with the bound `min_elem_bytes`: the largest count of such elements that the rest of the input could hold gets
// as far as the comparison with the key's shape, one more is refused by the bound itself, before anything is allocated or read. (This pins the
// bound to within the rounding of left / count: exactly where the prefix is far from the end, to a few bytes for the last sum-checks.)
static void check_bound(const NNLayout& L, const std::vector<uint8_t>& bytes, size_t at, size_t min_elem_bytes) {
  const uint64_t fits = (bytes.size() - at - 8) / min_elem_bytes;
  auto with = [&](uint64_t k) {
    std::vector<uint8_t> b = bytes;
    memcpy(&b[at], &k, 8);
    return b;
  };
  if (!refused_as(L, with(fits), "does not match the key's shape") || !refused_as(L, with(fits + 1), "length prefix exceeds the input")) {
    printf("  FAILED: the length prefix at byte %zu is not read with the bound %zu\n", at, min_elem_bytes);
    ++failures;
  }
}

static void check_nn(const sp_dims& ds, const sp_dims& dc, const uint64_t* h, const std::vector<uint64_t>& words, const std::vector<uint8_t>& bytes) {
  const size_t n = h[0], nb = h[1], nx = h[2], ny = h[3], vc_vars = h[4], vc_cons = h[5], vc_public = h[6], gold_words = h[7], gold_len = h[8];
  const vcirc::Shape vs = vcirc::Shape::from_circuit(vcirc::Circuit(nb, nx, ny, 32));
  CHECK(vs.total_vars == vc_vars && vs.num_cons == vc_cons && vs.num_public == vc_public);
  const NNLayout L(ds, dc, n, vs);
  CHECK(L.words() == words.size());
  CHECK(L.wire_len() == bytes.size());
  if (gold_words) CHECK(L.words() == gold_words && L.wire_len() == gold_len);
  if (L.words() != words.size()) return;
  CHECK(L.to_bytes(words.data(), words.size()) == bytes);
  CHECK(refusal(L, bytes) == SP_OK && L.from_bytes(bytes.data(), bytes.size()) == words);
  try {
    L.to_bytes(words.data(), words.size() - 4);
    CHECK(!"to_bytes took a short proof");
  } catch (const Error& e) {
    CHECK(e.code == SP_ERR_INVALID_INPUT_LENGTH);
  }
  // the view against offsets written out by hand (field elements; rows of the 2048-wide key from the equalized dimensions)
  const size_t rows_sh = ds.num_shared_unpadded ? ds.num_shared / 2048 : 0, rows_rest_of_step = (ds.num_shared + ds.num_precommitted + ds.num_rest) / 2048 - ds.num_shared / 2048;
  CHECK(L.rows_sh == rows_sh && L.rows_pre + L.rows_rest == rows_rest_of_step && L.rows_pre_c + L.rows_rest_c == rows_rest_of_step);
  const size_t vio = nb + nx + 1 + ny + vc_public, vlx = log2_ceil(vc_cons), vly = log2_ceil(next_pow2(vc_vars)) + 1;
  const fe_t* w = reinterpret_cast<const fe_t*>(words.data());
  const fe_t* end = w + words.size() / 4;
  const NNProofView v = L.view(words.data());
  CHECK(reinterpret_cast<const fe_t*>(v.delta) == w + 2 * rows_sh + n * (2 * rows_rest_of_step + ds.num_public) + 2 * rows_rest_of_step + dc.num_public);
  CHECK(v.blind_vE == end - 1);
  CHECK(v.rnd_u == end - (2 * 32 + 2) - 2 * vly - 3 - 3 * vlx - vio - 1 && v.rnd_X == v.rnd_u + 1);
  CHECK(v.steps.size() == n && v.vcomm.size() == vs.num_rounds && v.vchal.size() == vs.num_rounds);
  CHECK(reinterpret_cast<const fe_t*>(v.comm_shared) == w && reinterpret_cast<const fe_t*>(v.core.pre) + 2 * rows_rest_of_step == v.core.pub);
  Count c;
  L.visit(words.data(), c);
  size_t vrows_all = 0;
  for (size_t r = 0; r < vs.num_rounds; ++r) vrows_all += vs.vars_padded[r] / 32;
  const size_t vcons_rows = vc_cons / 32;
  // points: the shared rows, every instance's other rows, delta and beta, the verifier circuit's comm_w_per_round, comm_T, random_U.comm_W and comm_E
  CHECK(c.coords == 2 * (rows_sh + (n + 1) * rows_rest_of_step + 2 + vrows_all + vcons_rows + vrows_all + vcons_rows));
  CHECK(c.coords + c.scalars_ == words.size() / 4);
  CHECK(well_formed(L, words.data()));
  std::vector<uint64_t> bad_words = words;
  bad_words.back() = ~0ull;  // blind_vE >= the modulus
  CHECK(!well_formed(L, bad_words.data()));
  // malformed bytes
  std::vector<uint8_t> b(bytes.begin(), bytes.end() - 1);
  CHECK(refusal(L, b) == SP_ERR_INVALID_INPUT_LENGTH);  // one byte cut
  b = bytes;
  b.push_back(0);
  CHECK(refusal(L, b) == SP_ERR_INVALID_INPUT_LENGTH);  // one trailing byte
  b = bytes;
  b[0] ^= 1;
  CHECK(refusal(L, b) == SP_ERR_INVALID_INPUT_LENGTH);  // the first Option tag (comm_W_shared) flipped
  b = bytes;
  b[1] += 1;  // the first length prefix follows that tag: the shared commitment's rows, or the number of step instances
  CHECK(refusal(L, b) == SP_ERR_INVALID_INPUT_LENGTH);
  b = bytes;
  for (int i = 0; i < 8; ++i) b[1 + i] = i == 7 ? 0x10 : 0;  // 2^60
  CHECK(refused_as(L, b, "length prefix exceeds the input"));
  // the bound each kind of Vec is read with, at byte positions written out by hand from both ends of the image
  auto option_bytes = [](size_t r) { return 1 + (r ? 8 + 96 * r : 0); };
  auto instance_bytes = [&](size_t pre, size_t rest, size_t npub) { return 1 + option_bytes(pre) + 8 + 96 * rest + 8 + 32 * npub + 8; };
  const size_t steps_at = option_bytes(rows_sh);
  const size_t vrounds_at = steps_at + 8 + n * instance_bytes(L.rows_pre, L.rows_rest, ds.num_public) + instance_bytes(L.rows_pre_c, L.rows_rest_c, dc.num_public) +
                            2 * 96 + 8 + 32 * 2048 + 2 * 32;
  const size_t v_E_at = bytes.size() - 32 - 32 * 32 - 8, inner_at = bytes.size() - 2 * (8 + 32 * 32 + 32) - vly * (8 + 32 * 2) - 8;
  const size_t outer_at = inner_at - 3 * 32 - vlx * (8 + 32 * 3) - 8, comm_E_at = outer_at - 32 - (8 + 32 * vio) - 96 * vcons_rows - 8;
  if (rows_sh) check_bound(L, bytes, 1, 96);   // comm_W_shared: points
  check_bound(L, bytes, steps_at, 1 + 1 + 8 + 8 + 8);  // step_instances: two Option tags and three Vec lengths at least
  check_bound(L, bytes, vrounds_at, 8);        // comm_w_per_round: a Vec length at least
  check_bound(L, bytes, comm_E_at, 96);        // random_U.comm_E: points
  check_bound(L, bytes, outer_at, 8 + 32 * 3); // the outer sum-check: three coefficients and their length
  check_bound(L, bytes, inner_at, 8 + 32 * 2); // the inner sum-check: two
  check_bound(L, bytes, v_E_at, 32);           // eval_E: scalars
  // step and core rows that do not add up to the same number are refused at construction
  sp_dims odd = dc;
  odd.num_rest += 2048;
  try {
    NNLayout l2(ds, odd, n, vs);
    CHECK(!"a core with one more row was taken");
  } catch (const Error& e) {
    CHECK(e.code == SP_ERR_INTERNAL);
  }
}

static void check_spartan(const sp_dims& d, const std::vector<uint64_t>& words, const std::vector<uint8_t>& bytes) {
  const SpartanLayout L(d, d.num_shared + d.num_precommitted + d.num_rest);
  CHECK(L.words() == words.size());
  if (L.words() != words.size()) return;
  const sp_spartan_layout wl = L.wire();
  size_t len = 0;
  CHECK(sp_proof_serialize(&wl, words.data(), words.size(), nullptr, 0, &len) == SP_OK && len == bytes.size());
  std::vector<uint8_t> out(len);
  CHECK(sp_proof_serialize(&wl, words.data(), words.size(), out.data(), out.size(), &len) == SP_OK && out == bytes);
  sp_spartan_layout got;
  size_t nw = 0;
  CHECK(sp_proof_deserialize(bytes.data(), bytes.size(), &got, nullptr, 0, &nw) == SP_OK && nw == words.size() && memcmp(&got, &wl, sizeof got) == 0);
  const fe_t* w = reinterpret_cast<const fe_t*>(words.data());
  const fe_t* end = w + words.size() / 4;
  const size_t rows = (d.num_shared + d.num_precommitted + d.num_rest + 2047) / 2048, M = d.num_shared + d.num_precommitted + d.num_rest;
  const SpartanProofView v = L.view(words.data());
  CHECK(L.rows() == rows);
  CHECK(v.publics == w + 2 * rows && v.z_beta == end - 1 && v.z_vec == end - 2 - (M < 2048 ? M : 2048));
  CHECK(reinterpret_cast<const fe_t*>(v.delta) == v.z_vec - 4 && v.blind_eval_W == v.z_vec - 5);
  Count c;
  L.visit(words.data(), c);
  CHECK(c.coords == 2 * rows + 4 && c.coords + c.scalars_ == words.size() / 4);
  CHECK(well_formed(L, words.data()));
  std::vector<uint64_t> bad_words = words;
  bad_words[3] = ~0ull;  // x of the first commitment row >= the modulus
  CHECK(!well_formed(L, bad_words.data()));
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      printf("%s: cannot open\n", argv[a]);
      return 2;
    }
    uint64_t h[32];
    sp_dims ds, dc;
    static_assert(sizeof(sp_dims) == 80, "sp_dims is ten 64-bit values");
    bool ok = fread(h, 8, 1, f) == 1 && fread(&ds, sizeof ds, 1, f) == 1 && fread(&dc, sizeof dc, 1, f) == 1 && fread(h + 1, 8, 11, f) == 11;
    std::vector<uint64_t> words(ok ? h[10] : 0);
    std::vector<uint8_t> bytes(ok ? h[11] : 0);
    ok = ok && fread(words.data(), 8, words.size(), f) == words.size() && fread(bytes.data(), 1, bytes.size(), f) == bytes.size();
    fclose(f);
    if (!ok) {
      printf("%s: short case file\n", argv[a]);
      return 2;
    }
    const int before = failures;
    try {
      if (h[0] == 0)
        check_nn(ds, dc, h + 1, words, bytes);
      else
        check_spartan(ds, words, bytes);
    } catch (const std::exception& e) {
      printf("  FAILED: %s\n", e.what());
      ++failures;
    }
    printf("%s: %d mismatches\n", argv[a], failures - before);
  }
  return failures ? 1 : 0;
}
