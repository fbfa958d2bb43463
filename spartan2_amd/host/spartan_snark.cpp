// Host side ABOVE the C ABI: the protocol driver of the reference restated in C++ and calling ONLY the entry points of
// include/spartan_hip.h for everything that scales with the instance — exactly what the reference's Rust drivers would do
// through an `extern "C"` block. Mirrors
//   SplitR1CSShape::new            src/r1cs/mod.rs:810-911      (padding / column remap)
//   SpartanSNARK::setup            src/spartan.rs:146-173
//   SpartanSNARK::prep_prove       src/spartan.rs:176-216       (+ bellpepper/r1cs.rs:359-409 precommitted_witness)
//   SpartanSNARK::prove            src/spartan.rs:219-466       (+ bellpepper/r1cs.rs:411-538, hyrax_pc.rs:387-478, ipa.rs:125-170)
//   SpartanSNARK::verify           src/spartan.rs:469-578       (matrix evaluations and opening MSMs on the device)
// for circuits without verifier challenges: any mix of shared / precommitted / rest variables (bench circuits: precommitted-only,
// skip_synthesize + commit_zeros path :443; the reference's e2e CubicCircuit src/spartan.rs:587-651: rest-only).
//
// Randomness is injected: every blind / mask is the next 64-byte block of a caller-supplied tape reduced with from_uniform,
// in the reference's call order.
// Generators: this build's own derivation (the reference's is a third-party hash-to-curve): PARITY UNPINNED, see DESIGN.md.
#include <future>
#include <memory>

#include "proof_layout.hpp"

namespace spartan2 {

// ---- keys / state ----------------------------------------------------------------------------------------------------------
struct SpartanProverKey {  // src/spartan.rs:30-58
  sp_ctx* ctx = nullptr;
  sp_shape* S = nullptr;
  sp_ck *ck = nullptr, *ck_s = nullptr;
  sp_dims dims;
  SpartanLayout layout;  // of a proof under this key (proof_layout.hpp)
  size_t num_vars = 0, num_extra = 0, num_cols = 0;
  uint8_t vk_digest[32];
  std::vector<aff_t> gens, gens_s;
  // a SpartanVerifierKey loaded from its bytes (verifier_from_bytes): S holds the row-major structures alone. verify, verify_batch and the byte forms
  // read nothing else of a key; the C surface refuses such a key at every prover entry point ("verifier-only key")
  bool verifier_only = false;
  // a key loaded from its bytes, a verifier's or a prover's (prover_from_bytes): vk_to_bytes and pk_to_bytes refuse it - the caller holds the bytes
  bool from_bytes = false;
  // verify()'s device workspaces (T_x, T_y, the three products M T_y): allocated by the first verify on this key and kept - five hipMalloc / hipFree
  // pairs of 32-64 MB were half of a 3.3 ms verify. One verify at a time per key (as for every handle of the ABI).
  mutable sp_table *v_Tx = nullptr, *v_Ty = nullptr, *v_mv[3] = {nullptr, nullptr, nullptr};
  mutable std::vector<sp_table*> vb_Tx, vb_Ty;  // verify_batch()'s (T_x, T_y) pairs of one chunk, kept like the above
  ~SpartanProverKey() {
    for (sp_table* t : vb_Tx) sp_table_free(t);
    for (sp_table* t : vb_Ty) sp_table_free(t);
    sp_table_free(v_Tx);
    sp_table_free(v_Ty);
    for (sp_table* t : v_mv) sp_table_free(t);
    sp_shape_free(S);
    sp_ck_free(ck);
    sp_ck_free(ck_s);
  }
};

// How a helper thread waits for its owner. It sleeps on a condition variable that the owner notifies at each state change: measured at config 2, a
// lone prove is as fast this way as with a spinning helper (1.29-1.31 ms either way; wake-up ~10 us, off the critical path or under the MSM it
// starts), and a spinning helper costs one CPU per prove in flight on top of the owner's polling thread - under the 16-CPU CFS quota of the bench
// boxes eight such pairs got the whole cgroup throttled and resident kernels ran into their watchdog.
// A helper that waits INSIDE a prove for the owner's next notification (the opening's helper: delta once the outer sum-check is in its resident rounds,
// comm_LZ once the row challenges are drawn) may spin while few proves are in flight in the process: a sleeping thread's wake-up is the scheduler's
// to time - usually tens of microseconds, now and then milliseconds (one prove in 50 - 2000 was 2 - 5 ms long for it on the bench boxes). With many
// proves in flight (the 8-context throughput mode under a 16-CPU quota) the helpers sleep: a CPU per helper is then worth more than the odd late one.
// delta's MSM (ipa.rs:147; ~175 us of bucket kernels on the auxiliary stream) is issued by the opening's helper when the outer sum-check has this many
// rounds left (SPARTAN_DELTA_ROUNDS_LEFT, A/B): late enough to stay clear of the streaming rounds, early enough to be done before poly_ABC starts
static size_t delta_rounds_before_end() {
  static const size_t v = [] {
    const char* e = getenv("SPARTAN_DELTA_ROUNDS_LEFT");
    const int k = e ? atoi(e) : 17;
    return (size_t)(k < 1 ? 1 : k);
  }();
  return v;
}
static std::atomic<int> g_active_proves{0};
static constexpr int HELPER_SPIN_MAX_PROVES = 4;
static bool helper_may_spin() { return g_active_proves.load(std::memory_order_relaxed) <= HELPER_SPIN_MAX_PROVES; }
struct ActiveProve {
  ActiveProve() { g_active_proves.fetch_add(1, std::memory_order_relaxed); }
  ~ActiveProve() { g_active_proves.fetch_sub(1, std::memory_order_relaxed); }
};

// Per-prep-state driver options (ss_prep_set_flags; defaults from the environment at prep_prove time).
//   FLAG_PREFIX_CACHE: the transcript prefix new + vk + public_values + comm_W_shared / comm_W_precommitted is the same for every prove on one prep
//     state; with this flag its sponge state is computed once and cloned (Keccak256Transcript is Clone, keccak.rs:25) — an API-level optimisation
//     the reference does not make (it re-hashes the prefix in every prove, src/spartan.rs:226-236, r1cs.rs:422-427). Default OFF: the prefix is
//     re-hashed inside every prove (on a helper thread, under commit_zeros), so the timed region does the reference's work.
//   FLAG_LZ_DIRECT: the opening in the reference's own order (bind W with L, then the MSM over the key) instead of the MSM over the row commitments.
//   FLAG_REFERENCE_ORDER: prove_reference_order below — ONE thread, no helper jobs, only include/spartan_hip.h entry points (the one prep-time product it uses
//     is the FixedBaseMul table set of the committed rows, handed to sp_hyrax_prove_announce_tables), called
//     in the order of the statements of src/spartan.rs:226-466 (what an unchanged spartan.rs bound to the ABI does). bench.py reports it beside the headline.
enum : unsigned { FLAG_PREFIX_CACHE = 1u, FLAG_LZ_DIRECT = 2u, FLAG_REFERENCE_ORDER = 4u };

struct SpartanPrepSNARK {  // src/spartan.rs:107-124
  sp_table *W = nullptr, *caz = nullptr, *cbz = nullptr, *ccz = nullptr;      // witness + cached partial products
  sp_table *az = nullptr, *bz = nullptr, *cz = nullptr, *z = nullptr;          // scratch reused across prove calls
  sp_table *rx = nullptr, *abc = nullptr;
  sp_table *p0 = nullptr, *p1 = nullptr;  // per-pair products of the outer sum-check's first round (sp_multiply_vec_incremental_round0)
  sp_table* sat_z = nullptr;              // is_sat's own z = [W | 1 | X]: allocated by the first check on the state; no prove reads or writes it
  std::vector<aff_t> comm_W_fixed;  // rows committed at prep time: shared rows, then precommitted rows
  std::vector<fe_t> r_W_fixed;      // their blinds, same order
  size_t rows_shared = 0, rows_precommitted = 0;
  std::vector<uint8_t> comm_shared_bytes, comm_pre_bytes;  // transcript encodings (hyrax_pc.rs:714-729)
  bool is_small = true;
  const struct SpartanProverKey* key = nullptr;  // the key prep_prove made this state for (prove_batch refuses states of another key)
  sp_transcript* tr_prefix = nullptr;  // FLAG_PREFIX_CACHE: transcript state after the per-instance prefix (see prove)
  std::vector<fe_t> tr_publics;
  sp_transcript* tr_fresh = nullptr;   // default: the prefix re-hashed for this prove by the second helper
  Background bg2;
  unsigned flags = 0;
  Background bg;                        // hashes comm_W for the PCS transcript step while the sum-checks run, then starts comm_LZ's MSM
  sp_absorb_state* poly_com = nullptr;  // its result
  sp_points* comm_pts = nullptr;        // comm_W on the device: the bases of comm_LZ's MSM
  // FixedBaseMul tables of the rows committed here (shared, precommitted) and of h (msm.rs:653-689): with no rest variables the remaining rows of
  // comm_W are h * blind (commit_zeros), so comm_LZ = sum_fixed L_i comm_W[i] + (sum_rest L_i blind_i) h is one multi_mul over these tables
  // (sp_fbtables_multi_mul: 14 levels of additions in one launch instead of a 512-point MSM behind the last row challenge).
  // Up to 512 rows (2^20 variables): measured at 1024 / 2048 rows the walk (a 17-level chain over 256 / 512 blocks) loses to the MSM it would replace
  // (1.77 vs 1.70 ms, 2.58 vs 2.51 ms): there the sum-check's last rounds no longer cover it and its blocks compete with the streaming rounds.
  sp_fbtables* lz_tables = nullptr;
  std::vector<aff_t> lz_points;  // their bases (the committed rows, then h) while the build is still to be queued
  int lz_mode = 0;               // 1: queue the build behind the first prove on this state (prep_prove, SPARTAN_PREP_TABLES)
  void queue_lz_tables(sp_ctx* ctx) {  // end of a prove
    if (lz_mode != 1 || lz_tables || lz_points.empty()) return;
    lz_mode = 0;
    if (sp_fbtables_create_async(ctx, u64p(&lz_points[0].x), lz_points.size(), &lz_tables) != SP_OK) lz_tables = nullptr;  // (the MSM over the rows stays)
  }
  // host wall-clock of prep_prove's phases, ms (ss_prep_phases): witness (u64 -> elements on the device), commit (PCS::commit of the shared and
  // precommitted rows), tables (FixedBaseMul tables of the committed rows), matvec (multiply_vec_precommitted), scratch (allocations), total
  double prep_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  ~SpartanPrepSNARK() {
    sp_fbtables_free(lz_tables);
    bg.wait_nothrow();
    bg2.wait_nothrow();
    sp_transcript_free(tr_fresh);
    sp_points_free(comm_pts);
    sp_absorb_state_free(poly_com);
    sp_transcript_free(tr_prefix);
    for (sp_table* t : {W, caz, cbz, ccz, az, bz, cz, z, rx, abc, p0, p1, sat_z}) sp_table_free(t);
  }
};

struct PhaseTimes {
  double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // witness_commit, matvec, outer, poly_abc, inner, pcs, total, (spare)
  std::vector<std::pair<std::string, double>> laps;  // fine-grained host-side laps (diagnostics)
};

// SpartanSNARK::setup (src/spartan.rs:146-173)
SpartanProverKey* setup(sp_ctx* ctx, const R1CSIntView& R) {
  auto* pk = new SpartanProverKey();
  try {
    pk->ctx = ctx;
    PaddedShape P = pad_shape(R);
    pk->dims = P.dims;
    pk->num_vars = P.num_vars();
    pk->layout = SpartanLayout(P.dims, pk->num_vars);
    pk->num_extra = 1 + P.dims.num_public + P.dims.num_challenges;
    pk->num_cols = P.num_cols();
    sp_csr cs[3];
    for (int m = 0; m < 3; ++m) cs[m] = sp_csr{u64p(P.data[m].data()), P.idx[m].data(), P.ptr[m].data()};
    ck(sp_shape_from_csr(ctx, &cs[0], &cs[1], &cs[2], &P.dims, &pk->S), "shape_from_csr");
    pk->gens = from_label("ck", DEFAULT_COMMITMENT_WIDTH + 1);  // commitment_key (src/r1cs/mod.rs:1031-1043) -> PCS::setup(b"ck", ., 2048)
    pk->gens_s = from_label("ck_s", 2);                          // PCS::setup(b"ck_s", 1, 1)
    ck(sp_ck_create(ctx, u64p(&pk->gens[0].x), DEFAULT_COMMITMENT_WIDTH, u64p(&pk->gens[DEFAULT_COMMITMENT_WIDTH].x), &pk->ck), "ck_create");
    ck(sp_ck_create(ctx, u64p(&pk->gens_s[0].x), 1, u64p(&pk->gens_s[1].x), &pk->ck_s), "ck_s_create");
    spartan_vk_digest(P, pk->gens, pk->gens_s, pk->vk_digest);
  } catch (...) {
    delete pk;
    throw;
  }
  return pk;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- SpartanVerifierKey { vk_ee, ck_s, S } (src/spartan.rs:62-70) to and from its bincode bytes -----------------------------------------------------------
// Writing: setup keeps neither the circuit nor the padded CSR (its time and memory stay what they were), so the caller hands the circuit again; the stream is
// sp_wire_hyrax_key(ck), sp_wire_hyrax_key(ck_s), sp_wire_shape(.., 0) over the re-padded circuit, and it is returned only if it hashes to the key's digest -
// another circuit than the one the key was set up from is refused.
std::vector<uint8_t> vk_to_bytes(const SpartanProverKey& pk, const R1CSIntView& R) {
  if (pk.verifier_only) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "vk_to_bytes: verifier-only key (it was loaded from its bytes: keep those)");
  if (pk.from_bytes) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "vk_to_bytes: a key loaded from its bytes (keep those)");
  PaddedShape P = pad_shape(R);
  sp_csr cs[3];
  padded_csr(P, cs);
  sp_wire* w = nullptr;
  ck(sp_wire_new(0, &w), "wire_new");
  std::unique_ptr<sp_wire, void (*)(sp_wire*)> guard(w, sp_wire_free);
  ck(sp_wire_hyrax_key(w, u64p(&pk.gens[0].x), pk.gens.size() - 1, u64p(&pk.gens.back().x)), "wire vk_ee");
  ck(sp_wire_hyrax_key(w, u64p(&pk.gens_s[0].x), pk.gens_s.size() - 1, u64p(&pk.gens_s.back().x)), "wire ck_s");
  ck(sp_wire_shape(w, &P.dims, &cs[0], &cs[1], &cs[2], 0), "wire S");
  std::vector<uint8_t> out(sp_wire_len(w));
  ck(sp_wire_bytes(w, out.data(), out.size()), "wire_bytes");
  uint8_t dig[32];
  ck(sp_vk_digest_from_wire(out.data(), out.size(), dig), "vk digest of the written bytes");
  if (memcmp(dig, pk.vk_digest, 32) != 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "vk_to_bytes: the circuit is not the one this key was set up from (digest mismatch)");
  return out;
}
// the length of that stream from the circuit's sizes alone (the sizing pass of the two-pass protocol)
size_t vk_bytes_len(const SpartanProverKey& pk, const R1CSIntView& R) {
  const size_t rows = next_pow2(R.num_cons);
  size_t n = (8 + 8 + 64 * (pk.gens.size() - 1) + 96) + (8 + 8 + 64 * (pk.gens_s.size() - 1) + 96) + 80;
  for (int m = 0; m < 3; ++m) n += 8 + 40 * (size_t)R.m[m].indptr[R.num_cons] + 8 + 8 + 8 * (rows + 1) + 8;
  return n;
}

// Reading: the two Hyrax keys (sp_unwire_hyrax_key), the shape (sp_shape_from_wire: row-only, decode form by `flags` = SP_SHAPE_WIRE_*), no trailing bytes,
// the ten dimensions those SplitR1CSShape::new gives a circuit of the unpadded sizes; the digest is hashed from the bytes on a helper thread under the
// device work. The key is a SpartanProverKey marked verifier_only: what verify and verify_batch read of a key, and nothing else.
// host wall-clock of the calling thread's last verifier_from_bytes, ms (ss_verifier_stages): the two Hyrax keys read, sp_shape_from_wire, the two
// sp_ck_create, the digest on its helper thread, the wait for it behind everything else, the whole call
static thread_local double g_vk_stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
// ... and of its last prover_from_bytes (ss_prover_stages): the same six, then 1 / 0 = the shape was built on the device / the host, 1 / 0 = the digest was
// hashed / trusted
static thread_local double g_pk_stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
// which form of the full shape a prover load without a forcing flag takes: measured (profiles/prover_key.md), by the rule of profiles/verifier_key.md -
// the device form only if its median lies below the host form's minimum
static constexpr bool PK_FULL_DEVICE_DEFAULT = true;
enum : unsigned { SS_PK_TRUST_DIGEST = 1u << 16 };  // (outside the SP_SHAPE_WIRE_* range)

// One loader behind both keys. A verifier's (prover == false): the bytes are SpartanVerifierKey, the shape row-only, the digest hashed from them. A
// prover's: SpartanProverKey { ck, ck_s, S, vk_digest } (src/spartan.rs:42-49) - for Hyrax ck serialises as vk_ee does, so the stream is the verifier's
// bytes followed by the 32 raw digest bytes (bincode writes [u8; 32] without a length); the shape is the FULL shape, and the stored digest is compared with
// the hash of the bytes before it unless SS_PK_TRUST_DIGEST takes it as the reference's Deserialize does.
static SpartanProverKey* key_from_bytes(sp_ctx* ctx, const uint8_t* bytes, size_t n, unsigned flags, bool prover) {
  const std::string who_s = prover ? "prover_from_bytes" : "verifier_from_bytes";
  const char* const who = who_s.c_str();
  double* const stage_ms = prover ? g_pk_stage_ms : g_vk_stage_ms;
  for (int i = 0; i < 8; ++i) stage_ms[i] = 0;
  const double t_start = now_ms();
  if (!ctx || !bytes || n == 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, who_s + ": null context, null bytes or no bytes");
  bool trust_digest = false;
  if (!prover) {
    if (flags & SP_SHAPE_WIRE_FULL) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "verifier_from_bytes: a verifier's key holds the row-only shape");
  } else {
    trust_digest = flags & SS_PK_TRUST_DIGEST;
    flags &= ~(unsigned)SS_PK_TRUST_DIGEST;
    if (flags & (SP_SHAPE_WIRE_DEVICE | SP_SHAPE_WIRE_HOST)) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prover_from_bytes: a prover's key holds the full shape (SP_SHAPE_WIRE_FULL_DEVICE or SP_SHAPE_WIRE_FULL)");
    if (!(flags & (SP_SHAPE_WIRE_FULL_DEVICE | SP_SHAPE_WIRE_FULL))) flags |= PK_FULL_DEVICE_DEFAULT ? SP_SHAPE_WIRE_FULL_DEVICE : SP_SHAPE_WIRE_FULL;
    if (n <= 32) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prover_from_bytes: unexpected end of input (no room for the 32 digest bytes)");
    n -= 32;  // the key's bytes; the stored digest lies behind them
  }
  const uint8_t* const stored_digest = bytes + n;
  auto pk = std::make_unique<SpartanProverKey>();
  pk->ctx = ctx;
  pk->verifier_only = !prover;
  pk->from_bytes = true;
  ck(sp_ctx_bind_thread(ctx), "device");
  sp_unwire* r = nullptr;
  ck(sp_unwire_new(bytes, n, &r), "unwire_new");
  std::unique_ptr<sp_unwire, void (*)(sp_unwire*)> guard(r, sp_unwire_free);
  auto read_key = [&](std::vector<aff_t>& gens, size_t want_cols, const char* what) {
    size_t nc = 0;
    ck(sp_unwire_hyrax_key(r, nullptr, 0, &nc, nullptr), what);
    if (nc != want_cols) throw Error(SP_ERR_INVALID_INPUT_LENGTH, std::string(what) + ": num_cols is " + std::to_string(nc) + ", this build's is " + std::to_string(want_cols));
    gens.resize(nc + 1);
    ck(sp_unwire_hyrax_key(r, u64p(&gens[0].x), nc, &nc, u64p(&gens[nc].x)), what);
  };
  read_key(pk->gens, DEFAULT_COMMITMENT_WIDTH, prover ? "prover_from_bytes: ck" : "verifier_from_bytes: vk_ee");
  read_key(pk->gens_s, 1, prover ? "prover_from_bytes: ck_s" : "verifier_from_bytes: ck_s");
  const double t_keys = now_ms();
  // the digest needs the bytes alone
  double digest_ms = 0;
  std::future<int> digest = std::async(trust_digest ? std::launch::deferred : std::launch::async, [&] {
    if (trust_digest) {
      memcpy(pk->vk_digest, stored_digest, 32);
      return (int)SP_OK;
    }
    const double t0 = now_ms();
    const int rc = sp_vk_digest_from_wire(bytes, n, pk->vk_digest);
    digest_ms = now_ms() - t0;
    return rc;
  });
  struct Join {
    std::future<int>& f;
    ~Join() {
      if (f.valid()) f.wait();
    }
  } join{digest};
  ck(sp_shape_from_wire(ctx, r, flags, &pk->dims, &pk->S), "shape_from_wire");
  ck(sp_unwire_done(r), who);
  const double t_shape = now_ms();
  const sp_dims& d = pk->dims;
  const sp_dims want = padded_dims(d.num_cons_unpadded, d.num_shared_unpadded, d.num_precommitted_unpadded, d.num_rest_unpadded, d.num_public, d.num_challenges);
  if (memcmp(&want, &d, sizeof d) != 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, who_s + ": the ten dimensions are not those SplitR1CSShape::new gives the unpadded sizes");
  pk->num_vars = d.num_shared + d.num_precommitted + d.num_rest;
  pk->layout = SpartanLayout(d, pk->num_vars);
  pk->num_extra = 1 + d.num_public + d.num_challenges;
  pk->num_cols = pk->num_vars + pk->num_extra;
  ck(sp_ck_create(ctx, u64p(&pk->gens[0].x), DEFAULT_COMMITMENT_WIDTH, u64p(&pk->gens[DEFAULT_COMMITMENT_WIDTH].x), &pk->ck), "ck_create");
  ck(sp_ck_create(ctx, u64p(&pk->gens_s[0].x), 1, u64p(&pk->gens_s[1].x), &pk->ck_s), "ck_s_create");
  const double t_ck = now_ms();
  const int drc = digest.get();
  if (drc != SP_OK) throw Error(drc, who_s + ": the digest pass could not walk the bytes");
  if (prover && memcmp(pk->vk_digest, stored_digest, 32) != 0)
    throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prover_from_bytes: vk_digest: the stored digest is not the digest of the key's bytes (a prover under it makes proofs no verifier accepts)");
  const double t_end = now_ms();
  const double st[6] = {t_keys - t_start, t_shape - t_keys, t_ck - t_shape, digest_ms, t_end - t_ck, t_end - t_start};
  std::copy(st, st + 6, stage_ms);
  if (prover) stage_ms[6] = (flags & SP_SHAPE_WIRE_FULL_DEVICE) ? 1 : 0, stage_ms[7] = trust_digest ? 0 : 1;
  return pk.release();
}
SpartanProverKey* verifier_from_bytes(sp_ctx* ctx, const uint8_t* bytes, size_t n, unsigned flags) {
  return key_from_bytes(ctx, bytes, n, flags, false);
}
// A prover's key from the bytes pk_to_bytes writes: flags = SP_SHAPE_WIRE_FULL_DEVICE / SP_SHAPE_WIRE_FULL to force the form of the shape's decode (neither:
// PK_FULL_DEVICE_DEFAULT), SP_SHAPE_WIRE_TIMED, SS_PK_TRUST_DIGEST. The key is an ordinary SpartanProverKey (verifier_only == false).
SpartanProverKey* prover_from_bytes(sp_ctx* ctx, const uint8_t* bytes, size_t n, unsigned flags) {
  return key_from_bytes(ctx, bytes, n, flags, true);
}
// SpartanProverKey { ck, ck_s, S, vk_digest } as bincode: the verifier's bytes (vk_ee and ck serialise alike for Hyrax), then the digest
std::vector<uint8_t> pk_to_bytes(const SpartanProverKey& pk, const R1CSIntView& R) {
  if (pk.from_bytes) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "pk_to_bytes: a key loaded from its bytes (keep those)");
  std::vector<uint8_t> out = vk_to_bytes(pk, R);
  out.insert(out.end(), pk.vk_digest, pk.vk_digest + 32);
  return out;
}

// ---- SpartanSNARK::prep_prove (src/spartan.rs:176-216) for `count` states of one key in one pass -------------------------------------------------------
// ONE driver behind every witness source and every count. `fill_W` writes the witness segments into the zeroed tables W[0 .. count) (each segment at its
// padded offset): machine words from the frontend (prep_prove, prep_prove_batch) or the SHA-256 witness kernel (prep_prove_sha256, prep_prove_sha256_batch:
// one launch for all messages). Everything after it is the reference's prep_prove restated phase by phase over the batch: the blinds (from tape k, shared
// first), the commitments (sp_hyrax_commit_batch per segment: one launch, one copy, one wait and one normalisation for all states), the tables block, the
// cached products (one sp_multiply_vec per state, queued back to back; sp_multiply_vec_chunked - one walk over A, B, C per chunk of vectors - on request: it
// was measured and does not win, see the constants below), the scratch, one synchronise. State k is word for word the state a batch of one makes of
// witness k with tape k: group sums as canonical affine points and exact field sums, so neither depends on how the work was grouped. Still per state:
// the allocations and the lz_tables block (the tables are built lazily, behind a state's first prove).
// A batch of one takes the per-state calls: there is nothing to share. That is prep_prove and prep_prove_sha256: `who` = "prep_prove" names the single
// entry points, whose errors pass as they are and whose SPARTAN_PREP_TRACE line starts "prep_prove:"; any other `who` ("prep_prove_batch") prefixes an
// error with itself and the state at fault and traces as "prep_prove_batch(count):" - at count 1 as well.
// flags: SS_PREP_PER_STATE_COMMIT keeps one sp_hyrax_commit per state and segment, SS_PREP_PER_STATE_MATVEC one sp_multiply_vec per state,
// SS_PREP_CHUNKED_MATVEC takes sp_multiply_vec_chunked (same states; there so that one process can compare the paths; with both product flags set
// SS_PREP_PER_STATE_MATVEC wins).
// What the driver takes by default was measured (profiles/prep_prove_batch.md, config 2, one process, legs alternating):
//   commit: sp_hyrax_commit_batch beats one sp_hyrax_commit per state at every K >= 2 measured (1.15 against 2.37 ms at K = 4, 4.42 against 9.46 at
//     K = 16): PREP_BATCH_COMMIT_MIN = 2, there is no K at which the loop wins.
//   cached product: sp_multiply_vec_chunked does NOT beat one sp_multiply_vec per state at any K measured (k_spmv3_multi 0.093 ms a vector against
//     0.083 for k_spmv3<true>; the whole call 1.01 x at K = 4, 1.02 x at K = 16, inside the spread): PREP_CHUNKED_MATVEC_DEFAULT = false, the driver
//     takes the loop and the shared walk runs only when SS_PREP_CHUNKED_MATVEC asks for it.
enum : unsigned { SS_PREP_PER_STATE_COMMIT = 1, SS_PREP_PER_STATE_MATVEC = 2, SS_PREP_CHUNKED_MATVEC = 4 };
static constexpr size_t PREP_BATCH_COMMIT_MIN = 2;
static constexpr bool PREP_CHUNKED_MATVEC_DEFAULT = false;
static std::vector<SpartanPrepSNARK*> prep_prove_batch_from(const SpartanProverKey& pk, size_t count, bool is_small, Tape* tapes, unsigned flags,
                                                            const std::function<void(sp_table* const* W)>& fill_W, double* phase_ms, const char* who) {
  const sp_dims& d = pk.dims;
  const bool single = !strcmp(who, "prep_prove");
  std::vector<std::unique_ptr<SpartanPrepSNARK>> st(count);
  size_t at = (size_t)-1;  // the state a per-state step is working on (names the state in an error)
  try {
    sp_ctx* ctx = pk.ctx;
    const size_t M = pk.num_vars, N = d.num_cons;
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double t_begin = now_ms();
    double t_last = t_begin;
    auto phase = [&](int k) {
      const double t = now_ms();
      ms[k] += t - t_last;
      t_last = t;
    };
    // the environment, read here and nowhere else in prep
    const auto is = [](const char* e, char c) { return e && e[0] == c; };
    const unsigned state_flags = (is(getenv("SPARTAN_LZ_DIRECT"), '1') ? FLAG_LZ_DIRECT : 0u) | (is(getenv("SPARTAN_PREFIX_CACHE"), '1') ? FLAG_PREFIX_CACHE : 0u);
    // WHEN the FixedBaseMul tables of the committed rows are built (SPARTAN_PREP_TABLES): the build is ~3 ms of device work (profiles/r06_prep_prove.md) that
    // pays for itself from the second prove on a state onwards (50-100 us a prove) and slows whatever proves beside it. "lazy" (default): queued behind the
    // FIRST prove on the state - a state that is proven once (the reference's own use: prep_prove, prove, drop) never pays, the bench's repeated proves get
    // them from the third on; "prep": queued here; "sync": built here and waited for (round 5); "off": never.
    const char* tables_mode = getenv("SPARTAN_PREP_TABLES");
    const bool trace = getenv("SPARTAN_PREP_TRACE") != nullptr;
    const bool round0_products = !is(getenv("SPARTAN_ROUND0_PRODUCTS"), '0');  // "0": round 1 of the outer sum-check evaluates straight from Az, Bz, Cz (A/B)
    // 1. witness: shared_witness / precommitted_witness (bellpepper/r1cs.rs:306-409), each segment at its padded offset. The rest segment is filled here as
    // well: without verifier challenges it does not change between proves. Machine words go to the device as they are (8 bytes a value) and become
    // Montgomery-form elements there: sp_table_write_u64 (the reference hands the same words to msm_small, hyrax_pc.rs:266-292, and never builds wide
    // scalars for the commitment either).
    std::vector<sp_table*> Ws(count);
    for (at = 0; at < count; ++at) {
      st[at].reset(new SpartanPrepSNARK());
      SpartanPrepSNARK* ps = st[at].get();
      ps->bg.set_spin_policy(&helper_may_spin);
      ps->bg2.set_spin_policy(&helper_may_spin);
      ps->is_small = is_small;
      ps->key = &pk;
      ps->flags = state_flags;
      ck(sp_table_zeros(ctx, M, (size_t)-1, (size_t)-1, &ps->W), "alloc W");
      Ws[at] = ps->W;
    }
    at = (size_t)-1;
    fill_W(Ws.data());
    phase(0);
    // 2. blinds: PCS::blind (hyrax_pc.rs:192-205) from tape k, shared first
    const size_t CW = DEFAULT_COMMITMENT_WIDTH;
    const size_t rows_shared = d.num_shared_unpadded ? (d.num_shared + CW - 1) / CW : 0;
    const size_t rows_pre = d.num_precommitted_unpadded ? (d.num_precommitted + CW - 1) / CW : 0;
    for (at = 0; at < count; ++at) {
      SpartanPrepSNARK* ps = st[at].get();
      ps->rows_shared = rows_shared;
      ps->rows_precommitted = rows_pre;
      ps->r_W_fixed.resize(rows_shared + rows_pre);
      for (auto& b : ps->r_W_fixed) b = tapes[at].next();
      ps->comm_W_fixed.resize(ps->r_W_fixed.size());
    }
    at = (size_t)-1;
    // 3. commit: the shared segment of every state, then the precommitted one
    const bool batch_commit = !(flags & SS_PREP_PER_STATE_COMMIT) && count >= PREP_BATCH_COMMIT_MIN;
    for (int seg = 0; seg < 2; ++seg) {
      const size_t rows = seg == 0 ? rows_shared : rows_pre, first = seg == 0 ? 0 : rows_shared;
      const size_t off = seg == 0 ? 0 : d.num_shared, n = seg == 0 ? d.num_shared : d.num_precommitted;
      if (!rows) continue;
      if (batch_commit) {
        std::vector<const uint64_t*> bl(count);
        std::vector<uint64_t*> out(count);
        for (size_t k = 0; k < count; ++k) {
          bl[k] = u64p(st[k]->r_W_fixed.data() + first);
          out[k] = u64p(&st[k]->comm_W_fixed[first].x);
        }
        ck(sp_hyrax_commit_batch(ctx, pk.ck, count, Ws.data(), off, n, bl.data(), out.data()), seg == 0 ? "commit shared" : "commit precommitted");
      } else {
        for (at = 0; at < count; ++at)
          ck(sp_hyrax_commit(ctx, pk.ck, Ws[at], off, n, u64p(st[at]->r_W_fixed.data() + first), is_small ? 1 : 0, u64p(&st[at]->comm_W_fixed[first].x)),
             seg == 0 ? "commit shared" : "commit precommitted");
        at = (size_t)-1;
      }
      for (size_t k = 0; k < count; ++k)
        (seg == 0 ? st[k]->comm_shared_bytes : st[k]->comm_pre_bytes) = commitment_bytes(st[k]->comm_W_fixed.data() + first, rows);
    }
    phase(1);
    // 4. tables of the committed rows and h (SpartanPrepSNARK::lz_tables)
    for (at = 0; at < count; ++at) {
      SpartanPrepSNARK* ps = st[at].get();
      const size_t fixed = ps->comm_W_fixed.size(), rows_all = (M + CW - 1) / CW;
      if (!(ps->flags & FLAG_LZ_DIRECT) && d.num_rest_unpadded == 0 && d.num_challenges == 0 && fixed >= 1 && fixed + 1 <= 512 && rows_all > 1) {
        const char* mode = tables_mode;
        ps->lz_points.assign(ps->comm_W_fixed.begin(), ps->comm_W_fixed.end());
        ps->lz_points.push_back(pk.gens[CW]);  // h
        ps->lz_mode = !mode || !strcmp(mode, "lazy") ? 1 : (!strcmp(mode, "off") ? 0 : 2);
        if (mode && !strcmp(mode, "sync")) ck(sp_fbtables_create(ctx, u64p(&ps->lz_points[0].x), ps->lz_points.size(), &ps->lz_tables), "tables of the committed rows");
        else if (ps->lz_mode == 2) ck(sp_fbtables_create_async(ctx, u64p(&ps->lz_points[0].x), ps->lz_points.size(), &ps->lz_tables), "tables of the committed rows");
      }
    }
    phase(2);
    // 5. multiply_vec_precommitted (src/r1cs/mod.rs:1112-1128) for every state: z_k = [W_k cached | 0 ...]
    for (at = 0; at < count; ++at) {
      SpartanPrepSNARK* ps = st[at].get();
      ck(sp_table_zeros(ctx, 2 * M, (size_t)-1, (size_t)-1, &ps->z), "alloc z");
      ck(sp_table_copy(ctx, ps->z, 0, ps->W, 0, d.num_shared + d.num_precommitted), "copy W");
      ck(sp_table_set_len(ps->z, pk.num_cols, (size_t)-1, (size_t)-1), "z len");
      for (sp_table** t : {&ps->caz, &ps->cbz, &ps->ccz, &ps->az, &ps->bz, &ps->cz}) ck(sp_table_zeros(ctx, N, (size_t)-1, (size_t)-1, t), "alloc Az");
    }
    if (!(flags & SS_PREP_PER_STATE_MATVEC) && (PREP_CHUNKED_MATVEC_DEFAULT || (flags & SS_PREP_CHUNKED_MATVEC)) && count >= 2) {
      at = (size_t)-1;
      std::vector<const sp_table*> zs(count);
      std::vector<sp_table*> az(count), bz(count), cz(count);
      for (size_t k = 0; k < count; ++k) zs[k] = st[k]->z, az[k] = st[k]->caz, bz[k] = st[k]->cbz, cz[k] = st[k]->ccz;
      ck(sp_multiply_vec_chunked(ctx, pk.S, zs.data(), count, az.data(), bz.data(), cz.data()), "multiply_vec_precommitted");
    } else {
      for (at = 0; at < count; ++at) ck(sp_multiply_vec(ctx, pk.S, st[at]->z, st[at]->caz, st[at]->cbz, st[at]->ccz), "multiply_vec_precommitted");
    }
    at = (size_t)-1;
    if (trace) ck(sp_ctx_synchronize(ctx), "sync");
    phase(3);
    // 6. scratch
    for (at = 0; at < count; ++at) {
      SpartanPrepSNARK* ps = st[at].get();
      ck(sp_table_zeros(ctx, N, (size_t)-1, (size_t)-1, &ps->rx), "alloc rx");
      if (N >= 2 && round0_products) {
        ck(sp_table_zeros(ctx, N / 2, (size_t)-1, (size_t)-1, &ps->p0), "alloc round-0 products");
        ck(sp_table_zeros(ctx, N / 2, (size_t)-1, (size_t)-1, &ps->p1), "alloc round-0 products");
      }
      ck(sp_table_zeros(ctx, 2 * M, (size_t)-1, (size_t)-1, &ps->abc), "alloc poly_ABC");
    }
    at = (size_t)-1;
    ck(sp_ctx_synchronize(ctx), "sync");
    phase(4);
    ms[6] = now_ms() - t_begin;
    for (size_t k = 0; k < count; ++k)
      for (int i = 0; i < 8; ++i) st[k]->prep_ms[i] = ms[i] / (double)count;
    if (phase_ms) memcpy(phase_ms, ms, sizeof ms);
    if (trace) {
      const std::string name = single ? std::string(who) : std::string(who) + "(" + std::to_string(count) + ")";
      fprintf(stderr, "%s: witness %.3f commit %.3f tables %.3f matvec %.3f scratch %.3f total %.3f ms\n", name.c_str(), ms[0], ms[1], ms[2], ms[3], ms[4], ms[6]);
    }
  } catch (const Error& e) {
    // every state made so far goes with `st`
    if (single) throw;
    throw Error(e.code, std::string(who) + ": " + (at == (size_t)-1 ? std::string() : "state " + std::to_string(at) + ": ") + e.what());
  }
  std::vector<SpartanPrepSNARK*> out(count);
  for (size_t k = 0; k < count; ++k) out[k] = st[k].release();
  return out;
}

// the witness words of `count` states from the frontend: witnesses_u64[k] = shared | precommitted | rest, unpadded
static void upload_witnesses(const SpartanProverKey& pk, sp_table* const* W, const uint64_t* const* witnesses_u64, size_t count) {
  const sp_dims& d = pk.dims;
  for (size_t k = 0; k < count; ++k) {
    auto put = [&](size_t dst, size_t src, size_t cnt) { ck(sp_table_write_u64(pk.ctx, W[k], dst, witnesses_u64[k] + src, cnt), "upload W"); };
    put(0, 0, d.num_shared_unpadded);
    put(d.num_shared, d.num_shared_unpadded, d.num_precommitted_unpadded);
    // (with verifier challenges the rest segment is synthesized inside every prove, after the challenges are drawn: bellpepper/r1cs.rs:443-461)
    if (d.num_challenges == 0) put(d.num_shared + d.num_precommitted, d.num_shared_unpadded + d.num_precommitted_unpadded, d.num_rest_unpadded);
  }
}

SpartanPrepSNARK* prep_prove(const SpartanProverKey& pk, const uint64_t* witness_u64, size_t n_witness, bool is_small, Tape& tape) {
  const sp_dims& d = pk.dims;
  if (n_witness != d.num_shared_unpadded + d.num_precommitted_unpadded + d.num_rest_unpadded) throw Error(SP_ERR_INVALID_WITNESS_LENGTH, "InvalidWitnessLength");
  return prep_prove_batch_from(pk, 1, is_small, &tape, 0, [&](sp_table* const* W) { upload_witnesses(pk, W, &witness_u64, 1); }, nullptr, "prep_prove")[0];
}

// prep_prove for Sha256Circuit (benches/sha256_spartan.rs:78-136) with the witness generated on the device: the reference's prep_prove INCLUDES witness
// synthesis (src/spartan.rs:176-216 -> precommitted_witness, bellpepper/r1cs.rs:359-409); here it is sp_sha256_witness on a plan made once per key.
// The key is a sha256_spartan_circuit key (everything precommitted, 256 public digest bits) for the plan's message length; one key serves every message
// of that length. out_publics: the 256 digest bits in the order the circuit allocates them (big-endian bit order), from the host's SHA-256.
SpartanPrepSNARK* prep_prove_sha256(const SpartanProverKey& pk, const sp_sha256_plan* plan, const uint8_t* msg, size_t len, bool is_small, Tape& tape, uint64_t out_publics[256]) {
  const sp_dims& d = pk.dims;
  uint64_t info[5];
  ck(sp_sha256_plan_info(plan, info), "plan info");
  if (d.num_shared_unpadded != 0 || d.num_rest_unpadded != 0 || d.num_challenges != 0 || info[0] != d.num_precommitted_unpadded)
    throw Error(SP_ERR_INVALID_WITNESS_LENGTH, "InvalidWitnessLength: the plan's variable count is not the key's");
  if (len != info[3] || !info[4] || d.num_public != 256) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "the plan does not serve this message length / this key is not a SHA-256 digest circuit");
  sp_ctx* ctx = pk.ctx;
  uint8_t digest[32];
  SpartanPrepSNARK* ps = prep_prove_batch_from(pk, 1, is_small, &tape, 0, [&](sp_table* const* W) {
    ck(sp_sha256_witness(ctx, plan, msg, len, 1, W, d.num_shared, digest), "sha256 witness");
  }, nullptr, "prep_prove")[0];
  for (int i = 0; i < 256; ++i) out_publics[i] = (digest[i / 8] >> (7 - i % 8)) & 1u;
  return ps;
}

std::vector<SpartanPrepSNARK*> prep_prove_batch(const SpartanProverKey& pk, const uint64_t* const* witnesses_u64, size_t n_witness, size_t count, bool is_small, Tape* tapes,
                                                unsigned flags, double* phase_ms) {
  const sp_dims& d = pk.dims;
  for (size_t k = 0; k < count; ++k) {
    if (!witnesses_u64[k] && n_witness) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: state " + std::to_string(k) + ": null witness");
  }
  if (n_witness != d.num_shared_unpadded + d.num_precommitted_unpadded + d.num_rest_unpadded)
    throw Error(SP_ERR_INVALID_WITNESS_LENGTH, "prep_prove_batch: state 0: InvalidWitnessLength");
  return prep_prove_batch_from(pk, count, is_small, tapes, flags, [&](sp_table* const* W) { upload_witnesses(pk, W, witnesses_u64, count); }, phase_ms, "prep_prove_batch");
}

std::vector<SpartanPrepSNARK*> prep_prove_sha256_batch(const SpartanProverKey& pk, const sp_sha256_plan* plan, const uint8_t* msgs, size_t len, size_t count, bool is_small,
                                                       Tape* tapes, uint64_t* out_publics, unsigned flags, double* phase_ms) {
  const sp_dims& d = pk.dims;
  uint64_t info[5];
  ck(sp_sha256_plan_info(plan, info), "prep_prove_batch: plan info");
  if (d.num_shared_unpadded != 0 || d.num_rest_unpadded != 0 || d.num_challenges != 0 || info[0] != d.num_precommitted_unpadded)
    throw Error(SP_ERR_INVALID_WITNESS_LENGTH, "prep_prove_batch: InvalidWitnessLength: the plan's variable count is not the key's");
  if (len != info[3] || !info[4] || d.num_public != 256)
    throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: the plan does not serve this message length / this key is not a SHA-256 digest circuit");
  sp_ctx* ctx = pk.ctx;
  std::vector<uint8_t> digests(32 * count);
  std::vector<SpartanPrepSNARK*> out = prep_prove_batch_from(pk, count, is_small, tapes, flags, [&](sp_table* const* W) {
    ck(sp_sha256_witness(ctx, plan, msgs, len, count, W, d.num_shared, digests.data()), "sha256 witness");
  }, phase_ms, "prep_prove_batch");
  for (size_t k = 0; k < count; ++k)
    for (int i = 0; i < 256; ++i) out_publics[256 * k + i] = (digests[32 * k + i / 8] >> (7 - i % 8)) & 1u;
  return out;
}


// ---- prove's helper jobs ---------------------------------------------------------------------------------------------------------------------------
// What prove() hands to the two helper threads of its prep state (SpartanPrepSNARK::bg, bg2), as types of their own: each holds what its job reads and
// writes, run() is the job. prove() constructs them on its stack, submits [&job] { job.run(); } and joins through the guards below on every exit path.

// the transcript up to the rest commitment, as a state to adopt or clone (absorb_instance_prefix)
static sp_transcript* instance_prefix(sp_ctx* ctx, const SpartanProverKey& pk, const SpartanPrepSNARK& ps, const fe_t* publics, size_t npub) {
  Tr t0(ctx, "SpartanSNARK");
  absorb_instance_prefix(t0, pk.vk_digest, publics, npub, ps.comm_shared_bytes, ps.comm_pre_bytes);
  sp_transcript* t = t0.t;
  t0.t = nullptr;
  return t;
}

// ONE job for the second helper, submitted before anything else, carries the host chains nothing on the proving thread depends on until much later:
//   (1) the transcript prefix (src/spartan.rs:226-236, bellpepper/r1cs.rs:422-427): new + vk + public_values + comm_W_shared + comm_W_precommitted -
//       about 300 Keccak blocks at config 2, ~45 us. Re-hashed in every prove, as the reference does (FLAG_PREFIX_CACHE keeps the sponge state
//       across proves instead). Needed when comm_W_rest is absorbed, i.e. after commit_zeros has come back from the device: `prefix_ready`.
//   (2) the IPA mask d_vec (ipa.rs:139-145) and the blinds of delta and beta, which do not depend on the transcript: 2048 wide reductions from their
//       tape position, ~70 us. Needed when delta's MSM is issued (a third of the way into the outer sum-check): `dvec_ready`.
//   (3) the blind's term of comm_eval_W (src/spartan.rs:423-437): blind_eval_W is the next block of the tape, h_s * blind a host walk of 32 additions
//       that otherwise stands between the inner sum-check's last round and the opening's transcript; with it h_s * r_beta, the blind's term of
//       beta = <R, d> g_s + r_beta h_s (ipa.rs:148-149): `eval_W_term_ready`.
// The first helper stays free for the opening's job, which is posted the moment comm_W is complete.
struct PrefixJob {
  sp_ctx* ctx;
  SpartanPrepSNARK* ps;
  const SpartanProverKey* pk;
  const fe_t* publics;
  size_t npub;
  bool prefix_cached;
  Tape peek;  // at d_vec: behind the rest-row blinds (drawn by then) and blind_eval_W (then d_vec, r_delta, r_beta)
  fe_t* dvec;
  size_t n_ipa;
  fe_t blind_eval_W;  // peeked from its block of the tape
  // what the job delivers
  fe_t r_delta, r_beta, eval_W_term_blind;
  aff_t eval_W_term, beta_term;  // h_s * blind_eval_W, h_s * r_beta (valid once eval_W_term_ready is set)
  std::atomic<int> prefix_ready{0}, dvec_ready{0}, eval_W_term_ready{0};
  void run() {
    struct Flags {  // whatever happens in here, a waiter must not spin for ever (an exception resurfaces at the next wait())
      std::atomic<int>*a, *b;
      ~Flags() {
        a->store(1, std::memory_order_release);
        b->store(1, std::memory_order_release);
      }
    } flags{&prefix_ready, &dvec_ready};
    if (!prefix_cached) {
      sp_transcript_free(ps->tr_fresh);
      ps->tr_fresh = nullptr;
      ps->tr_fresh = instance_prefix(ctx, *pk, *ps, publics, npub);
    }
    prefix_ready.store(1, std::memory_order_release);
    for (size_t i = 0; i < n_ipa; ++i) dvec[i] = peek.next();
    r_delta = peek.next();  // ipa.rs:146: the blind of delta follows d_vec on the tape
    r_beta = peek.next();   // then beta's
    dvec_ready.store(1, std::memory_order_release);
    // (both blind terms of the opening's one-value commitments: comm_eval_W above and beta = <R, d> g_s + r_beta h_s, ipa.rs:148-149)
    aff_t two[2];
    const fe_t bl[2] = {blind_eval_W, r_beta};
    if (sp_fixed_base_mul_h(ctx, pk->ck_s, u64p(bl), 2, u64p(&two[0].x)) == SP_OK) {
      eval_W_term = two[0];
      eval_W_term_blind = blind_eval_W;
      beta_term = two[1];
      eval_W_term_ready.store(1, std::memory_order_release);
    }
  }
};
struct PrefixJoin {  // publics must outlive the job on every exit path
  Background& b;
  ~PrefixJoin() { b.wait_nothrow(); }
};

// The first helper's job, posted the moment comm_W is complete: comm_W's transcript encoding (64 B per row, Montgomery -> canonical) and the Keccak blocks
// of absorb("poly_com", ..), the first absorb after the inner sum-check's last squeeze (hyrax_pc.rs:387-400). With `ahead` the same job then issues
// delta's MSM and computes comm_LZ = sum_i L[i] comm_W[i] (= commit(L . W; <L, r_W>), hyrax_pc.rs:430-455, by the homomorphism of the commitment) as
// soon as the inner sum-check has bound the row variables: the MSM runs under the remaining rounds instead of after them.
struct LzAhead {
  std::atomic<int> state{0};  // 0: row challenges not drawn yet, 1: drawn, 2: abandoned
  std::atomic<int> rows_known{0};  // how many of them r[] holds so far (the helper expands eq(r, .) a level per challenge, as they arrive)
  size_t nvr = 0;
  fe_t r[24];
  sp_msm_job* job = nullptr;
  sp_vec_job* vec = nullptr;
  fe_t r_LZ;
  std::atomic<int> delta_state{0};  // 0: delta's MSM not issued yet, 1: issued, 2: abandoned
  sp_msm_job* delta_job = nullptr;
  fe_t r_delta;
  aff_t delta;
  bool delta_done = false;
  std::atomic<int> early_done{0};  // poly_com prepared and delta finished: what the PCS phase needs first (1 = done, 2 = gave up)
  aff_t comm_LZ;                   // the tables path (SpartanPrepSNARK::lz_tables): the helper delivers comm_LZ itself
  bool have_comm_LZ = false;
  // a helper that may not spin sleeps on this pair; the owner notifies after each state change (a notify without a sleeper is a user-space check)
  std::mutex mu;
  std::condition_variable cv;
  void publish(std::atomic<int>& flag, int v) {
    flag.store(v, std::memory_order_release);
    cv.notify_one();
  }
  // what the job reads: comm_W and its blinds, the key, the tables of the fixed rows + h (non-null: usable, every other row of comm_W is h * blind,
  // commit_zeros), d_vec and r_delta as the second helper's job delivers them (*dvr set)
  sp_ctx* ctx = nullptr;
  const aff_t* rows = nullptr;
  size_t nrows = 0;
  SpartanPrepSNARK* psp = nullptr;
  const fe_t* blinds = nullptr;
  bool ahead = false;  // false: the job ends with poly_com
  const sp_ck* key = nullptr;
  size_t cols = 0;
  const sp_fbtables* tabs = nullptr;
  size_t nfixed = 0;
  const fe_t* dv = nullptr;
  size_t dn = 0;
  const std::atomic<int>* dvr = nullptr;
  const fe_t* rda = nullptr;
  void run() {
    const std::vector<uint8_t> b = commitment_bytes(rows, nrows);
    ck(sp_transcript_preabsorb((const uint8_t*)"poly_com", 8, b.data(), b.size(), &psp->poly_com), "poly_com (prepare)");
    if (!ahead) return;
    ck(sp_ctx_bind_thread(ctx), "helper thread: device");  // a new thread starts on device 0; the context may live on another GPU
    ck(sp_points_upload(ctx, u64p(&rows[0].x), nrows, &psp->comm_pts), "comm_W (upload)");
    const auto t0 = std::chrono::steady_clock::now();
    // sleeps until the owner publishes the state (helper_may_spin above)
    auto wait_for = [&](std::atomic<int>& flag) {
      int st;
      while ((st = flag.load(std::memory_order_acquire)) == 0) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) return 2;  // the prover never got there
        if (!helper_may_spin()) {
          std::unique_lock<std::mutex> lk(mu);  // woken by publish(); the timeout covers a notify that raced the predicate
          cv.wait_for(lk, std::chrono::microseconds(100), [&] { return flag.load(std::memory_order_acquire) != 0; });
        } else {
          sp_relax();
        }
      }
      return st;
    };
    // delta (ipa.rs:147): issued from here once the outer sum-check has left its streaming rounds (the owner publishes delta_state from its
    // challenge observer): the MSM then runs under the resident tail kernel, which leaves the device idle, instead of beside the first rounds
    // of the inner sum-check (measured there: k_eval_quad_stream_lowhi 32 us against 18 us alone, profiles/r04_kernel_stats.md)
    if (wait_for(delta_state) != 1) return;
    while (dvr->load(std::memory_order_acquire) == 0) sp_relax();  // d_vec, r_delta (the second helper's job, posted first thing in the prove: long done)
    r_delta = *rda;
    ck(sp_msm_ck_begin(ctx, key, u64p(dv), dn, &delta_job), "delta (begin)");
    {
      sp_msm_job* j = delta_job;
      delta_job = nullptr;  // finish() consumes the job whatever it returns
      ck(sp_msm_ck_finish(ctx, key, j, u64p(&r_delta), u64p(&delta.x)), "delta (finish)");
    }
    delta_done = true;
    early_done.store(1, std::memory_order_release);
    if (tabs && nvr >= 1 && nrows == ((size_t)1 << nvr)) {
      // comm_LZ = sum_{fixed rows} L_i comm_W[i] + (sum_{zero rows} L_i blind_i) h, L = eq(r_rows, .): one multi_mul over the prepared tables. Its ~100 us
      // of dependent point additions are the critical path of the opening, so everything in front of the launch is kept off the last row challenge:
      // eq(r, .) is expanded a level per challenge as the inner sum-check draws them (the observer counts them in rows_known), and what the last
      // challenge r leaves to do is the last level (2^(nvr-1) products) and h's scalar, (1 - r) S0 + r S1 with S_c = sum over the zero rows of parity c
      // of P[i >> 1] blind_i taken one level up; <L, r_W> for z_delta follows the launch. (All of it at once behind the last challenge was ~40 us.)
      std::vector<fe_t> P(1, fe_one<S>());
      for (size_t known = 0; known + 1 < nvr; ++known) {
        const auto w0 = std::chrono::steady_clock::now();
        while ((size_t)rows_known.load(std::memory_order_acquire) <= known) {
          if (state.load(std::memory_order_acquire) == 2 || std::chrono::steady_clock::now() - w0 > std::chrono::seconds(20)) return;
          if (!helper_may_spin()) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait_for(lk, std::chrono::microseconds(50), [&] { return (size_t)rows_known.load(std::memory_order_acquire) > known; });
          } else {
            sp_relax();
          }
        }
        const fe_t rk = r[known];
        std::vector<fe_t> Q(2 * P.size());
        for (size_t i = 0; i < P.size(); ++i) {  // the new variable is the index LSB (eq.rs:66-76)
          const fe_t hi = fe_mul<S>(P[i], rk);
          Q[2 * i + 1] = hi;
          Q[2 * i] = fe_sub<S>(P[i], hi);
        }
        P.swap(Q);
      }
      fe_t S0 = fe_zero(), S1 = fe_zero();
      for (size_t i = nfixed; i < nrows; ++i) {
        const fe_t t = fe_mul<S>(P[i >> 1], blinds[i]);
        if (i & 1) S1 = fe_add<S>(S1, t);
        else S0 = fe_add<S>(S0, t);
      }
      if (wait_for(state) != 1) return;
      const fe_t rl = r[nvr - 1];
      bool launched = false;
      if (nfixed + 1 < 1024) {  // the last level on the device (k_multi_mul_coop EXPAND): the launch goes out before this thread forms it for r_LZ
        const fe_t s01[2] = {S0, S1};
        ck(sp_fbtables_multi_mul_begin_eq(ctx, tabs, u64p(P.data()), nfixed, u64p(s01), u64p(&rl)), "comm_LZ (begin)");
        ck(sp_rowmat_vec_eq_begin_with(ctx, psp->W, u64p(r), nvr, cols, dn == cols ? u64p(dv) : nullptr, &vec), "bind_with_delayed (begin)");
        launched = true;
      }
      std::vector<fe_t> sc(nfixed + 1);
      for (size_t h = 0; h < P.size(); ++h) {
        const fe_t hi = fe_mul<S>(P[h], rl), lo = fe_sub<S>(P[h], hi);
        if (2 * h < nfixed) sc[2 * h] = lo;
        if (2 * h + 1 < nfixed) sc[2 * h + 1] = hi;
      }
      const fe_t hs = fe_add<S>(S0, fe_mul<S>(rl, fe_sub<S>(S1, S0)));
      sc[nfixed] = hs;
      if (!launched) {
        ck(sp_fbtables_multi_mul_begin(ctx, tabs, u64p(sc.data()), sc.size()), "comm_LZ (begin)");
        ck(sp_rowmat_vec_eq_begin_with(ctx, psp->W, u64p(r), nvr, cols, dn == cols ? u64p(dv) : nullptr, &vec), "bind_with_delayed (begin)");
      }
      fe_t acc = hs;  // r_LZ = <L, r_W> (hyrax_pc.rs:446-455)
      for (size_t i = 0; i < nfixed; ++i) acc = fe_add<S>(acc, fe_mul<S>(sc[i], blinds[i]));
      r_LZ = acc;
      ck(sp_fbtables_multi_mul_finish(ctx, u64p(&comm_LZ.x)), "comm_LZ (finish)");
      have_comm_LZ = true;
      return;
    }
    if (wait_for(state) != 1) return;
    const size_t hb = nvr / 2, lb = nvr - hb;
    ck(sp_msm_eq_begin(ctx, psp->comm_pts, u64p(r), nvr, &job), "comm_LZ (begin)");
    ck(sp_rowmat_vec_eq_begin_with(ctx, psp->W, u64p(r), nvr, cols, dn == cols ? u64p(dv) : nullptr, &vec), "bind_with_delayed (begin)");
    // r_LZ = <L, r_W> with L = eq(r) = left (x) right: 2^nvr + 2^(nvr/2) products instead of 2 * 2^nvr
    const std::vector<fe_t> left = eq_evals_host(r, hb), right = eq_evals_host(r + hb, lb);
    fe_t acc = fe_zero();
    for (size_t a = 0; a < left.size(); ++a) {
      fe_t inner = fe_zero();
      for (size_t c2 = 0; c2 < right.size(); ++c2) inner = fe_add<S>(inner, fe_mul<S>(right[c2], blinds[a * right.size() + c2]));
      acc = fe_add<S>(acc, fe_mul<S>(left[a], inner));
    }
    r_LZ = acc;
  }
};
struct BgJoin {  // comm_W, r_W and the LzAhead must outlive the job on every exit path
  Background& b;
  std::atomic<int>&st, &st2;
  sp_ctx* ctx;
  sp_msm_job *&j1, *&j2;
  sp_vec_job*& v1;
  ~BgJoin() {
    int zero = 0;
    st2.compare_exchange_strong(zero, 2);
    zero = 0;
    st.compare_exchange_strong(zero, 2);
    b.wait_nothrow();
    // an abandoned prove (error exit) still owns whatever the helper had started: finish the jobs to release them
    uint64_t sink[8];
    if (j1) sp_msm_job_finish(ctx, j1, sink);
    if (j2) sp_msm_job_finish(ctx, j2, sink);
    if (v1) {
      std::vector<uint64_t> big(4 * 2048);
      sp_rowmat_vec_eq_finish(ctx, v1, big.data());
    }
    j1 = j2 = nullptr;
    v1 = nullptr;
  }
};
// evals_rx started four rounds before r_x is complete (sp_eq_table_begin builds the half tables of the first ell - 4 coordinates on a stream of
// its own; sp_eq_table_finish behind the last challenge is then one launch): the outer sum-check's challenge observer
struct EqObs {
  sp_ctx* ctx;
  size_t ell;
  fe_t r[24];
  LzAhead* lz;  // non-null: delta's MSM is the helper's to issue (see there)
  int rc = 0;
  bool begun = false;
  static void fn(void* u, size_t round, const uint64_t r[4]) {
    EqObs* o = (EqObs*)u;
    if (o->lz && round + delta_rounds_before_end() == o->ell) o->lz->publish(o->lz->delta_state, 1);
    if (round + 4 >= o->ell) return;  // the last four coordinates (the rounds the host runs itself after the hand-over) are applied by sp_eq_table_finish
    memcpy(&o->r[round], r, 32);
    if (round + 5 == o->ell) {
      o->rc = sp_eq_table_begin(o->ctx, u64p(o->r), o->ell - 4, o->ell);
      o->begun = o->rc == 0;
    }
  }
};

// <R, d> (ipa.rs:148) with R = eq(point[nvr..]) = left (x) right: the partial sums T[b] = sum_a left[a] d[a |right| + b] need only `left`, whose
// variables are bound hb rounds after the row variables - the second helper computes them under the remaining rounds and the prover finishes with
// |right| products instead of |R| + |left| after the last round
struct IpAhead {
  size_t first = 0, hb = 0, nright = 0;  // left = eq(r_y[first .. first + hb))
  fe_t left_r[16], right_r[16];
  std::vector<fe_t> T;
  bool submitted = false;
  // ... and once the last challenge is drawn the same job finishes <R, d> and beta = <R, d> ck_c + r_beta h_c (ipa.rs:148-149) beside the prover's
  // own work on eval_W; it waits for that challenge with a short bounded spin
  std::atomic<int> right_ready{0};
  size_t nright_vars = 0, last_round = 0;
  fe_t r_beta, ip;
  aff_t beta;
  bool beta_ready = false;
  sp_ctx* ctx = nullptr;
  const sp_ck* ck_s = nullptr;
  const aff_t* beta_term = nullptr;           // h_s * r_beta from the first helper job ...
  const std::atomic<int>* term_ready = nullptr;  // ... valid when this is set
  const fe_t* dvec = nullptr;
  void run() {
    const std::vector<fe_t> left = eq_evals_host(left_r, hb);
    T.assign(nright, fe_zero());
    for (size_t a = 0; a < left.size(); ++a)
      for (size_t b = 0; b < nright; ++b) T[b] = fe_add<S>(T[b], fe_mul<S>(left[a], dvec[a * nright + b]));
    const auto t0 = std::chrono::steady_clock::now();
    while (right_ready.load(std::memory_order_acquire) == 0) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(150)) return;  // (the prover finishes <R, d> and beta itself; a helper does not sit on a CPU of the quota)
      sp_relax();
    }
    const std::vector<fe_t> right = eq_evals_host(right_r, nright_vars);
    fe_t acc = fe_zero();
    for (size_t b = 0; b < right.size(); ++b) acc = fe_add<S>(acc, fe_mul<S>(right[b], T[b]));
    ip = acc;
    if (term_ready->load(std::memory_order_acquire)) ck(sp_hyrax_commit_small_with_term(ctx, ck_s, u64p(&ip), 1, u64p(&beta_term->x), u64p(&beta.x)), "beta");
    else ck(sp_hyrax_commit_small(ctx, ck_s, u64p(&ip), 1, u64p(&r_beta), u64p(&beta.x)), "beta");
    beta_ready = true;
  }
};
// the inner sum-check's challenge observer: r_y[0] selects W against (1, X); r_y[1 ..= nvr] are the row variables of W (MSB first): once they are drawn
// the first helper can start comm_LZ; the column variables go to the IpAhead, whose job is posted when `left` is complete
struct Obs {
  LzAhead* lz;
  bool on;
  IpAhead* ipa;
  Background* bg2;
  static void fn(void* u, size_t round, const uint64_t r[4]) {
    Obs* o = (Obs*)u;
    if (!o->on || round == 0) return;
    if (round <= o->lz->nvr) {
      memcpy(&o->lz->r[round - 1], r, 32);
      o->lz->rows_known.store((int)round, std::memory_order_release);
      if (round == o->lz->nvr) o->lz->publish(o->lz->state, 1);
      return;
    }
    IpAhead* ip = o->ipa;
    if (!ip->hb || round < ip->first) return;
    if (round >= ip->first + ip->hb) {
      memcpy(&ip->right_r[round - ip->first - ip->hb], r, 32);
      if (round == ip->last_round) ip->right_ready.store(1, std::memory_order_release);
      return;
    }
    memcpy(&ip->left_r[round - ip->first], r, 32);
    if (round + 1 == ip->first + ip->hb) {
      o->bg2->submit([ip] { ip->run(); });
      ip->submitted = true;
    }
  }
};
struct IpJoin {  // the IpAhead and dvec outlive the job on every exit path
  Background& b;
  ~IpJoin() { b.wait_nothrow(); }
};

// SpartanSNARK::prove (src/spartan.rs:219-466)
// `synth`: circuit.synthesize(.., Some(&challenges)) for circuits with verifier challenges (bellpepper/r1cs.rs:443-461): receives the challenges and
// writes the num_rest_unpadded values of the rest segment (Montgomery limbs); non-zero return = SynthesisError
ProofBuf prove_reference_order(const SpartanProverKey& pk, SpartanPrepSNARK& ps, const uint64_t* publics_u64, size_t npub, Tape& tape, PhaseTimes* pt, ss_rest_hook synth,
                                      void* synth_user);
ProofBuf prove(const SpartanProverKey& pk, SpartanPrepSNARK& ps, const uint64_t* publics_u64, size_t npub, Tape& tape, PhaseTimes* pt, ss_rest_hook synth = nullptr,
                      void* synth_user = nullptr) {
  if (ps.flags & FLAG_REFERENCE_ORDER) return prove_reference_order(pk, ps, publics_u64, npub, tape, pt, synth, synth_user);
  const sp_dims& d = pk.dims;
  sp_ctx* ctx = pk.ctx;
  const size_t M = pk.num_vars, N = d.num_cons, W_ = DEFAULT_COMMITMENT_WIDTH;
  if (npub != d.num_public) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "public_values length");
  ck(sp_ctx_bind_thread(ctx), "device");  // the caller may be a thread other than the one that created the context
  const ActiveProve active_prove;
  const double t_start = now_ms();
  double t_lap = t_start;
  auto lap = [&](const char* name) {
    if (!pt) return;
    double t = now_ms();
    pt->laps.emplace_back(name, t - t_lap);
    t_lap = t;
  };
  // First thing: the commitment to the rest segment (bellpepper/r1cs.rs:463-491) when it is all padding, i.e. commit_zeros (hyrax_pc.rs:305-319) = h * blind
  // per row. Its kernel (~30 us of dependent point additions) + the host's batch normalisation + the absorb of the rows + the squeeze of tau is the chain
  // the outer sum-check's first evaluation waits for, so the blinds are drawn and the kernel launched before anything else on this thread.
  const size_t rows_pre = ps.comm_W_fixed.size(), rows_rest = (d.num_rest + W_ - 1) / W_;
  std::vector<fe_t> r_W_rest(rows_rest);
  for (auto& b : r_W_rest) b = tape.next();
  lap("rest_blinds");
  sp_fb_job* rest_job = nullptr;
  FbJobGuard rest_job_guard{ctx, rest_job, rows_rest};
  if (rows_rest && d.num_rest_unpadded == 0) ck(sp_fixed_base_mul_h_begin(ctx, pk.ck, u64p(r_W_rest.data()), rows_rest, &rest_job), "commit_zeros (begin)");
  lap("commit_zeros_begin");
  const std::vector<fe_t> publics = publics_from_u64(publics_u64, npub);
  lap("publics");

  // the second helper's job (PrefixJob): the transcript prefix, d_vec and the blinds, the two blind terms
  const size_t n_ipa = M < W_ ? M : W_;
  const std::unique_ptr<fe_t[]> dvec_store(new fe_t[n_ipa]);  // (not value-initialised: the helper's draw writes every element; a zeroed vector was 12 us here)
  fe_t* const dvec = dvec_store.get();
  const bool prefix_cached = (ps.flags & FLAG_PREFIX_CACHE) != 0;
  if (prefix_cached) {
    if (!ps.tr_prefix) {
      ps.tr_prefix = instance_prefix(ctx, pk, ps, publics.data(), npub);
      ps.tr_publics = publics;
    } else if (ps.tr_publics.size() != publics.size() || memcmp(ps.tr_publics.data(), publics.data(), publics.size() * sizeof(fe_t)) != 0) {
      throw Error(SP_ERR_INTERNAL, "public values changed between proves on one prep state");
    }
  }
  PrefixJob pre{ctx, &ps, &pk, publics.data(), npub, prefix_cached, Tape{tape.bytes, tape.blocks, tape.pos + 1}, dvec, n_ipa,
                fe_from_uniform<S>(tape.bytes + 64 * (tape.pos < tape.blocks ? tape.pos : 0))};
  ps.bg2.submit([&pre] { pre.run(); });
  lap("helper_submit");
  // a flag the second helper's job raises; if the helper has not even begun the job 30 us after it was posted, the job runs here (Background::try_steal)
  auto await_flag = [&ps](std::atomic<int>& flag) {
    for (unsigned spins = 0; flag.load(std::memory_order_acquire) == 0; ++spins) {
      if ((spins & 63u) == 63u) ps.bg2.try_steal();
      sp_relax();
    }
  };
  PrefixJoin prefix_join{ps.bg2};
  lap("transcript_prefix");
  Tr tr(nullptr, Tr::Adopt{});
  auto acquire_transcript = [&] {
    if (tr.t) return;
    if (prefix_cached) ck(sp_transcript_clone(ps.tr_prefix, &tr.t), "transcript_clone");
    else {
      await_flag(pre.prefix_ready);
      tr.t = ps.tr_fresh;
      ps.tr_fresh = nullptr;
      if (!tr.t) {
        ps.bg2.wait();  // (rethrows what the job threw)
        throw Error(SP_ERR_INTERNAL, "transcript prefix was not prepared");
      }
    }
  };
  // verifier challenges (bellpepper/r1cs.rs:429-431) and the rest of the witness that depends on them (:443-461): squeezed right after the
  // precommitted commitment, before anything that needs z
  std::vector<fe_t> challenges;
  if (d.num_challenges) {
    acquire_transcript();
    challenges = squeeze_challenges(tr, d.num_challenges);
    const std::vector<fe_t> rest = synthesize_rest(synth, synth_user, u64p(challenges.data()), challenges.size(), d.num_rest_unpadded);
    if (d.num_rest_unpadded) ck(sp_table_write(ctx, ps.W, d.num_shared + d.num_precommitted, u64p(rest.data()), d.num_rest_unpadded), "W rest");
  }

  // z = [W | 1 | public | challenges]   (src/spartan.rs:246-253); the table is 2M long so the inner sum-check can run in place
  // The matrix-vector product below reads only the rest / public / challenge columns of z (multiply_vec_incremental_into, src/r1cs/mod.rs:1170-1211: the
  // precommitted part is cached), so only those go through the main stream in front of it; the bulk - the shared and precommitted columns and the zeros
  // of the high half, 96 MB at config 2 - is assembled beside the main stream and joined in front of the outer sum-check (its first reader is the inner one).
  ck(sp_table_set_len(ps.z, 2 * M, (size_t)-1, (size_t)-1), "z len");
  // (a rest segment that is all padding has no matrix entries in its columns: it goes with the bulk)
  const size_t z_fixed = d.num_rest_unpadded ? d.num_shared + d.num_precommitted : M;
  if (M > z_fixed) ck(sp_table_copy(ctx, ps.z, z_fixed, ps.W, z_fixed, M - z_fixed), "z <- W rest");
  {
    const std::vector<fe_t> tail = z_tail(pk.num_extra, publics, challenges);
    if (tail.size() <= 2048) ck(sp_table_write_async(ctx, ps.z, M, u64p(tail.data()), tail.size()), "z tail");  // no synchronisation in front of the matrix-vector product
    else ck(sp_table_write(ctx, ps.z, M, u64p(tail.data()), tail.size()), "z tail");
  }
  ck(sp_table_set_len(ps.z, pk.num_cols, (size_t)-1, (size_t)-1), "z len");
  lap("z_build");
  // Az, Bz, Cz (src/spartan.rs:271-279) depend only on z: issue the product now so that it runs under the commit_zeros job and the host work
  // below instead of after them (the reference computes it after the commitments; the values are the same)
  const double t_mv0 = now_ms();
  if (ps.p0) ck(sp_multiply_vec_incremental_round0(ctx, pk.S, ps.z, ps.caz, ps.cbz, ps.ccz, ps.az, ps.bz, ps.cz, ps.p0, ps.p1), "multiply_vec_incremental");
  else ck(sp_multiply_vec_incremental(ctx, pk.S, ps.z, ps.caz, ps.cbz, ps.ccz, ps.az, ps.bz, ps.cz), "multiply_vec_incremental");
  lap("spmv_issue");
  ck(sp_table_assemble_aside(ctx, ps.z, 0, ps.W, 0, z_fixed, M + pk.num_extra, M - pk.num_extra, 0), "z bulk");
  ck(sp_ctx_aside_join(ctx), "z bulk (join)");  // queued behind the product: by the time the main stream gets there the bulk of z has long been written
  const double t_mv_issue = now_ms() - t_mv0;
  // (the rest segment's commitment: commit_zeros was started at the top and is collected here, after everything the device can be given in the meantime has
  // been issued; a segment with values takes PCS::commit on the resident witness)
  std::vector<aff_t> comm_W(rows_pre + rows_rest);
  std::copy(ps.comm_W_fixed.begin(), ps.comm_W_fixed.end(), comm_W.begin());
  lap("z_bulk_issue");

  const bool rest_job_used = rest_job != nullptr;  // the rest rows are h * blind (commit_zeros)
  if (rest_job) {
    sp_fb_job* j = rest_job;
    rest_job = nullptr;  // finish() consumes the job whatever it returns
    ck(sp_fixed_base_mul_h_finish(ctx, j, u64p(&comm_W[rows_pre].x)), "commit_zeros (finish)");
  }
  else if (rows_rest) commit_rest_values(ctx, pk.ck, ps.W, d, ps.is_small, r_W_rest.data(), comm_W.data() + rows_pre);
  lap("commit_zeros_finish");
  acquire_transcript();
  lap("prefix_join");
  absorb_comm_W_rest(tr, comm_W.data() + rows_pre, rows_rest);
  lap("absorb_comm_W_rest");
  const std::vector<fe_t> r_W = combine_blinds(ps.r_W_fixed, r_W_rest);
  // comm_W is complete: the first helper's job (LzAhead) from here on
  ps.bg.wait();  // (idle: nothing has been posted to the first helper in this prove yet)
  sp_absorb_state_free(ps.poly_com);
  ps.poly_com = nullptr;
  const size_t lz_rows = (M + W_ - 1) / W_, lz_nvr = log2_ceil(lz_rows);
  const bool lz_direct = (ps.flags & FLAG_LZ_DIRECT) != 0;  // the reference's own order (bind W with L first, then the MSM over the key)
  LzAhead lz;
  // (lz.r_delta is set by the opening's job once d_vec and the blinds are drawn: dvec_ready)
  lz.nvr = lz_nvr;
  const bool lz_ahead = !lz_direct && lz_nvr > 0 && lz_nvr <= 20 && comm_W.size() == ((size_t)1 << lz_nvr) && r_W.size() == comm_W.size();
  const size_t lz_cols = (size_t)1 << (log2_ceil(M) - lz_nvr);
  // (tables whose build - queued by prep_prove a moment ago - has not ended are not waited for: this prove takes the MSM over the row commitments)
  const bool lz_tables_path = lz_ahead && ps.lz_tables && rest_job_used && ps.comm_W_fixed.size() + rows_rest == comm_W.size() && sp_fbtables_ready(ps.lz_tables, 0) == 1;
  lz.ctx = ctx;
  lz.rows = comm_W.data();
  lz.nrows = comm_W.size();
  lz.psp = &ps;
  lz.blinds = r_W.data();
  lz.ahead = lz_ahead;
  lz.key = pk.ck;
  lz.cols = lz_cols;
  lz.tabs = lz_tables_path ? ps.lz_tables : nullptr;
  lz.nfixed = ps.comm_W_fixed.size();
  lz.dv = dvec;
  lz.dn = n_ipa;
  lz.dvr = &pre.dvec_ready;
  lz.rda = &pre.r_delta;
  ps.bg.submit([&lz] { lz.run(); });
  BgJoin bg_join{ps.bg, lz.state, lz.delta_state, ctx, lz.job, lz.delta_job, lz.vec};
  const double t_wit = now_ms();

  const size_t num_rounds_x = log2_ceil(N), num_rounds_y = log2_ceil(M) + 1;
  std::vector<fe_t> tau(num_rounds_x);
  for (auto& t : tau) t = tr.squeeze("t");
  lap("tau");

  const double t_mv = now_ms();

  ProofBuf proof;
  proof.header(comm_W, publics, challenges);
  // outer sum-check (src/spartan.rs:291-310)
  std::vector<fe_t> outer_polys(3 * num_rounds_x), r_x(num_rounds_x);
  fe_t claims_outer[3];
  const fe_t zero = fe_zero();
  EqObs eq_obs{ctx, num_rounds_x, {}, lz_ahead ? &lz : nullptr};
  const bool use_eq_obs = num_rounds_x >= 12 && num_rounds_x <= 20;
  if (use_eq_obs)
    ck(sp_sumcheck_cubic3_observed(ctx, u64p(&zero), u64p(tau.data()), num_rounds_x, ps.az, ps.bz, ps.cz, ps.p0, ps.p0 ? ps.p1 : nullptr, tr.t, &EqObs::fn, &eq_obs,
                                   u64p(outer_polys.data()), u64p(r_x.data()), u64p(claims_outer)),
       "outer sum-check");
  else if (ps.p0)
    ck(sp_sumcheck_cubic3_round0(ctx, u64p(&zero), u64p(tau.data()), num_rounds_x, ps.az, ps.bz, ps.cz, ps.p0, ps.p1, tr.t, u64p(outer_polys.data()), u64p(r_x.data()),
                                 u64p(claims_outer)),
       "outer sum-check");
  else
    ck(sp_sumcheck_cubic3(ctx, u64p(&zero), u64p(tau.data()), num_rounds_x, ps.az, ps.bz, ps.cz, tr.t, u64p(outer_polys.data()), u64p(r_x.data()),
                          u64p(claims_outer)),
       "outer sum-check");
  if (eq_obs.rc) throw Error(eq_obs.rc, std::string("evals_rx (begin): ") + sp_last_error());
  if (lz_ahead) lz.publish(lz.delta_state, 1);  // (a sum-check of fewer than 15 rounds, or one without the observer, has not done it)
  tr.absorb_scalars("claims_outer", claims_outer, 3);
  proof.outer(outer_polys.data(), num_rounds_x, claims_outer);
  const double t_outer = now_ms();

  const fe_t r = tr.squeeze("r");
  const fe_t claim_inner_joint = joint_inner_claim(claims_outer, r);
  // evals_rx + bind_and_prepare_poly_ABC (src/spartan.rs:316-322)
  ck(sp_eq_table_finish(ctx, u64p(r_x.data()), num_rounds_x, ps.rx), "evals_rx");  // (= sp_eq_table_into when nothing was begun)
  ck(sp_poly_abc(ctx, pk.S, ps.rx, u64p(&r), 2 * M, ps.abc), "poly_ABC");
  const double t_abc = now_ms();

  sp_msm_job* delta_job = nullptr;
  await_flag(pre.dvec_ready);  // d_vec, r_delta, r_beta from here on
  if (!lz_ahead) ck(sp_msm_ck_begin(ctx, pk.ck, u64p(dvec), n_ipa, &delta_job), "delta (begin)");
  // inner sum-check. The reference runs round 0 by hand on the compact vectors (src/spartan.rs:323-384); that round is
  // value-identical to a generic prove_quad round on the 2M-long tables with (lo_eff, hi_eff) = (M, num_extra).
  ck(sp_table_set_len(ps.abc, 2 * M, M, pk.num_extra), "abc len");
  ck(sp_table_set_len(ps.z, 2 * M, M, pk.num_extra), "z len");
  std::vector<fe_t> inner_polys(2 * num_rounds_y), r_y(num_rounds_y);
  fe_t claims_inner[2];
  // the row variables go to the first helper (comm_LZ), the column variables to the second (<R, d>, beta): Obs, IpAhead
  IpAhead ipa;
  ipa.beta_term = &pre.beta_term;
  ipa.term_ready = &pre.eval_W_term_ready;
  ipa.r_beta = pre.r_beta;
  ipa.dvec = dvec;
  ipa.ctx = ctx;
  ipa.ck_s = pk.ck_s;
  if (lz_ahead) {
    const size_t k = (num_rounds_y - 1) - lz_nvr;
    ipa.first = 1 + lz_nvr;
    ipa.hb = k / 2;
    ipa.nright = (size_t)1 << (k - ipa.hb);
    ipa.nright_vars = k - ipa.hb;
    ipa.last_round = num_rounds_y - 1;
    if (ipa.nright_vars > 16) ipa.hb = 0;
    if (ipa.hb == 0 || ipa.hb > 16 || (((size_t)1 << ipa.hb) * ipa.nright) != n_ipa) ipa.hb = 0;  // (not this shape: the prover computes <R, d> itself)
  }
  Obs obs{&lz, lz_ahead, &ipa, &ps.bg2};
  IpJoin ip_join{ps.bg2};
  ck(sp_sumcheck_quad_observed(ctx, u64p(&claim_inner_joint), num_rounds_y, ps.abc, ps.z, tr.t, &Obs::fn, &obs, u64p(inner_polys.data()), u64p(r_y.data()),
                               u64p(claims_inner)),
     "inner sum-check");
  proof.inner(inner_polys.data(), num_rounds_y);
  const fe_t eval_W = eval_W_from(claims_inner[1], r_y.data(), num_rounds_y, publics, challenges);
  lap("inner+eval_W");
  const double t_inner = now_ms();

  // pcs (src/spartan.rs:423-437) -> HyraxPCS::prove (hyrax_pc.rs:387-478) -> InnerProductArgumentLinear::prove (ipa.rs:125-170).
  // Device work is issued first (row-matrix product, comm_LZ's MSM on the auxiliary stream); the host-side pieces that do not
  // depend on it (commitment to eval_W, hashing comm_W, <R, d>, beta) run underneath. Transcript ORDER is the reference's.
  const fe_t blind_eval_W = tape.next();
  proof.pf(eval_W);
  proof.pf(blind_eval_W);
  const fe_t* point = r_y.data() + 1;
  const size_t npoint = num_rounds_y - 1;
  const size_t num_rows = (M + W_ - 1) / W_, nvr = log2_ceil(num_rows);
  aff_t comm_LZ;
  std::vector<fe_t> R, LZ;
  fe_t r_LZ;
  sp_msm_job* lz_job = nullptr;
  if (nvr == 0) {
    comm_LZ = comm_W[0];
    R = eq_evals_host(point, npoint);
    LZ.resize(M);
    ck(sp_table_read(ctx, ps.W, 0, M, u64p(LZ.data())), "read W");
    r_LZ = r_W[0];
  } else if (lz_ahead) {
    // comm_LZ's MSM and the row-matrix product have been running since round nvr of the inner sum-check
    LZ.resize(lz_cols);
    if (lz_tables_path) {
      // the helper delivers comm_LZ itself (one multi_mul over the prepared tables): join it only where comm_LZ is absorbed; what is needed before
      // that (poly_com, delta) was finished under the inner sum-check
      const auto t0 = std::chrono::steady_clock::now();
      for (unsigned spins = 0; lz.early_done.load(std::memory_order_acquire) == 0; ++spins) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) throw Error(SP_ERR_INTERNAL, "the PCS helper did not finish delta");
        if ((spins & 63u) == 63u) ps.bg.try_steal();  // the helper thread never woke for this prove: its whole job runs here (every state it waits for is published)
        sp_relax();
      }
    } else {
      ps.bg.wait();
      if (!lz.job || !lz.vec || !lz.delta_done) throw Error(SP_ERR_INTERNAL, "comm_LZ was not started");
      lz_job = lz.job;
      lz.job = nullptr;
      r_LZ = lz.r_LZ;
    }
    lap("helper_join");
  } else {
    std::vector<fe_t> L = eq_evals_host(point, nvr);
    LZ.resize((size_t)1 << (npoint - nvr));
    ck(sp_rowmat_vec(ctx, ps.W, L.size(), LZ.size(), u64p(L.data()), u64p(LZ.data())), "bind_with_delayed");
    ck(sp_msm_ck_begin(ctx, pk.ck, u64p(LZ.data()), LZ.size(), &lz_job), "comm_LZ (begin)");
    lap("eq_L+rowmat_vec+msm_begin");
    r_LZ = fe_zero();
    for (size_t i = 0; i < L.size(); ++i) r_LZ = fe_add<S>(r_LZ, fe_mul<S>(L[i], r_W[i]));
  }
  aff_t comm_eval_W;
  if (pre.eval_W_term_ready.load(std::memory_order_acquire) && memcmp(&pre.eval_W_term_blind, &blind_eval_W, sizeof(fe_t)) == 0)
    ck(sp_hyrax_commit_small_with_term(ctx, pk.ck_s, u64p(&eval_W), 1, u64p(&pre.eval_W_term.x), u64p(&comm_eval_W.x)), "commit eval_W");
  else
    ck(sp_hyrax_commit_small(ctx, pk.ck_s, u64p(&eval_W), 1, u64p(&blind_eval_W), u64p(&comm_eval_W.x)), "commit eval_W");
  lap("comm_eval_W");
  if (!lz_tables_path) ps.bg.wait();
  ck(sp_transcript_absorb_prepared(tr.t, ps.poly_com), "poly_com");
  lap("poly_com");
  tr.dom_sep("inner product argument (linear)");
  const size_t n = (size_t)1 << (nvr == 0 ? npoint : npoint - nvr);  // |R|
  if (n != n_ipa) throw Error(SP_ERR_INTERNAL, "IPA width mismatch");
  tape.skip(n);  // the d_vec blocks that were peeked at the start
  const fe_t r_delta = tape.next(), r_beta = tape.next();
  // <R, d> (ipa.rs:148) with R = eq(point[nvr..]) = left (x) right: n + sqrt(n) products, R itself is never needed
  fe_t ip = fe_zero();
  aff_t delta, beta;
  bool have_beta = false;
  if (R.empty() && ipa.submitted) {
    ps.bg2.wait();
    if (ipa.beta_ready && memcmp(&ipa.r_beta, &r_beta, sizeof(fe_t)) == 0) {
      ip = ipa.ip;
      beta = ipa.beta;
      have_beta = true;
    }
  }
  lap("ipa_join");
  if (have_beta) {
  } else if (R.empty() && ipa.submitted) {
    const size_t k = npoint - nvr;
    const std::vector<fe_t> right = eq_evals_host(point + nvr + ipa.hb, k - ipa.hb);
    if (right.size() != ipa.T.size()) throw Error(SP_ERR_INTERNAL, "<R, d>: partial sums of the wrong width");
    for (size_t b = 0; b < right.size(); ++b) ip = fe_add<S>(ip, fe_mul<S>(right[b], ipa.T[b]));
  } else if (R.empty()) {
    const size_t k = npoint - nvr, hb = k / 2;
    const std::vector<fe_t> left = eq_evals_host(point + nvr, hb), right = eq_evals_host(point + nvr + hb, k - hb);
    for (size_t a = 0; a < left.size(); ++a) {
      fe_t inner = fe_zero();
      for (size_t b = 0; b < right.size(); ++b) inner = fe_add<S>(inner, fe_mul<S>(right[b], dvec[a * right.size() + b]));
      ip = fe_add<S>(ip, fe_mul<S>(left[a], inner));
    }
  } else {
    for (size_t i = 0; i < n; ++i) ip = fe_add<S>(ip, fe_mul<S>(R[i], dvec[i]));
  }
  if (!have_beta) ck(sp_hyrax_commit_small(ctx, pk.ck_s, u64p(&ip), 1, u64p(&r_beta), u64p(&beta.x)), "beta");
  if (lz_ahead) {
    delta = lz.delta;  // finished by the helper with the blind peeked from the same tape position
    if (memcmp(&r_delta, &lz.r_delta, sizeof(fe_t)) != 0) throw Error(SP_ERR_INTERNAL, "tape positions of r_delta disagree");
  } else {
    // delta's device part finished long ago (it was issued before the inner sum-check): its window Horner runs on the host while the device
    // still works on comm_LZ
    ck(sp_msm_ck_finish(ctx, pk.ck, delta_job, u64p(&r_delta), u64p(&delta.x)), "delta (finish)");
  }
  lap("host_side_under_msm");
  if (lz_tables_path) {
    ps.bg.wait();
    if (!lz.have_comm_LZ || !lz.vec) throw Error(SP_ERR_INTERNAL, "comm_LZ was not delivered");
    comm_LZ = lz.comm_LZ;
    r_LZ = lz.r_LZ;
  } else if (lz_job && lz_ahead) ck(sp_msm_job_finish(ctx, lz_job, u64p(&comm_LZ.x)), "comm_LZ (finish)");  // the blinds are inside the row commitments
  else if (lz_job) ck(sp_msm_ck_finish(ctx, pk.ck, lz_job, u64p(&r_LZ), u64p(&comm_LZ.x)), "comm_LZ (finish)");
  lap("comm_LZ_finish");
  absorb_ipa_instance(tr, comm_LZ, comm_eval_W, delta, beta);
  const fe_t rr = tr.squeeze("r");
  proof.pp(delta);
  proof.pp(beta);
  const bool zvec_on_device = lz_ahead && n == lz_cols && n == n_ipa;  // the helper's job gave d_vec to the product's job (begin_with)
  if (zvec_on_device) {
    // z_vec = r * LZ + d (ipa.rs:160-163), the last step of the prove: one launch behind the product the device already holds, delivered through mapped
    // memory straight into the proof (2048 products were 33 us on this thread and the two helpers)
    sp_vec_job* vj = lz.vec;
    lz.vec = nullptr;
    const size_t at = proof.words.size();
    proof.words.resize(at + 4 * n);
    ck(sp_rowmat_vec_eq_finish_scaled(ctx, vj, u64p(&rr), proof.words.data() + at), "z_vec");
  } else {
    if (lz_ahead) {
      sp_vec_job* vj = lz.vec;
      lz.vec = nullptr;
      ck(sp_rowmat_vec_eq_finish(ctx, vj, u64p(LZ.data())), "bind_with_delayed (finish)");
    }
    // z_vec = r * LZ + d: split three ways with the two helper threads when it is wide enough to pay
    std::vector<fe_t> zv(n);
    auto part = [&zv, &LZ, dvec, rr](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) zv[i] = fe_add<S>(fe_mul<S>(rr, LZ[i]), dvec[i]);
    };
    if (n >= 1024 && lz_ahead) {
      const size_t a = n * 46 / 100, b = a + (n - a) / 2;  // the owner starts at once, the helpers have to wake up first
      ps.bg.submit([&part, a, b] { part(a, b); });
      ps.bg2.submit([&part, b, n] { part(b, n); });
      part(0, a);
      ps.bg.wait();
      ps.bg2.wait();
    } else {
      part(0, n);
    }
    proof.words.insert(proof.words.end(), u64p(zv.data()), u64p(zv.data()) + 4 * n);
  }
  proof.pf(fe_add<S>(fe_mul<S>(rr, r_LZ), r_delta));
  proof.pf(fe_add<S>(fe_mul<S>(rr, blind_eval_W), r_beta));
  lap("z_vec");
  const double t_end = now_ms();
  if (pt) fill_phase_ms(pt->ms, t_start, t_wit, t_mv, t_outer, t_abc, t_inner, t_end, t_mv_issue);  // the matrix-vector product is issued inside the witness phase and runs under it
  ps.queue_lz_tables(ctx);
  return proof;
}

// SpartanSNARK::prove exactly as src/spartan.rs:219-466 states it — one statement of the reference per call of the ABI, in its order, on the calling
// thread alone: no helper threads, nothing issued ahead of where the reference computes it; of prep_prove's products only the FixedBaseMul tables of the rows it
// committed are used (the shim keeps them in its PrepSNARK and names them when it announces the opening). Whatever overlap there is
// happens BELOW the ABI (the round loops' launch-ahead and resident tails, sp_hyrax_prove's two walks beside its hashing). This is the time an unchanged
// spartan.rs gets from a shim that binds include/spartan_hip.h; the proof is the same bytes as prove()'s.
ProofBuf prove_reference_order(const SpartanProverKey& pk, SpartanPrepSNARK& ps, const uint64_t* publics_u64, size_t npub, Tape& tape, PhaseTimes* pt, ss_rest_hook synth,
                                      void* synth_user) {
  const sp_dims& d = pk.dims;
  sp_ctx* ctx = pk.ctx;
  const size_t M = pk.num_vars, N = d.num_cons, W_ = DEFAULT_COMMITMENT_WIDTH;
  if (npub != d.num_public) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "public_values length");
  ck(sp_ctx_bind_thread(ctx), "device");
  const double t_start = now_ms();
  static const bool laps_on = getenv("SPARTAN_HOST_LAPS") != nullptr;
  double t_lap = t_start;
  auto lap = [&](const char* name) {
    if (!laps_on) return;
    const double t = now_ms();
    fprintf(stderr, "ref lap %-28s %.3f ms\n", name, t - t_lap);
    t_lap = t;
  };
  const std::vector<fe_t> publics = publics_from_u64(publics_u64, npub);
  // :226-236 transcript, vk, public values; r1cs_instance_and_witness (src/bellpepper/r1cs.rs:411-540)
  Tr tr(ctx, "SpartanSNARK");
  ck(sp_transcript_set_async(tr.t, 1), "transcript");  // (the shim's TranscriptEngine: long absorbs hashed beside the caller's next calls)
  absorb_instance_prefix(tr, pk.vk_digest, publics.data(), npub, ps.comm_shared_bytes, ps.comm_pre_bytes);
  std::vector<fe_t> challenges;
  if (d.num_challenges) {
    challenges = squeeze_challenges(tr, d.num_challenges);
    const std::vector<fe_t> rest = synthesize_rest(synth, synth_user, u64p(challenges.data()), challenges.size(), d.num_rest_unpadded);
    if (d.num_rest_unpadded) ck(sp_table_write(ctx, ps.W, d.num_shared + d.num_precommitted, u64p(rest.data()), d.num_rest_unpadded), "W rest");
  }
  lap("transcript prefix");
  const size_t rows_pre = ps.comm_W_fixed.size(), rows_rest = (d.num_rest + W_ - 1) / W_;
  std::vector<fe_t> r_W_rest(rows_rest);
  for (auto& b : r_W_rest) b = tape.next();  // PCS::blind (r1cs.rs:466)
  std::vector<aff_t> comm_W(rows_pre + rows_rest);
  std::copy(ps.comm_W_fixed.begin(), ps.comm_W_fixed.end(), comm_W.begin());
  commit_rest_rows(ctx, pk.ck, ps.W, d, ps.is_small, r_W_rest.data(), rows_rest, comm_W.data() + rows_pre);
  lap("commit rest rows");
  absorb_comm_W_rest(tr, comm_W.data() + rows_pre, rows_rest);
  lap("absorb comm_W_rest");
  const std::vector<fe_t> r_W = combine_blinds(ps.r_W_fixed, r_W_rest);
  // The shim's r1cs_instance_and_witness wrapper ends by announcing the opening PCS::prove will be asked for (sp_hyrax_prove_announce): commitment, blinds
  // and the IPA's randomness exist here — the reference draws that randomness inside InnerProductArgumentLinear::prove from OsRng; with the injected
  // tape it is the cols + 2 blocks behind blind_eval_W's one — and the library starts the opening's transcript-independent parts under the sum-checks.
  struct Announced {  // an error exit must not leave the announcement (it points at ps.W) on the context
    sp_ctx* ctx;
    bool done = false;
    ~Announced() {
      if (!done) (void)sp_hyrax_prove_retract(ctx);
    }
  } announced{ctx};
  if (tape.pos + 1 < tape.blocks) {
    // (with the tables of the committed rows the shim's prep_prove built - ps.lz_tables: the precommitted rows and h - when the remaining rows are commit_zeros)
    if (ps.lz_tables && rows_rest && d.num_rest_unpadded == 0)
      ck(sp_hyrax_prove_announce_tables(ctx, pk.ck, u64p(&comm_W[0].x), comm_W.size(), ps.W, M, u64p(r_W.data()), tape.bytes + 64 * (tape.pos + 1), tape.blocks - tape.pos - 1,
                                        ps.lz_tables, rows_pre),
         "PCS::prove (announce)");
    else
      ck(sp_hyrax_prove_announce(ctx, pk.ck, u64p(&comm_W[0].x), comm_W.size(), ps.W, M, u64p(r_W.data()), tape.bytes + 64 * (tape.pos + 1), tape.blocks - tape.pos - 1),
         "PCS::prove (announce)");
  }
  lap("announce");
  const double t_wit = now_ms();
  // :246-253 z = [W | 1 | public | challenges]
  ck(sp_table_set_len(ps.z, 2 * M, (size_t)-1, (size_t)-1), "z len");
  ck(sp_table_copy(ctx, ps.z, 0, ps.W, 0, M), "z <- W");
  {
    ck(sp_table_zero(ctx, ps.z, M, M), "clear z high half");
    const std::vector<fe_t> tail = z_tail(pk.num_extra, publics, challenges);
    if (tail.size() <= 2048) ck(sp_table_write_async(ctx, ps.z, M, u64p(tail.data()), tail.size()), "z tail");
    else ck(sp_table_write(ctx, ps.z, M, u64p(tail.data()), tail.size()), "z tail");
  }
  ck(sp_table_set_len(ps.z, pk.num_cols, (size_t)-1, (size_t)-1), "z len");
  lap("z");
  // :262-264 tau
  const size_t num_rounds_x = log2_ceil(N), num_rounds_y = log2_ceil(M) + 1;
  std::vector<fe_t> tau(num_rounds_x);
  for (auto& t : tau) t = tr.squeeze("t");
  lap("tau");
  // :267-283 multiply_vec_incremental_into
  ck(sp_multiply_vec_incremental(ctx, pk.S, ps.z, ps.caz, ps.cbz, ps.ccz, ps.az, ps.bz, ps.cz), "multiply_vec_incremental");
  lap("multiply_vec_incremental");
  const double t_mv = now_ms();
  ProofBuf proof;
  proof.header(comm_W, publics, challenges);
  // :291-310 outer sum-check
  std::vector<fe_t> outer_polys(3 * num_rounds_x), r_x(num_rounds_x);
  fe_t claims_outer[3];
  const fe_t zero = fe_zero();
  ck(sp_sumcheck_cubic3(ctx, u64p(&zero), u64p(tau.data()), num_rounds_x, ps.az, ps.bz, ps.cz, tr.t, u64p(outer_polys.data()), u64p(r_x.data()), u64p(claims_outer)),
     "outer sum-check");
  tr.absorb_scalars("claims_outer", claims_outer, 3);
  proof.outer(outer_polys.data(), num_rounds_x, claims_outer);
  const double t_outer = now_ms();
  // :311-322 r, evals_rx, bind_and_prepare_poly_ABC
  const fe_t r = tr.squeeze("r");
  const fe_t claim_inner_joint = joint_inner_claim(claims_outer, r);
  ck(sp_eq_table_into(ctx, u64p(r_x.data()), num_rounds_x, ps.rx), "evals_rx");
  ck(sp_poly_abc(ctx, pk.S, ps.rx, u64p(&r), 2 * M, ps.abc), "poly_ABC");
  const double t_abc = now_ms();
  // :323-404 inner sum-check (manual round 0 == a generic round on (lo_eff, hi_eff) = (M, num_extra) tables)
  ck(sp_table_set_len(ps.abc, 2 * M, M, pk.num_extra), "abc len");
  ck(sp_table_set_len(ps.z, 2 * M, M, pk.num_extra), "z len");
  std::vector<fe_t> inner_polys(2 * num_rounds_y), r_y(num_rounds_y);
  fe_t claims_inner[2];
  ck(sp_sumcheck_quad(ctx, u64p(&claim_inner_joint), num_rounds_y, ps.abc, ps.z, tr.t, u64p(inner_polys.data()), u64p(r_y.data()), u64p(claims_inner)), "inner sum-check");
  proof.inner(inner_polys.data(), num_rounds_y);
  // :405-421 eval_W
  const fe_t eval_W = eval_W_from(claims_inner[1], r_y.data(), num_rounds_y, publics, challenges);
  lap("eval_W");
  const double t_inner = now_ms();
  // :423-436 blind, commit to eval_W, PCS::prove
  const fe_t blind_eval_W = tape.next();
  aff_t comm_eval_W;
  ck(sp_hyrax_commit_small(ctx, pk.ck_s, u64p(&eval_W), 1, u64p(&blind_eval_W), u64p(&comm_eval_W.x)), "commit eval_W");
  lap("commit eval_W");
  proof.pf(eval_W);
  proof.pf(blind_eval_W);
  const size_t num_rows = (M + W_ - 1) / W_, cols = M / num_rows;
  // (the draws of ipa.rs:139-149 happen inside the call, from the randomness stream at its current position: cols + 2 blocks)
  if (tape.pos + cols + 2 > tape.blocks) throw Error(SP_ERR_INTERNAL, "random tape exhausted");
  std::vector<uint64_t> arg(16 + 4 * cols + 8);
  ck(sp_hyrax_prove(ctx, pk.ck, pk.ck_s, tr.t, u64p(&comm_W[0].x), comm_W.size(), ps.W, M, u64p(r_W.data()), u64p(r_y.data() + 1), num_rounds_y - 1, u64p(&comm_eval_W.x),
                    u64p(&blind_eval_W), tape.bytes + 64 * tape.pos, tape.blocks - tape.pos, arg.data()),
     "PCS::prove");
  announced.done = true;  // consumed
  tape.skip(cols + 2);
  proof.words.insert(proof.words.end(), arg.begin(), arg.end());
  const double t_end = now_ms();
  if (pt) fill_phase_ms(pt->ms, t_start, t_wit, t_mv, t_outer, t_abc, t_inner, t_end);
  ps.queue_lz_tables(ctx);
  return proof;
}

// ---- prove_batch: many proofs of one key, the two sum-checks in lockstep -----------------------------------------------------------------------------
// prove_reference_order restated over `count` prepared states of ONE key, on one thread, phase by phase: every statement of src/spartan.rs:226-466 is
// run for proof 0 .. count - 1 before the next statement is begun, and the outer and the inner sum-check run as ONE lockstep sum-check each
// (sp_sumcheck_cubic3_lockstep / sp_sumcheck_quad_lockstep: a launch per round for all proofs, one wait, `count` transcripts fed on this thread).
// The openings are ONE sp_hyrax_prove_batch call (every device stage a launch for all proofs) behind the inner sum-check, or - SS_BATCH_OPENING_AHEAD -
// the same opening begun ahead: sp_hyrax_prove_batch_begin once the rest commitments are in comm_W (the mask vectors, the delta walks and the
// commitments' hashing run under the sum-checks), sp_hyrax_prove_batch_rows from the inner sum-check's hook at the round that completes
// r_y[1 ..= nvr] (L^T W and the comm_LZ walks run under its remaining rounds), sp_hyrax_prove_batch_finish where the batched call stood;
// SS_BATCH_OPENING_BEHIND keeps the one call. flags & SS_BATCH_PER_PROOF_OPENING keeps them as `count` sp_hyrax_prove calls, one after the other, and
// wins over both. evals_rx + poly_ABC and the rest
// commitments have a batched form as well (flags and defaults below). Still the per-proof calls prove_reference_order makes: the z assembly,
// sp_multiply_vec_incremental, the eval_W commitment and the lz_tables build. Proof k is word for word what
// prove(pk, *ps[k], publics[k], tapes[k]) returns and consumes the same tape blocks; every state can be proved again afterwards, alone or in a batch.
// pt (optional): the batch's wall-clock per phase, in prove's slots.
// flags & SS_BATCH_PER_PROOF_POLYABC / SS_BATCH_BATCHED_POLYABC: evals_rx + poly_ABC as one sp_eq_table_into + sp_poly_abc per proof / as ONE
// sp_poly_abc_batch call; SS_BATCH_PER_PROOF_REST_COMMIT / SS_BATCH_BATCHED_REST_COMMIT: the rest commitments one call per proof / one call for all
// (commit_zeros: one sp_fixed_base_mul_h over count x rows blinds; a non-empty rest segment: sp_hyrax_commit_batch). Same proofs either way; the flags
// are there so that one process can compare the paths, and PER_PROOF wins when both of a pair are set. With neither, the driver takes what was measured
// (profiles/prove_batch.md, config 2, one process, legs alternating): each constant is the smallest K from which the batched form is taken,
// SIZE_MAX = never (the entry point stays reachable by flag). Rule: the smallest measured K (1, 4, 16) at which the median of the batch with both forms
// batched lies below the MINIMUM of the same batch with that one form per proof.
//   poly_ABC: 3.83 ms against a minimum of 3.94 at K = 4, 10.75 against 11.03 at K = 16 (the launches: 76 us a proof against 82): BATCH_POLYABC_MIN = 4.
//   rest commitment (commit_zeros at config 2): 3.83 against 3.88 at K = 4, 10.75 against 11.20 at K = 16: BATCH_REST_COMMIT_MIN = 4.
//   the opening begun ahead, by the same rule against the same batch with SS_BATCH_OPENING_BEHIND: 3.61 ms against a minimum of 3.77 at K = 4, 9.91
//   against 10.42 at K = 16 (pcs_prove 0.61 -> 0.18 and 1.70 -> 0.45 ms; the delta walks show up in matrix_vector_multiply, +0.09 / +0.34 ms, and the
//   row stage in inner_sumcheck, +0.11 / +0.07): BATCH_OPENING_AHEAD_MIN = 4. One placement was measured: _begin once comm_W is complete, _rows at the
//   inner round that completes the row point.
//   K = 2 and 3 were not measured and keep the per-proof calls and the opening behind.
enum : unsigned {
  SS_BATCH_PER_PROOF_OPENING = 1,
  SS_BATCH_PER_PROOF_POLYABC = 2,
  SS_BATCH_BATCHED_POLYABC = 4,
  SS_BATCH_PER_PROOF_REST_COMMIT = 8,
  SS_BATCH_BATCHED_REST_COMMIT = 16,
  SS_BATCH_OPENING_AHEAD = 32,
  SS_BATCH_OPENING_BEHIND = 64
};
static constexpr size_t BATCH_POLYABC_MIN = 4;
static constexpr size_t BATCH_REST_COMMIT_MIN = 4;
static constexpr size_t BATCH_OPENING_AHEAD_MIN = 4;
// a batch opened ahead never outlives its chunk: dropped on every exit that has not handed it to sp_hyrax_prove_batch_finish
struct OpeningAhead {
  sp_ctx* ctx;
  sp_opening_job* job = nullptr;
  size_t count = 0, nvr = 0;
  std::vector<fe_t> row_pts;  // count x nvr, filled by the inner sum-check's hook
  int rc = SP_OK;
  ~OpeningAhead() {
    if (job) sp_hyrax_prove_batch_drop(ctx, job);
  }
  // sp_lockstep_hook of the inner sum-check: r_y[0] separates W from (1, X); rounds 1 .. nvr draw the opening's row variables
  static void on_inner_round(void* user, size_t round, const uint64_t* r) {
    OpeningAhead& a = *static_cast<OpeningAhead*>(user);
    if (!a.job || a.rc || round == 0 || round > a.nvr) return;
    for (size_t k = 0; k < a.count; ++k) memcpy(&a.row_pts[k * a.nvr + round - 1], r + 4 * k, sizeof(fe_t));
    if (round == a.nvr) a.rc = sp_hyrax_prove_batch_rows(a.ctx, a.job, u64p(a.row_pts.data()));
  }
};
static void prove_batch_chunk(const SpartanProverKey& pk, SpartanPrepSNARK* const* pss, size_t count, const uint64_t* publics_u64, size_t npub, Tape* tapes,
                              ProofBuf* out, size_t first, double* ms, unsigned flags) {
  const sp_dims& d = pk.dims;
  sp_ctx* ctx = pk.ctx;
  const size_t M = pk.num_vars, N = d.num_cons, W_ = DEFAULT_COMMITMENT_WIDTH;
  const size_t num_rounds_x = log2_ceil(N), num_rounds_y = log2_ceil(M) + 1;
  struct Item {
    SpartanPrepSNARK* ps = nullptr;
    Tape* tape = nullptr;
    std::unique_ptr<Tr> tr;
    std::vector<fe_t> publics, r_W_rest, r_W;
    std::vector<aff_t> comm_W;
    fe_t claims_outer[3], claims_inner[2], r;
    std::vector<fe_t> r_y;
    ProofBuf proof;
  };
  std::vector<Item> items(count);
  // every per-proof statement runs through here: an error names the proof it happened in
  auto each = [&](auto&& fn) {
    for (size_t k = 0; k < count; ++k) {
      try {
        fn(items[k], k);
      } catch (const Error& e) {
        throw Error(e.code, "prove_batch: proof " + std::to_string(first + k) + ": " + e.what());
      }
    }
  };
  double t_last = now_ms();
  auto phase = [&](int slot) {
    const double t = now_ms();
    if (ms) ms[slot] += t - t_last;
    t_last = t;
  };
  const size_t rows_rest = (d.num_rest + W_ - 1) / W_;
  const std::vector<fe_t> no_challenges;  // (prove_batch refuses circuits with verifier challenges)
  const bool batch_abc = !(flags & SS_BATCH_PER_PROOF_POLYABC) && ((flags & SS_BATCH_BATCHED_POLYABC) || count >= BATCH_POLYABC_MIN);
  const bool batch_rest = rows_rest && !(flags & SS_BATCH_PER_PROOF_REST_COMMIT) && ((flags & SS_BATCH_BATCHED_REST_COMMIT) || count >= BATCH_REST_COMMIT_MIN);
  const bool opening_ahead =
      !(flags & (SS_BATCH_PER_PROOF_OPENING | SS_BATCH_OPENING_BEHIND)) && ((flags & SS_BATCH_OPENING_AHEAD) || count >= BATCH_OPENING_AHEAD_MIN);
  // :226-236 transcript, vk, public values; r1cs_instance_and_witness (src/bellpepper/r1cs.rs:411-540)
  each([&](Item& it, size_t k) {
    it.ps = pss[k];
    it.tape = &tapes[k];
    it.publics = publics_from_u64(publics_u64 + k * npub, npub);
    it.tr.reset(new Tr(ctx, "SpartanSNARK"));
    ck(sp_transcript_set_async(it.tr->t, 1), "transcript");
    absorb_instance_prefix(*it.tr, pk.vk_digest, it.publics.data(), npub, it.ps->comm_shared_bytes, it.ps->comm_pre_bytes);
  });
  // PCS::blind (r1cs.rs:466)
  each([&](Item& it, size_t) {
    it.r_W_rest.resize(rows_rest);
    for (auto& b : it.r_W_rest) b = it.tape->next();
  });
  // commit_zeros (:467-469) or the rest commitment, and its absorb; combine_blinds (r1cs.rs:515-524)
  each([&](Item& it, size_t) {
    SpartanPrepSNARK& ps = *it.ps;
    const size_t rows_pre = ps.comm_W_fixed.size();
    it.comm_W.resize(rows_pre + rows_rest);
    std::copy(ps.comm_W_fixed.begin(), ps.comm_W_fixed.end(), it.comm_W.begin());
    if (!batch_rest) commit_rest_rows(ctx, pk.ck, ps.W, d, ps.is_small, it.r_W_rest.data(), rows_rest, it.comm_W.data() + rows_pre);
  });
  if (batch_rest && d.num_rest_unpadded == 0) {
    // commit_zeros of every proof in ONE call: the same base h and the same words per scalar, count x rows_rest blinds
    std::vector<fe_t> blinds(count * rows_rest);
    std::vector<aff_t> rows(count * rows_rest);
    for (size_t k = 0; k < count; ++k) std::copy(items[k].r_W_rest.begin(), items[k].r_W_rest.end(), blinds.begin() + k * rows_rest);
    ck(sp_fixed_base_mul_h(ctx, pk.ck, u64p(blinds.data()), blinds.size(), u64p(&rows[0].x)), "prove_batch: commit_zeros");
    for (size_t k = 0; k < count; ++k) std::copy(rows.begin() + k * rows_rest, rows.begin() + (k + 1) * rows_rest, items[k].comm_W.begin() + items[k].ps->comm_W_fixed.size());
  } else if (batch_rest) {
    std::vector<const sp_table*> Ws(count);
    std::vector<const uint64_t*> bl(count);
    std::vector<uint64_t*> outs(count);
    for (size_t k = 0; k < count; ++k) {
      Ws[k] = items[k].ps->W;
      bl[k] = u64p(items[k].r_W_rest.data());
      outs[k] = u64p(&items[k].comm_W[items[k].ps->comm_W_fixed.size()].x);
    }
    ck(sp_hyrax_commit_batch(ctx, pk.ck, count, Ws.data(), d.num_shared + d.num_precommitted, d.num_rest, bl.data(), outs.data()), "prove_batch: commit rest");
  }
  each([&](Item& it, size_t) {
    absorb_comm_W_rest(*it.tr, it.comm_W.data() + it.ps->comm_W_fixed.size(), rows_rest);
    it.r_W = combine_blinds(it.ps->r_W_fixed, it.r_W_rest);
  });
  // The opening, begun ahead: comm_W and its blinds are complete, and the IPA's randomness is the tape's blocks behind blind_eval_W's (the one draw
  // between here and PCS::prove), as prove_reference_order's announcement takes them. The pointers are checked against the tape's position when the opening comes.
  const size_t num_rows = (M + W_ - 1) / W_, cols = M / num_rows, rows_W = items[0].comm_W.size();
  std::vector<const uint64_t*> comms(count), blinds(count);
  std::vector<const sp_table*> polys(count);
  std::vector<const uint8_t*> rngs_ahead(count);
  std::vector<size_t> rng_blocks_ahead(count);
  bool ahead_fits = true;
  for (size_t k = 0; k < count; ++k) {
    Item& it = items[k];
    comms[k] = u64p(&it.comm_W[0].x);
    blinds[k] = u64p(it.r_W.data());
    polys[k] = it.ps->W;
    ahead_fits = ahead_fits && it.tape->pos + 1 + cols + 2 <= it.tape->blocks;  // (an exhausted tape is reported where prove reports it)
    rngs_ahead[k] = it.tape->bytes + 64 * (it.tape->pos + 1);
    rng_blocks_ahead[k] = ahead_fits ? it.tape->blocks - it.tape->pos - 1 : 0;
  }
  OpeningAhead ahead{ctx};
  if (opening_ahead && ahead_fits) {
    ahead.count = count;
    for (ahead.nvr = 0; ((size_t)1 << ahead.nvr) < num_rows; ++ahead.nvr) {}
    ahead.row_pts.resize(count * ahead.nvr);
    ck(sp_hyrax_prove_batch_begin(ctx, pk.ck, pk.ck_s, count, comms.data(), rows_W, polys.data(), M, blinds.data(), rngs_ahead.data(), rng_blocks_ahead.data(), &ahead.job),
       "prove_batch: PCS::prove (begin)");
  }
  phase(0);
  // :246-253 z = [W | 1 | public]
  each([&](Item& it, size_t) {
    SpartanPrepSNARK& ps = *it.ps;
    ck(sp_table_set_len(ps.z, 2 * M, (size_t)-1, (size_t)-1), "z len");
    ck(sp_table_copy(ctx, ps.z, 0, ps.W, 0, M), "z <- W");
    ck(sp_table_zero(ctx, ps.z, M, M), "clear z high half");
    const std::vector<fe_t> tail = z_tail(pk.num_extra, it.publics, no_challenges);
    // (the staged asynchronous write reuses a few pinned slots behind events; `tail` dies with this statement, so the plain write it is)
    ck(sp_table_write(ctx, ps.z, M, u64p(tail.data()), tail.size()), "z tail");
    ck(sp_table_set_len(ps.z, pk.num_cols, (size_t)-1, (size_t)-1), "z len");
  });
  // :262-264 tau
  std::vector<fe_t> taus(count * num_rounds_x);
  each([&](Item& it, size_t k) {
    for (size_t i = 0; i < num_rounds_x; ++i) taus[k * num_rounds_x + i] = it.tr->squeeze("t");
  });
  // :267-283 multiply_vec_incremental_into
  each([&](Item& it, size_t) {
    SpartanPrepSNARK& ps = *it.ps;
    ck(sp_multiply_vec_incremental(ctx, pk.S, ps.z, ps.caz, ps.cbz, ps.ccz, ps.az, ps.bz, ps.cz), "multiply_vec_incremental");
  });
  phase(1);
  each([&](Item& it, size_t) { it.proof.header(it.comm_W, it.publics, no_challenges); });
  // :291-310 outer sum-check, all proofs in lockstep
  std::vector<sp_table*> tA(count), tB(count), tC(count);
  std::vector<sp_transcript*> trs(count);
  for (size_t k = 0; k < count; ++k) {
    tA[k] = items[k].ps->az;
    tB[k] = items[k].ps->bz;
    tC[k] = items[k].ps->cz;
    trs[k] = items[k].tr->t;
  }
  std::vector<fe_t> claims(count, fe_zero()), outer_polys(count * 3 * num_rounds_x), r_x(count * num_rounds_x), outer_final(count * 3);
  ck(sp_sumcheck_cubic3_lockstep(ctx, count, u64p(claims.data()), u64p(taus.data()), num_rounds_x, tA.data(), tB.data(), tC.data(), trs.data(), u64p(outer_polys.data()),
                                 u64p(r_x.data()), u64p(outer_final.data())),
     "prove_batch: outer sum-check");
  each([&](Item& it, size_t k) {
    for (int i = 0; i < 3; ++i) it.claims_outer[i] = outer_final[3 * k + i];
    it.tr->absorb_scalars("claims_outer", it.claims_outer, 3);
    it.proof.outer(&outer_polys[k * 3 * num_rounds_x], num_rounds_x, it.claims_outer);
  });
  phase(2);
  // :311-322 r, evals_rx, bind_and_prepare_poly_ABC
  each([&](Item& it, size_t k) {
    SpartanPrepSNARK& ps = *it.ps;
    it.r = it.tr->squeeze("r");
    claims[k] = joint_inner_claim(it.claims_outer, it.r);
    if (batch_abc) return;
    ck(sp_eq_table_into(ctx, u64p(&r_x[k * num_rounds_x]), num_rounds_x, ps.rx), "evals_rx");
    ck(sp_poly_abc(ctx, pk.S, ps.rx, u64p(&it.r), 2 * M, ps.abc), "poly_ABC");
  });
  if (batch_abc) {  // one walk per chunk of proofs over their interleaved eq tables; ps.rx is not written on this path
    std::vector<fe_t> rs(count);
    std::vector<sp_table*> abcs(count);
    for (size_t k = 0; k < count; ++k) {
      rs[k] = items[k].r;
      abcs[k] = items[k].ps->abc;
    }
    ck(sp_poly_abc_batch(ctx, pk.S, count, u64p(r_x.data()), num_rounds_x, u64p(rs.data()), 2 * M, abcs.data()), "prove_batch: poly_ABC");
  }
  phase(3);
  // :323-404 inner sum-check (manual round 0 == a generic round on (lo_eff, hi_eff) = (M, num_extra) tables), all proofs in lockstep
  each([&](Item& it, size_t k) {
    SpartanPrepSNARK& ps = *it.ps;
    ck(sp_table_set_len(ps.abc, 2 * M, M, pk.num_extra), "abc len");
    ck(sp_table_set_len(ps.z, 2 * M, M, pk.num_extra), "z len");
    tA[k] = ps.abc;
    tB[k] = ps.z;
  });
  std::vector<fe_t> inner_polys(count * 2 * num_rounds_y), r_y(count * num_rounds_y), inner_final(count * 2);
  ck(sp_sumcheck_quad_lockstep_observed(ctx, count, u64p(claims.data()), num_rounds_y, tA.data(), tB.data(), trs.data(), u64p(inner_polys.data()), u64p(r_y.data()),
                                        u64p(inner_final.data()), ahead.job ? &OpeningAhead::on_inner_round : nullptr, &ahead),
     "prove_batch: inner sum-check");
  ck(ahead.rc, "prove_batch: PCS::prove (rows)");
  std::vector<fe_t> eval_W(count);
  // :405-421 eval_W
  each([&](Item& it, size_t k) {
    it.proof.inner(&inner_polys[k * 2 * num_rounds_y], num_rounds_y);
    it.r_y.assign(r_y.begin() + k * num_rounds_y, r_y.begin() + (k + 1) * num_rounds_y);
    eval_W[k] = eval_W_from(inner_final[2 * k + 1], it.r_y.data(), num_rounds_y, it.publics, no_challenges);
  });
  phase(4);
  // :423-436 blind, commit to eval_W, PCS::prove. Per proof: the blind and the commitment of eval_W (a host walk of two table
  // entries); then the openings - sp_hyrax_prove_batch_finish of the job begun ahead, or ONE sp_hyrax_prove_batch call, or with
  // SS_BATCH_PER_PROOF_OPENING one sp_hyrax_prove per proof, one after the other, over the same arguments; then the per-proof appends
  const size_t arg_words = 16 + 4 * cols + 8, npt = num_rounds_y - 1;
  std::vector<fe_t> blind_eval_W(count), points(count * npt);
  std::vector<aff_t> comm_eval_W(count);
  std::vector<const uint8_t*> rngs(count);
  std::vector<size_t> rng_blocks(count);
  each([&](Item& it, size_t k) {
    Tape& tape = *it.tape;
    blind_eval_W[k] = tape.next();
    ck(sp_hyrax_commit_small(ctx, pk.ck_s, u64p(&eval_W[k]), 1, u64p(&blind_eval_W[k]), u64p(&comm_eval_W[k].x)), "commit eval_W");
    it.proof.pf(eval_W[k]);
    it.proof.pf(blind_eval_W[k]);
    if (tape.pos + cols + 2 > tape.blocks) throw Error(SP_ERR_INTERNAL, "random tape exhausted");
    rngs[k] = tape.bytes + 64 * tape.pos;
    rng_blocks[k] = tape.blocks - tape.pos;
    if (ahead.job && rngs[k] != rngs_ahead[k]) throw Error(SP_ERR_INTERNAL, "the opening was begun on other tape blocks than PCS::prove draws");
    std::copy(it.r_y.begin() + 1, it.r_y.end(), points.begin() + k * npt);
  });
  std::vector<uint64_t> args(count * arg_words);
  if (ahead.job) {
    sp_opening_job* job = ahead.job;
    ahead.job = nullptr;  // consumed by _finish whatever it returns
    ck(sp_hyrax_prove_batch_finish(ctx, job, pk.ck, pk.ck_s, count, trs.data(), comms.data(), rows_W, polys.data(), M, blinds.data(), u64p(points.data()), npt,
                                   u64p(&comm_eval_W[0].x), u64p(blind_eval_W.data()), rngs.data(), rng_blocks.data(), args.data()),
       "prove_batch: PCS::prove (finish)");
  } else if (flags & SS_BATCH_PER_PROOF_OPENING)
    each([&](Item&, size_t k) {
      ck(sp_hyrax_prove(ctx, pk.ck, pk.ck_s, trs[k], comms[k], rows_W, polys[k], M, blinds[k], u64p(&points[k * npt]), npt, u64p(&comm_eval_W[k].x), u64p(&blind_eval_W[k]),
                        rngs[k], rng_blocks[k], &args[k * arg_words]),
         "PCS::prove");
    });
  else
    ck(sp_hyrax_prove_batch(ctx, pk.ck, pk.ck_s, count, trs.data(), comms.data(), rows_W, polys.data(), M, blinds.data(), u64p(points.data()), npt, u64p(&comm_eval_W[0].x),
                            u64p(blind_eval_W.data()), rngs.data(), rng_blocks.data(), args.data()),
       "prove_batch: PCS::prove");
  each([&](Item& it, size_t k) {
    it.tape->skip(cols + 2);
    it.proof.words.insert(it.proof.words.end(), args.begin() + k * arg_words, args.begin() + (k + 1) * arg_words);
    it.ps->queue_lz_tables(ctx);
    out[k] = std::move(it.proof);
  });
  phase(5);
}
std::vector<ProofBuf> prove_batch(const SpartanProverKey& pk, SpartanPrepSNARK* const* pss, size_t count, const uint64_t* publics_u64, size_t npub, Tape* tapes,
                                  PhaseTimes* pt, unsigned flags) {
  const sp_dims& d = pk.dims;
  if (count == 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: no states");
  if (!pss || !tapes || (npub && !publics_u64)) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: null argument");
  if (npub != d.num_public) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: public_values length");
  if (d.num_challenges > 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: circuits with verifier challenges are proved one at a time (prove)");
  for (size_t k = 0; k < count; ++k) {
    if (!pss[k]) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: null state, proof " + std::to_string(k));
    if (pss[k]->key != &pk) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: proof " + std::to_string(k) + ": the state was prepared for another key");
    for (size_t j = 0; j < k; ++j)
      if (pss[j] == pss[k]) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: the same state twice, proofs " + std::to_string(j) + " and " + std::to_string(k));
  }
  const double t_start = now_ms();
  std::vector<ProofBuf> out(count);
  if (pt) std::fill(pt->ms, pt->ms + 8, 0.0);
  if (count == 1) {
    out[0] = prove(pk, *pss[0], publics_u64, npub, tapes[0], pt);
    return out;
  }
  ck(sp_ctx_bind_thread(pk.ctx), "device");
  for (size_t first = 0; first < count; first += SP_LOCKSTEP_MAX) {  // more than SP_LOCKSTEP_MAX states: chunk by chunk
    const size_t n = std::min<size_t>(SP_LOCKSTEP_MAX, count - first);
    if (n == 1) {
      try {
        out[first] = prove_reference_order(pk, *pss[first], publics_u64 + first * npub, npub, tapes[first], nullptr, nullptr, nullptr);
      } catch (const Error& e) {
        throw Error(e.code, "prove_batch: proof " + std::to_string(first) + ": " + e.what());
      }
      continue;
    }
    prove_batch_chunk(pk, pss + first, n, publics_u64 + first * npub, npub, tapes + first, out.data() + first, first, pt ? pt->ms : nullptr, flags);
  }
  if (pt) pt->ms[6] = now_ms() - t_start;
  return out;
}

// ---- R1CSShape::is_sat (src/r1cs/mod.rs:358-394) on a prepared state ----------------------------------------------------------------------------
// z = [W | 1 | X] with the tail prove writes (z_tail; src/spartan.rs:246-253) but in a table of its own, the row check on the device (sp_shape_is_sat), then
// `res_comm` (:379): PCS::commit of the rows committed at prep_prove - shared, then precommitted - with the stored blinds and the state's is_small,
// compared with comm_W_fixed (or with `expect_comm`, the same number of rows, when the caller holds the commitment it wants checked). For circuits with
// verifier challenges the caller supplies them - its last prove's, or any: the constraints hold for every challenge - and the rest witness comes
// through the hook prove takes. Nothing a later prove reads is written: W, the cached products, the working tables and the randomness tape are left alone.
// Returns true when both checks hold; *reason = the reference's reason string otherwise ("R1CS is unsatisfiable" first, :381-391).
bool is_sat(const SpartanProverKey& pk, SpartanPrepSNARK& ps, const uint64_t* publics_u64, size_t npub, const uint64_t* challenges, ss_rest_hook synth, void* synth_user,
            const uint64_t* expect_comm, sp_sat_report* report, std::vector<uint64_t>* bad_rows, const char** reason) {
  const sp_dims& d = pk.dims;
  sp_ctx* ctx = pk.ctx;
  const size_t M = pk.num_vars, fixed = d.num_shared + d.num_precommitted;
  if (npub != d.num_public) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "public_values length");
  if (d.num_challenges && (!challenges || !synth)) throw Error(SP_ERR_INTERNAL, "a circuit with verifier challenges needs its challenges and its synthesize callback");
  ck(sp_ctx_bind_thread(ctx), "device");
  if (!ps.sat_z) ck(sp_table_zeros(ctx, pk.num_cols, (size_t)-1, (size_t)-1, &ps.sat_z), "alloc z (is_sat)");
  ck(sp_table_copy(ctx, ps.sat_z, 0, ps.W, 0, M), "z <- W");
  std::vector<fe_t> ch(d.num_challenges);
  if (d.num_challenges) memcpy(ch.data(), challenges, d.num_challenges * sizeof(fe_t));
  if (d.num_challenges) {  // circuit.synthesize(.., Some(&challenges)) (bellpepper/r1cs.rs:443-461); the rest segment goes into z, not into W
    const std::vector<fe_t> rest = synthesize_rest(synth, synth_user, challenges, d.num_challenges, d.num_rest_unpadded);
    if (d.num_rest_unpadded) ck(sp_table_write(ctx, ps.sat_z, fixed, u64p(rest.data()), d.num_rest_unpadded), "z rest");
  }
  const std::vector<fe_t> tail = z_tail(pk.num_extra, publics_from_u64(publics_u64, npub), ch);
  ck(sp_table_write(ctx, ps.sat_z, M, u64p(tail.data()), tail.size()), "z tail");
  ck(sp_shape_is_sat(ctx, pk.S, ps.sat_z, nullptr, nullptr, report), "shape_is_sat");
  // res_comm
  const size_t rows = ps.comm_W_fixed.size();
  std::vector<aff_t> again(rows);
  if (ps.rows_shared) ck(sp_hyrax_commit(ctx, pk.ck, ps.W, 0, d.num_shared, u64p(ps.r_W_fixed.data()), ps.is_small ? 1 : 0, u64p(&again[0].x)), "commit shared (is_sat)");
  if (ps.rows_precommitted)
    ck(sp_hyrax_commit(ctx, pk.ck, ps.W, d.num_shared, d.num_precommitted, u64p(ps.r_W_fixed.data() + ps.rows_shared), ps.is_small ? 1 : 0, u64p(&again[ps.rows_shared].x)),
       "commit precommitted (is_sat)");
  const aff_t* want = expect_comm ? reinterpret_cast<const aff_t*>(expect_comm) : ps.comm_W_fixed.data();
  bad_rows->clear();
  for (size_t i = 0; i < rows; ++i)
    if (memcmp(&again[i], &want[i], sizeof(aff_t)) != 0) bad_rows->push_back(i);
  *reason = report->num_failing ? "R1CS is unsatisfiable" : (!bad_rows->empty() ? "Invalid commitment" : nullptr);
  return *reason == nullptr;
}

// ---- SpartanSNARK::verify (src/spartan.rs:469-578) — SURVEY 8(f) rank 3 ---------------------------------------------------------------
// The work that scales with the instance runs on the device through the same ABI: the three matrix evaluations A(rx,ry), B, C
// (`evaluate_with_tables_fast`, src/r1cs/mod.rs:1216-1226) as ONE sp_multiply_vec against the table T_y = eq(r_y) followed by three dot
// products with T_x = eq(r_x); comm_LZ = <L, comm rows> (hyrax_pc.rs:480-531) and the IPA check's <z_vec, ck> (ipa.rs:173-221) as device MSMs.
// The O(log N) parts (transcript, round-polynomial checks, single scalar multiplications) stay on the host. Returns 0 = accept, else the index
// of the failed check (1 shape, 2 outer sum-check, 3 outer claim, 4 inner sum-check, 5 inner claim, 6 opening) — the oracle's codes.
//
// The function is three steps, which verify() runs on one proof and verify_batch() on many:
//   (a) verify_step_a    parse, canonicity and on-curve checks, transcript, both sum-check verifications, eval_Z: checks 1-4 (host only)
//   (b) verify_step_b    the three matrix evaluations and check 5 (single proof); check5() is the comparison both forms share
//   (c) opening_prepare_host, opening_comm_LZ, opening_challenge  the opening up to the IPA's challenge r: R and <z_vec, R> (can fail check 6), comm_LZ, comm_eval_W
//       opening_check    the two group equations of InnerProductArgumentLinear::verify for ONE proof: check 6

struct VerifyState {  // one proof between the steps
  // views into the caller's words
  const aff_t* comm_W = nullptr;
  const fe_t *publics = nullptr, *z_vec = nullptr;
  fe_t eval_W, blind_eval_W, z_delta, z_beta;
  aff_t delta, beta;
  size_t rows = 0, lx = 0, ly = 0, nz = 0;
  // step (a)
  ZJob zjob;
  std::unique_ptr<Tr> tr;
  std::vector<fe_t> r_x, r_y;
  fe_t r, r2, claim_inner_final, eval_Z;
  // opening_prepare
  aff_t comm_LZ, comm_eval_W;
  std::vector<fe_t> L;  // eq(point[..nvr]); empty for a single-row polynomial (comm_LZ = comm_W[0])
  fe_t rr, ip;  // the IPA challenge and <z_vec, R>
};

// step (a). start_z: begin <z_vec, ck> on the auxiliary stream as soon as the proof has parsed (the single-proof form; a batch folds all z_vec into one MSM)
static int verify_step_a(const SpartanProverKey& pk, const uint64_t* words, size_t nwords, bool start_z, VerifyState& st) {
  sp_ctx* ctx = pk.ctx;
  const sp_dims& d = pk.dims;
  const SpartanLayout& lay = pk.layout;
  const size_t rows_sh = lay.rows_shared, rows_pre = lay.rows_precommitted, rows_rest = lay.rows_rest, rows = lay.rows(), lx = lay.rounds_x, ly = lay.rounds_y, nz = lay.z_len;
  if (nwords != lay.words() || !well_formed(lay, words)) return 1;
  const SpartanProofView pv = lay.view(words);
  const aff_t* comm_W = pv.comm_W;
  const fe_t *publics = pv.publics, *challenges = pv.challenges, *outer = pv.outer, *claims = pv.claims, *inner = pv.inner, *z_vec = pv.z_vec;
  st.comm_W = comm_W;
  st.publics = publics;
  st.z_vec = z_vec;
  st.eval_W = *pv.eval_W;
  st.blind_eval_W = *pv.blind_eval_W;
  st.z_delta = *pv.z_delta;
  st.z_beta = *pv.z_beta;
  st.delta = *pv.delta;
  st.beta = *pv.beta;
  st.rows = rows;
  st.lx = lx;
  st.ly = ly;
  st.nz = nz;

  st.zjob.ctx = ctx;
  st.zjob.key = pk.ck;
  if (start_z) ck(sp_msm_ck_begin(ctx, pk.ck, u64p(z_vec), nz, &st.zjob.job), "<z, ck> (begin)");

  st.tr.reset(new Tr(ctx, "SpartanSNARK"));
  Tr& tr = *st.tr;
  tr.absorb("vk", pk.vk_digest, 32);
  tr.absorb_scalars("public_values", publics, d.num_public);
  auto absorb_rows = [&](const char* label, size_t lo, size_t cnt) {
    std::vector<uint8_t> b = commitment_bytes(comm_W + lo, cnt);
    tr.absorb(label, b.data(), b.size());
  };
  if (rows_sh) absorb_rows("comm_W_shared", 0, rows_sh);
  if (rows_pre) absorb_rows("comm_W_precommitted", rows_sh, rows_pre);
  for (size_t i = 0; i < d.num_challenges; ++i)  // validate (src/r1cs/mod.rs:1516-1526): the instance's challenges must be the transcript's
    if (!fe_eq(tr.squeeze("challenge"), challenges[i])) return 1;
  absorb_rows("comm_W_rest", rows_sh + rows_pre, rows_rest);
  std::vector<fe_t> tau(lx);
  for (auto& t : tau) t = tr.squeeze("t");
  fe_t claim_outer_final;
  std::vector<fe_t>&r_x = st.r_x, &r_y = st.r_y;
  if (!sumcheck_verify(tr, fe_zero(), lx, 3, outer, &claim_outer_final, &r_x)) return 2;
  const fe_t one = fe_one<S>();
  fe_t taus_bound_rx = one;  // EqPolynomial::evaluate (src/polys/eq.rs:45-57)
  for (size_t i = 0; i < lx; ++i)
    taus_bound_rx = fe_mul<S>(taus_bound_rx, fe_add<S>(fe_mul<S>(tau[i], r_x[i]), fe_mul<S>(fe_sub<S>(one, tau[i]), fe_sub<S>(one, r_x[i]))));
  if (!fe_eq(claim_outer_final, fe_mul<S>(taus_bound_rx, fe_sub<S>(fe_mul<S>(claims[0], claims[1]), claims[2])))) return 3;
  tr.absorb_scalars("claims_outer", claims, 3);
  const fe_t r = tr.squeeze("r"), r2 = fe_mul<S>(r, r);
  const fe_t claim_inner_joint = fe_add<S>(fe_add<S>(claims[0], fe_mul<S>(r, claims[1])), fe_mul<S>(r2, claims[2]));
  if (!sumcheck_verify(tr, claim_inner_joint, ly, 2, inner, &st.claim_inner_final, &r_y)) return 4;
  std::vector<fe_t> X(1 + d.num_public + d.num_challenges);
  X[0] = one;
  std::copy(publics, publics + d.num_public + d.num_challenges, X.begin() + 1);  // challenges follow the public values in the buffer and in X
  const fe_t eval_X = sparse_poly_evaluate(ly - 1, X, r_y.data() + 1);
  st.eval_Z = fe_add<S>(fe_mul<S>(fe_sub<S>(one, r_y[0]), st.eval_W), fe_mul<S>(r_y[0], eval_X));
  st.r = r;
  st.r2 = r2;
  return 0;
}

// check 5 given A(rx,ry), B(rx,ry), C(rx,ry)
static bool check5(const VerifyState& st, const fe_t eabc[3]) {
  return fe_eq(st.claim_inner_final, fe_mul<S>(fe_add<S>(fe_add<S>(eabc[0], fe_mul<S>(st.r, eabc[1])), fe_mul<S>(st.r2, eabc[2])), st.eval_Z));
}

// step (b), single proof: A(rx,ry), B(rx,ry), C(rx,ry) = T_x^T (M T_y): one SpMV against T_y, three dot products with T_x
static int verify_step_b(const SpartanProverKey& pk, const VerifyState& st) {
  sp_ctx* ctx = pk.ctx;
  const size_t N = pk.dims.num_cons, lx = st.lx, ly = st.ly;
  fe_t eabc[3];
  {
    if (!pk.v_Tx) {
      ck(sp_table_zeros(ctx, (size_t)1 << lx, (size_t)-1, (size_t)-1, &pk.v_Tx), "T_x alloc");
      ck(sp_table_zeros(ctx, (size_t)1 << ly, (size_t)-1, (size_t)-1, &pk.v_Ty), "T_y alloc");
      for (int i = 0; i < 3; ++i) ck(sp_table_zeros(ctx, N, (size_t)-1, (size_t)-1, &pk.v_mv[i]), "M T_y alloc");
    }
    sp_table *Tx = pk.v_Tx, *Ty = pk.v_Ty, **mv = pk.v_mv;
    ck(sp_table_set_len(Tx, (size_t)1 << lx, (size_t)-1, (size_t)-1), "T_x len");
    ck(sp_table_set_len(Ty, (size_t)1 << ly, (size_t)-1, (size_t)-1), "T_y len");
    ck(sp_eq_table_into(ctx, u64p(st.r_x.data()), lx, Tx), "T_x");
    ck(sp_eq_table_into(ctx, u64p(st.r_y.data()), ly, Ty), "T_y");
    ck(sp_table_set_len(Ty, pk.num_cols, (size_t)-1, (size_t)-1), "T_y as z");
    ck(sp_multiply_vec(ctx, pk.S, Ty, mv[0], mv[1], mv[2]), "M T_y");
    for (int i = 0; i < 3; ++i) ck(sp_table_dot(ctx, Tx, mv[i], N, u64p(&eabc[i])), "T_x . (M T_y)");
  }
  return check5(st, eabc) ? 0 : 5;
}

// step (c), transcript part. HyraxPCS::verify (hyrax_pc.rs:480-531) + InnerProductArgumentLinear::verify (ipa.rs:173-221) up to the challenge r:
// comm_eval_W and comm_LZ are absorbed before r is drawn, so both exist per proof in a batch as well. Two halves: opening_prepare_host touches the
// proof's own transcript and host memory only (a batch runs it on host threads); opening_comm_LZ and opening_challenge make the device calls and draw r.
static int opening_prepare_host(VerifyState& st) {
  Tr& tr = *st.tr;
  {
    std::vector<uint8_t> b = commitment_bytes(st.comm_W, st.rows);
    tr.absorb("poly_com", b.data(), b.size());
  }
  const fe_t* point = st.r_y.data() + 1;
  const size_t npoint = st.ly - 1, nz = st.nz, num_rows = ((size_t)1 << npoint) / nz, nvr = log2_ceil(num_rows);
  std::vector<fe_t> R;
  if (nvr == 0) {
    st.L.clear();
    R = eq_evals_host(point, npoint);
  } else {
    st.L = eq_evals_host(point, nvr);
    R = eq_evals_host(point + nvr, npoint - nvr);
    if (st.rows < st.L.size()) return 6;
  }
  if (R.size() != nz) return 6;
  fe_t ip = fe_zero();
  for (size_t i = 0; i < nz; ++i) ip = fe_add<S>(ip, fe_mul<S>(st.z_vec[i], R[i]));
  st.ip = ip;
  return 0;
}
// comm_LZ = <L, comm rows> (hyrax_pc.rs:497-506) on the main stream
static void opening_comm_LZ(const SpartanProverKey& pk, VerifyState& st) {
  if (st.L.empty()) st.comm_LZ = st.comm_W[0];
  else ck(sp_msm(pk.ctx, u64p(st.L.data()), reinterpret_cast<const uint64_t*>(st.comm_W), st.L.size(), u64p(&st.comm_LZ.x)), "comm_LZ");
}
// comm_eval_W, then the IPA's transcript steps up to its challenge (ipa.rs:181-194)
static void opening_challenge(const SpartanProverKey& pk, VerifyState& st) {
  Tr& tr = *st.tr;
  ck(sp_hyrax_commit_small(pk.ctx, pk.ck_s, u64p(&st.eval_W), 1, u64p(&st.blind_eval_W), u64p(&st.comm_eval_W.x)), "commit eval_W");
  tr.dom_sep("inner product argument (linear)");
  {
    uint8_t b[128];
    point_bytes(st.comm_LZ, b);
    point_bytes(st.comm_eval_W, b + 64);
    tr.absorb("U", b, 128);
    point_bytes(st.delta, b);
    tr.absorb("delta", b, 64);
    point_bytes(st.beta, b);
    tr.absorb("beta", b, 64);
  }
  st.rr = tr.squeeze("r");
}

// step (c), the group equations of one proof (ipa.rs:196-221)
static int opening_check(const SpartanProverKey& pk, VerifyState& st) {
  sp_ctx* ctx = pk.ctx;
  // r * comm_LZ and r * comm_eval_W: one wNAF scalar per pair of points (vartime_scalar_mul, msm.rs:779-867); h * z_delta and
  // <z_vec, R> * ck_c + z_beta * h_c through the fixed-base tables of the keys (hyrax_pc.rs:81-96)
  aff_t pr2[2] = {st.comm_LZ, st.comm_eval_W}, rp[2], hzd, rhs2;
  ck(sp_vartime_scalar_mul(ctx, u64p(&pr2[0].x), 2, u64p(&st.rr), u64p(&rp[0].x)), "r * (comm_LZ, comm_eval_W)");
  ck(sp_fixed_base_mul_h(ctx, pk.ck, u64p(&st.z_delta), 1, u64p(&hzd.x)), "h * z_delta");
  ck(sp_hyrax_commit_small(ctx, pk.ck_s, u64p(&st.ip), 1, u64p(&st.z_beta), u64p(&rhs2.x)), "<z, R> * ck_c + z_beta * h_c");
  aff_t zc;  // <z_vec, ck>: verify() started it before the transcript work
  {
    if (!st.zjob.job) ck(sp_msm_ck_begin(ctx, pk.ck, u64p(st.z_vec), st.nz, &st.zjob.job), "<z, ck> (begin)");
    sp_msm_job* j = st.zjob.job;
    st.zjob.job = nullptr;
    ck(sp_msm_ck_finish(ctx, pk.ck, j, nullptr, u64p(&zc.x)), "<z, ck> (finish)");
  }
  const jac_t lhs1 = jac_add_mixed(jac_from_affine(rp[0]), st.delta), rhs1 = jac_add_mixed(jac_from_affine(zc), hzd);
  if (!same_point(lhs1, rhs1)) return 6;
  const jac_t lhs2 = jac_add_mixed(jac_from_affine(rp[1]), st.beta);
  if (!same_point(lhs2, jac_from_affine(rhs2))) return 6;
  return 0;
}

int verify(const SpartanProverKey& pk, const uint64_t* words, size_t nwords, uint64_t* out_publics) {
  VerifyState st;
  int code;
  if ((code = verify_step_a(pk, words, nwords, true, st))) return code;
  if ((code = verify_step_b(pk, st))) return code;
  if ((code = opening_prepare_host(st))) return code;
  opening_comm_LZ(pk, st);
  opening_challenge(pk, st);
  if ((code = opening_check(pk, st))) return code;
  if (out_publics) memcpy(out_publics, st.publics, pk.dims.num_public * sizeof(fe_t));  // verify() returns the public values it accepted (src/spartan.rs:577)
  return 0;
}

// ---- verify_batch: `count` proofs under one key in one pass ---------------------------------------------------------
// codes[k] == verify(proof k) for every k; a batch of one IS verify; from two proofs on, what the proofs share is paid once:
//   step (a) and the host part of the opening per proof on host threads (they touch no device state);
//   step (b) per chunk of sp_shape_matrix_evals_chunk() survivors: the chunk's eq tables and ONE sp_shape_matrix_evals_batched (no product tables); check 5 is exact;
//   step (c) comm_LZ_k per proof on the auxiliary stream under step (b), the IPA challenge r_k per proof, then the group equations of all survivors as one random linear combination
//       sum_k rho_k (r_k comm_LZ_k + delta_k)  ==  < sum_k rho_k z_vec_k, ck >  +  (sum_k rho_k z_delta_k) h
//       sum_k rho'_k beta_k  ==  (sum_k rho'_k (<z_vec_k, R_k> - r_k eval_W_k)) ck_c  +  (sum_k rho'_k (z_beta_k - r_k blind_eval_W_k)) h_c
//     (comm_LZ_k = sum_i L_k[i] comm_W_k[i] is formed per proof all the same: its bytes go into the transcript r_k is drawn from, so the left side of the
//     first equation is an MSM over the 2 K points comm_LZ_k, delta_k rather than over the K (rows + 1) rows).
//     If either equation fails, opening_check names the proofs with code 6 one by one.
// The weights come from the library's Keccak transcript over everything the batch holds (batch_weights), so a prover who fixes the proofs first cannot
// aim at them: a false accept needs a guessed 256-bit challenge.
// rho_k = w[2 k], rho'_k = w[2 k + 1]. Transcript "SpartanSNARK::verify_batch": absorb "vk" (digest), "count" (K, 8 bytes LE), then per proof in batch
// order "proof_len" (words, 8 bytes LE) and "proof" (the words as they are, LE), then "seed" (32 bytes) if the caller gave one; squeeze "rho" 2 K times.
static std::vector<fe_t> batch_weights(const SpartanProverKey& pk, const uint64_t* const* words, const size_t* nwords, size_t count, const uint8_t* seed) {
  Tr tr(pk.ctx, "SpartanSNARK::verify_batch");
  tr.absorb("vk", pk.vk_digest, 32);
  auto le8 = [](uint64_t v, uint8_t b[8]) {
    for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(v >> (8 * i));
  };
  uint8_t b8[8];
  le8(count, b8);
  tr.absorb("count", b8, 8);
  for (size_t k = 0; k < count; ++k) {
    le8(nwords[k], b8);
    tr.absorb("proof_len", b8, 8);
    tr.absorb("proof", reinterpret_cast<const uint8_t*>(words[k]), nwords[k] * 8);
  }
  if (seed) tr.absorb("seed", seed, 32);
  std::vector<fe_t> w(2 * count);
  for (auto& x : w) x = tr.squeeze("rho");
  return w;
}

void verify_batch(const SpartanProverKey& pk, const uint64_t* const* words, const size_t* nwords, size_t count, const uint8_t* seed, int* codes,
                  uint64_t* out_publics, ss_verify_batch_info* info) {
  sp_ctx* ctx = pk.ctx;
  ss_verify_batch_info inf{0, 1, 0, 0};
  if (info) *info = inf;
  if (count == 0) return;
  ck(sp_ctx_bind_thread(ctx), "device");  // the caller may be a thread other than the one that created the context
  const size_t npub = pk.dims.num_public;
  if (count == 1) {  // nothing to share: the single-proof form, which starts <z_vec, ck> under its transcript work (no chunk, no combined equations)
    codes[0] = verify(pk, words[0], nwords[0], out_publics);
    return;
  }
  const size_t KC = sp_shape_matrix_evals_chunk();  // pairs per launch: the device memory of a batch is this many (T_x, T_y) pairs
  // the weights need the proofs alone: hashed on a thread of their own under steps (a) and (b)
  std::future<std::vector<fe_t>> weights = std::async(std::launch::async, [&] { return batch_weights(pk, words, nwords, count, seed); });
  struct Join {
    std::future<std::vector<fe_t>>& f;
    ~Join() {
      if (f.valid()) f.wait();
    }
  } join{weights};
  std::vector<VerifyState> st(count);
  std::vector<int> host6(count, 0);  // what the opening's host part says (0 or 6): counts only for a proof that passes check 5
  parallel_for(count, (size_t)1 << 20, [&](size_t k) {
    if ((codes[k] = verify_step_a(pk, words[k], nwords[k], false, st[k])) == 0) host6[k] = opening_prepare_host(st[k]);
  });
  std::vector<size_t> live;
  for (size_t k = 0; k < count; ++k)
    if (codes[k] == 0) live.push_back(k);
  // comm_LZ_k needs r_y alone: a helper thread runs these MSMs on the auxiliary stream (sp_msm_eq_begin: sum_i eq(r, i) comm_W[i], the same group element)
  // under the matrix evaluations of step (b) on the main stream. A proof that then fails check 5 has had its comm_LZ formed for nothing (an upload and
  // one MSM beside the main stream's work): waiting for check 5 instead would put every MSM behind the matrix evaluations again.
  const std::vector<size_t> after_a = live;
  std::future<void> lz = std::async(std::launch::async, [&] {
    ck(sp_ctx_bind_thread(ctx), "helper thread: device");  // a new thread starts on device 0; the context may live on another GPU
    struct Pts {
      sp_points* p = nullptr;
      ~Pts() { sp_points_free(p); }
    } pts;
    for (size_t k : after_a) {
      VerifyState& s = st[k];
      if (host6[k]) continue;
      if (s.L.empty()) {
        s.comm_LZ = s.comm_W[0];
        continue;
      }
      sp_msm_job* job = nullptr;
      ck(sp_points_upload(ctx, reinterpret_cast<const uint64_t*>(s.comm_W), s.L.size(), &pts.p), "comm_W upload");
      ck(sp_msm_eq_begin(ctx, pts.p, u64p(s.r_y.data() + 1), log2_ceil(s.L.size()), &job), "comm_LZ (begin)");
      ck(sp_msm_job_finish(ctx, job, u64p(&s.comm_LZ.x)), "comm_LZ (finish)");
    }
  });
  struct JoinLz {
    std::future<void>& f;
    ~JoinLz() {
      if (f.valid()) f.wait();
    }
  } join_lz{lz};
  // step (b)
  if (!live.empty()) {
    const size_t lx = st[live[0]].lx, ly = st[live[0]].ly;
    if (pk.vb_Tx.empty()) {
      for (size_t j = 0; j < KC; ++j) {
        sp_table *tx = nullptr, *ty = nullptr;
        ck(sp_table_zeros(ctx, (size_t)1 << lx, (size_t)-1, (size_t)-1, &tx), "T_x alloc");
        pk.vb_Tx.push_back(tx);
        ck(sp_table_zeros(ctx, (size_t)1 << ly, (size_t)-1, (size_t)-1, &ty), "T_y alloc");
        pk.vb_Ty.push_back(ty);
      }
    }
    std::vector<size_t> next;
    for (size_t c0 = 0; c0 < live.size(); c0 += KC) {
      const size_t kc = std::min(KC, live.size() - c0);
      std::vector<fe_t> eabc(3 * kc);
      for (size_t j = 0; j < kc; ++j) {
        const VerifyState& s = st[live[c0 + j]];
        ck(sp_eq_table_into(ctx, u64p(s.r_x.data()), lx, pk.vb_Tx[j]), "T_x");
        ck(sp_eq_table_into(ctx, u64p(s.r_y.data()), ly, pk.vb_Ty[j]), "T_y");
      }
      ck(sp_shape_matrix_evals_batched(ctx, pk.S, pk.vb_Tx.data(), pk.vb_Ty.data(), kc, u64p(eabc.data())), "matrix_evals_batched");
      inf.matrix_chunks++;
      for (size_t j = 0; j < kc; ++j) {
        const size_t k = live[c0 + j];
        if (check5(st[k], eabc.data() + 3 * j)) next.push_back(k);
        else codes[k] = 5;
      }
    }
    live.swap(next);
  }
  // step (c): the challenge of every proof that is left
  lz.get();
  {
    std::vector<size_t> next;
    for (size_t k : live)
      if ((codes[k] = host6[k]) == 0) {
        opening_challenge(pk, st[k]);
        next.push_back(k);
      }
    live.swap(next);
  }
  const std::vector<fe_t> w = weights.get();
  if (!live.empty()) {
    const size_t nz = st[live[0]].nz, n = live.size();
    inf.opening_proofs = n;
    std::vector<fe_t> zsum(nz, fe_zero()), s1(2 * n), s2(n);
    std::vector<aff_t> p1(2 * n), p2(n);
    fe_t zd = fe_zero(), c2 = fe_zero(), b2 = fe_zero();
    for (size_t i = 0; i < n; ++i) {
      const VerifyState& s = st[live[i]];
      const fe_t rho = w[2 * live[i]], rho2 = w[2 * live[i] + 1];
      zd = fe_add<S>(zd, fe_mul<S>(rho, s.z_delta));
      p1[2 * i] = s.comm_LZ;
      s1[2 * i] = fe_mul<S>(rho, s.rr);
      p1[2 * i + 1] = s.delta;
      s1[2 * i + 1] = rho;
      p2[i] = s.beta;
      s2[i] = rho2;
      c2 = fe_add<S>(c2, fe_mul<S>(rho2, fe_sub<S>(s.ip, fe_mul<S>(s.rr, s.eval_W))));
      b2 = fe_add<S>(b2, fe_mul<S>(rho2, fe_sub<S>(s.z_beta, fe_mul<S>(s.rr, s.blind_eval_W))));
    }
    parallel_for(8, (size_t)1 << 20, [&](size_t part) {  // sum_k rho_k z_vec_k, a column range per thread
      for (size_t j = part * nz / 8, e = (part + 1) * nz / 8; j < e; ++j)
        for (size_t i = 0; i < n; ++i) zsum[j] = fe_add<S>(zsum[j], fe_mul<S>(w[2 * live[i]], st[live[i]].z_vec[j]));
    });
    ZJob zj;
    zj.ctx = ctx;
    zj.key = pk.ck;
    ck(sp_msm_ck_begin(ctx, pk.ck, u64p(zsum.data()), nz, &zj.job), "<sum rho z, ck> (begin)");
    aff_t lhs1, lhs2, rhs1, rhs2;
    ck(sp_msm(ctx, u64p(s1.data()), u64p(&p1[0].x), 2 * n, u64p(&lhs1.x)), "sum rho (r comm_LZ + delta)");
    ck(sp_msm(ctx, u64p(s2.data()), u64p(&p2[0].x), n, u64p(&lhs2.x)), "sum rho' beta");
    ck(sp_hyrax_commit_small(ctx, pk.ck_s, u64p(&c2), 1, u64p(&b2), u64p(&rhs2.x)), "combined right side of the second equation");
    {
      sp_msm_job* j = zj.job;
      zj.job = nullptr;
      ck(sp_msm_ck_finish(ctx, pk.ck, j, u64p(&zd), u64p(&rhs1.x)), "<sum rho z, ck> (finish)");
    }
    const bool ok = same_point(jac_from_affine(lhs1), jac_from_affine(rhs1)) && same_point(jac_from_affine(lhs2), jac_from_affine(rhs2));
    inf.opening_batched_ok = ok ? 1 : 0;
    if (!ok) {
      for (size_t k : live) codes[k] = opening_check(pk, st[k]);
      inf.fallback_proofs = n;
    }
  }
  if (out_publics)
    for (size_t k = 0; k < count; ++k)
      if (codes[k] == 0) memcpy(out_publics + 4 * npub * k, st[k].publics, npub * sizeof(fe_t));
  if (info) *info = inf;
}

}  // namespace spartan2

// ---- C surface for the harness (tests, bench.py) -----------------------------------------------------------------------------
using namespace spartan2;
static thread_local std::string g_err;
static int catch_all() {
  try {
    throw;
  } catch (const Error& e) {
    g_err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_err = e.what();
    return SP_ERR_INTERNAL;
  }
}

// the prover entry points take the key through this: a key loaded from its bytes holds none of the prover's structures
static SpartanProverKey& prover_key(void* pk, const char* who) {
  auto* k = (SpartanProverKey*)pk;
  if (k && k->verifier_only) throw Error(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": verifier-only key (loaded by ss_verifier_from_bytes; proving takes the key of ss_setup)");
  return *k;
}

extern "C" {
const char* ss_last_error() { return g_err.c_str(); }
void ss_set_error(const char* msg) { g_err = msg; }

// SplitR1CSShape::new for callers that drive the sparse kernels directly. Returns an opaque PaddedShape.
int ss_pad_shape(size_t num_cons, size_t num_shared, size_t num_precommitted, size_t num_rest, size_t num_public, size_t num_challenges, const int64_t* Ad,
                 const uint32_t* Ai, const uint64_t* Ap, const int64_t* Bd, const uint32_t* Bi, const uint64_t* Bp, const int64_t* Cd, const uint32_t* Ci,
                 const uint64_t* Cp, void** out) {
  try {
    *out = new PaddedShape(pad_shape(make_view(num_cons, num_shared, num_precommitted, num_rest, num_public, num_challenges, Ad, Ai, Ap, Bd, Bi, Bp, Cd, Ci, Cp)));
    return 0;
  } catch (...) {
    return catch_all();
  }
}
void ss_padded_free(void* p) { delete (PaddedShape*)p; }
void ss_padded_equalize(void* a, void* b) { equalize(*(PaddedShape*)a, *(PaddedShape*)b); }  // SplitR1CSShape::equalize (src/r1cs/mod.rs:913-971)
void ss_padded_dims(void* p, uint64_t out[10]) { memcpy(out, &((PaddedShape*)p)->dims, sizeof(sp_dims)); }
void ss_padded_csr(void* p, int which, const uint64_t** data, const uint32_t** idx, const uint64_t** ptr, uint64_t* nnz) {
  auto* P = (PaddedShape*)p;
  *data = u64p(P->data[which].data());
  *idx = P->idx[which].data();
  *ptr = P->ptr[which].data();
  *nnz = P->data[which].size();
}
int ss_from_label(const char* label, size_t n, uint64_t* out) {
  try {
    std::vector<aff_t> g = from_label(label, n);
    memcpy(out, g.data(), n * sizeof(aff_t));
    return 0;
  } catch (...) {
    return catch_all();
  }
}

int ss_setup(sp_ctx* ctx, size_t num_cons, size_t num_shared, size_t num_precommitted, size_t num_rest, size_t num_public, size_t num_challenges,
             const int64_t* Ad, const uint32_t* Ai, const uint64_t* Ap, const int64_t* Bd, const uint32_t* Bi, const uint64_t* Bp, const int64_t* Cd,
             const uint32_t* Ci, const uint64_t* Cp, void** out_pk) {
  try {
    *out_pk = setup(ctx, make_view(num_cons, num_shared, num_precommitted, num_rest, num_public, num_challenges, Ad, Ai, Ap, Bd, Bi, Bp, Cd, Ci, Cp));
    return 0;
  } catch (...) {
    return catch_all();
  }
}
void ss_pk_free(void* pk) { delete (SpartanProverKey*)pk; }
// The key's SpartanVerifierKey as bincode bytes (see vk_to_bytes): the circuit arguments of ss_setup again. Two passes: out == NULL returns the length,
// otherwise the bytes are written (cap must hold them) and the length returned; < 0 = error (ss_last_error), among them a circuit other than the key's.
long ss_vk_to_bytes(void* pk, size_t num_cons, size_t num_shared, size_t num_precommitted, size_t num_rest, size_t num_public, size_t num_challenges, const int64_t* Ad,
                    const uint32_t* Ai, const uint64_t* Ap, const int64_t* Bd, const uint32_t* Bi, const uint64_t* Bp, const int64_t* Cd, const uint32_t* Ci,
                    const uint64_t* Cp, uint8_t* out, size_t cap) {
  try {
    if (!pk) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "ss_vk_to_bytes: null key");
    const R1CSIntView R = make_view(num_cons, num_shared, num_precommitted, num_rest, num_public, num_challenges, Ad, Ai, Ap, Bd, Bi, Bp, Cd, Ci, Cp);
    const SpartanProverKey& key = prover_key(pk, "ss_vk_to_bytes");
    if (key.from_bytes) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "ss_vk_to_bytes: a key loaded from its bytes (keep those)");
    if (!out) return (long)vk_bytes_len(key, R);
    const std::vector<uint8_t> b = vk_to_bytes(key, R);
    if (cap < b.size()) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "ss_vk_to_bytes: buffer too small");
    memcpy(out, b.data(), b.size());
    return (long)b.size();
  } catch (...) {
    return catch_all();
  }
}
// The key's SpartanProverKey { ck, ck_s, S, vk_digest } as bincode bytes: ss_vk_to_bytes's protocol and bytes, followed by the 32 digest bytes.
long ss_pk_to_bytes(void* pk, size_t num_cons, size_t num_shared, size_t num_precommitted, size_t num_rest, size_t num_public, size_t num_challenges, const int64_t* Ad,
                    const uint32_t* Ai, const uint64_t* Ap, const int64_t* Bd, const uint32_t* Bi, const uint64_t* Bp, const int64_t* Cd, const uint32_t* Ci,
                    const uint64_t* Cp, uint8_t* out, size_t cap) {
  try {
    if (!pk) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "ss_pk_to_bytes: null key");
    const R1CSIntView R = make_view(num_cons, num_shared, num_precommitted, num_rest, num_public, num_challenges, Ad, Ai, Ap, Bd, Bi, Bp, Cd, Ci, Cp);
    const SpartanProverKey& key = prover_key(pk, "ss_pk_to_bytes");
    if (key.from_bytes) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "ss_pk_to_bytes: a key loaded from its bytes (keep those)");
    if (!out) return (long)vk_bytes_len(key, R) + 32;
    const std::vector<uint8_t> b = pk_to_bytes(key, R);
    if (cap < b.size()) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "ss_pk_to_bytes: buffer too small");
    memcpy(out, b.data(), b.size());
    return (long)b.size();
  } catch (...) {
    return catch_all();
  }
}
// A prover's key from those bytes (see key_from_bytes): no circuit, no setup. flags: SP_SHAPE_WIRE_FULL_DEVICE / SP_SHAPE_WIRE_FULL force the device / host
// form of the full shape (neither: ss_prover_full_device_default), SP_SHAPE_WIRE_TIMED, SS_PK_TRUST_DIGEST (1 << 16) takes the stored digest unhashed. Every
// prover and verifier entry point takes the key as it takes ss_setup's; ss_vk_to_bytes / ss_pk_to_bytes refuse it; ss_pk_free ends it.
int ss_prover_from_bytes(sp_ctx* ctx, const uint8_t* bytes, size_t n, unsigned flags, void** out_pk) {
  try {
    if (!out_pk) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "ss_prover_from_bytes: null out");
    *out_pk = nullptr;
    *out_pk = prover_from_bytes(ctx, bytes, n, flags);
    return 0;
  } catch (...) {
    return catch_all();
  }
}
// ms of the calling thread's last ss_prover_from_bytes: ss_verifier_stages' six, then 1 / 0 = shape on the device / host, 1 / 0 = digest hashed / trusted
void ss_prover_stages(double out[8]) { memcpy(out, g_pk_stage_ms, sizeof g_pk_stage_ms); }
int ss_prover_full_device_default(void) { return PK_FULL_DEVICE_DEFAULT ? 1 : 0; }
// A verifier's key from those bytes (see verifier_from_bytes). flags: 0, or SP_SHAPE_WIRE_DEVICE / SP_SHAPE_WIRE_HOST to force a decode form, and
// SP_SHAPE_WIRE_TIMED. The key is taken by ss_verify, ss_verify_bytes, ss_verify_batch, ss_verify_bytes_batch, ss_pk_info, ss_pk_shape_info,
// ss_proof_layout, ss_proof_words and ss_proof_to_bytes; every prover entry point refuses it ("verifier-only key"). ss_verifier_free (= ss_pk_free) ends it.
int ss_verifier_from_bytes(sp_ctx* ctx, const uint8_t* bytes, size_t n, unsigned flags, void** out_vk) {
  try {
    if (!out_vk) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "ss_verifier_from_bytes: null out");
    *out_vk = nullptr;
    *out_vk = verifier_from_bytes(ctx, bytes, n, flags);
    return 0;
  } catch (...) {
    return catch_all();
  }
}
void ss_verifier_free(void* vk) { delete (SpartanProverKey*)vk; }
// ms of the calling thread's last ss_verifier_from_bytes: Hyrax keys read, sp_shape_from_wire, the two sp_ck_create, the digest (helper thread), the wait
// for the digest behind the rest, the whole call; two spare slots
void ss_verifier_stages(double out[8]) { memcpy(out, g_vk_stage_ms, sizeof g_vk_stage_ms); }
int ss_pk_shape_info(void* pk_, uint64_t out[8]) { return sp_shape_info(((SpartanProverKey*)pk_)->S, out); }
void ss_pk_info(void* pk_, uint64_t dims_out[10], uint8_t digest[32]) {
  auto* pk = (SpartanProverKey*)pk_;
  memcpy(dims_out, &pk->dims, sizeof(sp_dims));
  memcpy(digest, pk->vk_digest, 32);
}
int ss_prep_prove(void* pk, const uint64_t* witness_u64, size_t n, int is_small, const uint8_t* tape, size_t tape_blocks, size_t* tape_used, void** out_ps) {
  try {
    Tape t{tape, tape_blocks};
    *out_ps = prep_prove(prover_key(pk, "ss_prep_prove"), witness_u64, n, is_small != 0, t);
    if (tape_used) *tape_used = t.pos;
    return 0;
  } catch (...) {
    return catch_all();
  }
}
// prep_prove with the SHA-256 witness generated on the device (see prep_prove_sha256): out_publics = the 256 digest bits to hand to ss_prove
int ss_prep_prove_sha256(void* pk, const sp_sha256_plan* plan, const uint8_t* msg, size_t len, int is_small, const uint8_t* tape, size_t tape_blocks, size_t* tape_used,
                         void** out_ps, uint64_t out_publics[256]) {
  try {
    Tape t{tape, tape_blocks};
    *out_ps = prep_prove_sha256(prover_key(pk, "ss_prep_prove_sha256"), plan, msg, len, is_small != 0, t, out_publics);
    if (tape_used) *tape_used = t.pos;
    return 0;
  } catch (...) {
    return catch_all();
  }
}
// prep_prove for `count` states of one key in one pass (see prep_prove_batch_from): witnesses_u64[k] = the n_witness words of state k (one length for all:
// the key's), tapes[k] / tape_blocks[k] = its tape, tape_used[k] = the blocks it consumed, out_ps[k] = its state - the state ss_prep_prove makes of the same
// witness and tape, to be proved alone or in any ss_prove_batch, checked, freed on its own. phase_ms (8, optional): the batch's wall-clock per phase in
// ss_prep_phases' slots. flags: SS_PREP_PER_STATE_COMMIT (1) = one sp_hyrax_commit per state, SS_PREP_PER_STATE_MATVEC (2) = one sp_multiply_vec per state
// (what the driver takes anyway, as measured), SS_PREP_CHUNKED_MATVEC (4) = the cached products through sp_multiply_vec_chunked.
// count == 0, null arguments and a wrong witness length are refused before any device work; on any failure every state made so far is freed and out_ps
// is not written; the error names the state where one is at fault ("prep_prove_batch: state 2: ...").
int ss_prep_prove_batch_opts(void* pk, const uint64_t* const* witnesses_u64, size_t n_witness, size_t count, int is_small, const uint8_t* const* tapes,
                             const size_t* tape_blocks, size_t* tape_used, void** out_ps, double* phase_ms, unsigned flags) {
  try {
    if (count == 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: count must be at least 1");
    if (!pk || !witnesses_u64 || !tapes || !tape_blocks || !out_ps) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: null argument");
    std::vector<Tape> ts;
    for (size_t k = 0; k < count; ++k) {
      if (!tapes[k]) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: state " + std::to_string(k) + ": null tape");
      ts.push_back(Tape{tapes[k], tape_blocks[k]});
    }
    std::vector<SpartanPrepSNARK*> st = prep_prove_batch(prover_key(pk, "ss_prep_prove_batch"), witnesses_u64, n_witness, count, is_small != 0, ts.data(), flags, phase_ms);
    for (size_t k = 0; k < count; ++k) {
      out_ps[k] = st[k];
      if (tape_used) tape_used[k] = ts[k].pos;
    }
    return 0;
  } catch (...) {
    return catch_all();
  }
}
int ss_prep_prove_batch(void* pk, const uint64_t* const* witnesses_u64, size_t n_witness, size_t count, int is_small, const uint8_t* const* tapes, const size_t* tape_blocks,
                        size_t* tape_used, void** out_ps, double* phase_ms) {
  return ss_prep_prove_batch_opts(pk, witnesses_u64, n_witness, count, is_small, tapes, tape_blocks, tape_used, out_ps, phase_ms, 0);
}
// the same with the SHA-256 witnesses generated on the device in ONE launch (see prep_prove_sha256): msgs = count x len bytes, out_publics = count x 256 digest bits
int ss_prep_prove_sha256_batch_opts(void* pk, const sp_sha256_plan* plan, const uint8_t* msgs, size_t len, size_t count, int is_small, const uint8_t* const* tapes,
                                    const size_t* tape_blocks, size_t* tape_used, void** out_ps, uint64_t* out_publics, double* phase_ms, unsigned flags) {
  try {
    if (count == 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: count must be at least 1");
    if (!pk || !plan || (!msgs && len) || !tapes || !tape_blocks || !out_ps || !out_publics) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: null argument");
    std::vector<Tape> ts;
    for (size_t k = 0; k < count; ++k) {
      if (!tapes[k]) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: state " + std::to_string(k) + ": null tape");
      ts.push_back(Tape{tapes[k], tape_blocks[k]});
    }
    std::vector<SpartanPrepSNARK*> st = prep_prove_sha256_batch(prover_key(pk, "ss_prep_prove_sha256_batch"), plan, msgs, len, count, is_small != 0, ts.data(), out_publics, flags, phase_ms);
    for (size_t k = 0; k < count; ++k) {
      out_ps[k] = st[k];
      if (tape_used) tape_used[k] = ts[k].pos;
    }
    return 0;
  } catch (...) {
    return catch_all();
  }
}
int ss_prep_prove_sha256_batch(void* pk, const sp_sha256_plan* plan, const uint8_t* msgs, size_t len, size_t count, int is_small, const uint8_t* const* tapes,
                               const size_t* tape_blocks, size_t* tape_used, void** out_ps, uint64_t* out_publics, double* phase_ms) {
  return ss_prep_prove_sha256_batch_opts(pk, plan, msgs, len, count, is_small, tapes, tape_blocks, tape_used, out_ps, out_publics, phase_ms, 0);
}
void ss_prep_free(void* ps) { delete (SpartanPrepSNARK*)ps; }
// host wall-clock of the last prep_prove's phases, ms: witness, commit, tables, matvec, scratch, (spare), total, (spare). A state made by
// ss_prep_prove_batch* carries the BATCH's phase times divided by its count (the phases ran once for all states).
// the FixedBaseMul tables of the committed rows (queued by prep_prove): 1 = built, 0 = still building (wait != 0: blocks), -1 = this state has none
int ss_prep_tables_ready(void* ps, int wait) {
  auto* p = (SpartanPrepSNARK*)ps;
  return p->lz_tables ? sp_fbtables_ready(p->lz_tables, wait) : -1;
}
void ss_prep_phases(void* ps, double out[8]) { memcpy(out, ((SpartanPrepSNARK*)ps)->prep_ms, sizeof(double) * 8); }
// driver options of one prep state: bit 0 = cache the transcript prefix across proves, bit 1 = opening in the reference's order (see FLAG_*)
void ss_prep_set_flags(void* ps, unsigned flags) { ((SpartanPrepSNARK*)ps)->flags = flags; }
unsigned ss_prep_get_flags(void* ps) { return ((SpartanPrepSNARK*)ps)->flags; }
// comm_W_precommitted rows (affine) and the cached Az/Bz/Cz for parity checks
int ss_prep_export(void* pk_, void* ps_, uint64_t* comm_rows, uint64_t* caz, uint64_t* cbz, uint64_t* ccz) {
  try {
    auto* pk = (SpartanProverKey*)pk_;
    auto* ps = (SpartanPrepSNARK*)ps_;
    if (comm_rows && !ps->comm_W_fixed.empty()) memcpy(comm_rows, ps->comm_W_fixed.data(), ps->comm_W_fixed.size() * sizeof(aff_t));
    const size_t N = pk->dims.num_cons;
    if (caz) ck(sp_table_read(pk->ctx, ps->caz, 0, N, caz), "read caz");
    if (cbz) ck(sp_table_read(pk->ctx, ps->cbz, 0, N, cbz), "read cbz");
    if (ccz) ck(sp_table_read(pk->ctx, ps->ccz, 0, N, ccz), "read ccz");
    return 0;
  } catch (...) {
    return catch_all();
  }
}
// R1CSShape::is_sat on a prepared state (see is_sat): 0 = satisfied and the commitment matches; SP_ERR_UNSAT with ss_last_error() = the reference's reason
// ("R1CS is unsatisfiable", which takes precedence, or "Invalid commitment"); another negative value = misuse / library error. The report and the list of
// mismatching commitment rows (at most bad_rows_cap of the *n_bad_rows found; shared rows first) are filled in either case. challenges (num_challenges x 4
// Montgomery limbs) and synth: circuits with verifier challenges only. expect_comm_rows: NULL = compare with the commitment the state holds.
int ss_prep_is_sat(void* pk, void* ps, const uint64_t* publics_u64, size_t npub, const uint64_t* challenges, ss_rest_hook synth, void* synth_user,
                   const uint64_t* expect_comm_rows, sp_sat_report* report, uint64_t* bad_rows, size_t bad_rows_cap, size_t* n_bad_rows) {
  try {
    prover_key(pk, "ss_prep_is_sat");
    if (!ps) throw Error(SP_ERR_INTERNAL, "is_sat before prep_prove");
    sp_sat_report local;
    std::vector<uint64_t> bad;
    const char* reason = nullptr;
    const bool ok = is_sat(prover_key(pk, "ss_prep_is_sat"), *(SpartanPrepSNARK*)ps, publics_u64, npub, challenges, synth, synth_user, expect_comm_rows, report ? report : &local, &bad, &reason);
    if (n_bad_rows) *n_bad_rows = bad.size();
    if (bad_rows) std::copy(bad.begin(), bad.begin() + std::min(bad.size(), bad_rows_cap), bad_rows);
    if (ok) return 0;
    g_err = reason;
    return SP_ERR_UNSAT;
  } catch (...) {
    return catch_all();
  }
}
// SpartanSNARK::verify on the device-backed path: 0 = accept, 1..6 = the failed check (see spartan2::verify); < 0 = library error
// out_publics (may be NULL): num_public scalars (Montgomery limbs) of the statement that was accepted
int ss_verify(void* pk, const uint64_t* words, size_t nwords, uint64_t* out_publics) {
  try {
    return verify(*(SpartanProverKey*)pk, words, nwords, out_publics);
  } catch (...) {
    return catch_all();
  }
}
// verify_batch (see spartan2::verify_batch): `count` proofs of this key, codes[k] = what ss_verify returns for proof k (0 accept, 1..6). seed: 32 bytes
// mixed into the weights of the combined opening check, or NULL. out_publics (may be NULL): count x num_public scalars, row k written when codes[k] == 0.
// info may be NULL. Returns 0, or < 0 = library error (the codes are then meaningless).
int ss_verify_batch(void* pk, const uint64_t* const* words, const size_t* nwords, size_t count, const uint8_t* seed, int* codes, uint64_t* out_publics,
                    ss_verify_batch_info* info) {
  try {
    verify_batch(*(SpartanProverKey*)pk, words, nwords, count, seed, codes, out_publics, info);
    return 0;
  } catch (...) {
    return catch_all();
  }
}
void ss_proof_layout(void* pk, sp_spartan_layout* out) { *out = ((SpartanProverKey*)pk)->layout.wire(); }
// the proof as bincode bytes of SpartanSNARK (src/spartan.rs:125-137); out may be NULL to learn *len
int ss_proof_to_bytes(void* pk, const uint64_t* words, size_t nwords, uint8_t* out, size_t cap, size_t* len) {
  try {
    const sp_spartan_layout L = ((SpartanProverKey*)pk)->layout.wire();
    ck(sp_proof_serialize(&L, words, nwords, out, cap, len), "proof_serialize");
    return 0;
  } catch (...) {
    return catch_all();
  }
}
// verify on the serialised proof (what a verifier that received bytes runs): 0 = accept, 1..6 = the failed check — bytes that do not decode, or decode
// to a proof of another shape, fail check 1 like a malformed flat proof —, < 0 = error
int ss_verify_bytes(void* pk_, const uint8_t* bytes, size_t n, uint64_t* out_publics) {
  try {
    auto* pk = (SpartanProverKey*)pk_;
    sp_spartan_layout L;
    size_t nwords = 0;
    if (sp_proof_deserialize(bytes, n, &L, nullptr, 0, &nwords) != SP_OK) return 1;
    const sp_spartan_layout want = pk->layout.wire();
    if (memcmp(&L, &want, sizeof L) != 0) return 1;
    std::vector<uint64_t> words(nwords);
    ck(sp_proof_deserialize(bytes, n, &L, words.data(), words.size(), &nwords), "proof_deserialize");
    return verify(*pk, words.data(), nwords, out_publics);
  } catch (...) {
    return catch_all();
  }
}
// the same over serialised proofs: bytes that do not decode to a proof of this key's shape get code 1, as in ss_verify_bytes
int ss_verify_bytes_batch(void* pk_, const uint8_t* const* bytes, const size_t* nbytes, size_t count, const uint8_t* seed, int* codes, uint64_t* out_publics,
                          ss_verify_batch_info* info) {
  try {
    auto* pk = (SpartanProverKey*)pk_;
    const sp_spartan_layout want = pk->layout.wire();
    std::vector<std::vector<uint64_t>> store(count);
    std::vector<const uint64_t*> words(count);
    std::vector<size_t> nwords(count);
    for (size_t k = 0; k < count; ++k) {
      sp_spartan_layout L;
      size_t nw = 0;
      if (sp_proof_deserialize(bytes[k], nbytes[k], &L, nullptr, 0, &nw) == SP_OK && memcmp(&L, &want, sizeof L) == 0) {
        store[k].resize(nw);
        ck(sp_proof_deserialize(bytes[k], nbytes[k], &L, store[k].data(), store[k].size(), &nw), "proof_deserialize");
      }  // else: no words, which fails the length check of step (a) with code 1
      words[k] = store[k].data();
      nwords[k] = store[k].size();
    }
    verify_batch(*pk, words.data(), nwords.data(), count, seed, codes, out_publics, info);
    return 0;
  } catch (...) {
    return catch_all();
  }
}
size_t ss_proof_words(void* pk) { return ((SpartanProverKey*)pk)->layout.words(); }
// prove() — writes the proof in the canonical layout; phase_ms[7]: witness_commit, matrix_vector_multiply, outer_sumcheck,
// prepare_poly_ABC, inner_sumcheck, pcs_prove, total (the reference's span names, src/spartan.rs:267-437)
int ss_prove_hook(void* pk, void* ps, const uint64_t* publics_u64, size_t npub, const uint8_t* tape, size_t tape_blocks, size_t* tape_used, uint64_t* out_words,
                  size_t out_cap, double* phase_ms, ss_rest_hook synth, void* synth_user);
int ss_prove(void* pk, void* ps, const uint64_t* publics_u64, size_t npub, const uint8_t* tape, size_t tape_blocks, size_t* tape_used, uint64_t* out_words,
             size_t out_cap, double* phase_ms) {
  return ss_prove_hook(pk, ps, publics_u64, npub, tape, tape_blocks, tape_used, out_words, out_cap, phase_ms, nullptr, nullptr);
}
// the same for circuits with verifier challenges: `synth` is the circuit's synthesize callback (see prove)
int ss_prove_hook(void* pk, void* ps, const uint64_t* publics_u64, size_t npub, const uint8_t* tape, size_t tape_blocks, size_t* tape_used, uint64_t* out_words,
                  size_t out_cap, double* phase_ms, ss_rest_hook synth, void* synth_user) {
  try {
    Tape t{tape, tape_blocks};
    PhaseTimes pt;
    ProofBuf pf = prove(prover_key(pk, "ss_prove"), *(SpartanPrepSNARK*)ps, publics_u64, npub, t, &pt, synth, synth_user);
    if (pf.words.size() > out_cap) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "proof buffer too small");
    memcpy(out_words, pf.words.data(), pf.words.size() * 8);
    if (tape_used) *tape_used = t.pos;
    if (phase_ms) memcpy(phase_ms, pt.ms, 7 * sizeof(double));
    if (getenv("SPARTAN_HOST_LAPS")) {
      for (auto& l : pt.laps) fprintf(stderr, "lap %-28s %.3f ms\n", l.first.c_str(), l.second);
    }
    // SPARTAN_SLOW_PROVE_MS=<t>: a prove that took longer than t ms leaves its phases and laps on stderr (diagnostics for rare stalls)
    static const double slow_ms = [] {
      const char* e = getenv("SPARTAN_SLOW_PROVE_MS");
      return e ? atof(e) : 0.0;
    }();
    if (slow_ms > 0 && pt.ms[6] > slow_ms) {
      fprintf(stderr, "[slow prove] %.3f ms: witness %.3f mv %.3f outer %.3f abc %.3f inner %.3f pcs %.3f\n", pt.ms[6], pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4], pt.ms[5]);
      for (auto& l : pt.laps) fprintf(stderr, "[slow prove]   lap %-28s %.3f ms\n", l.first.c_str(), l.second);
    }
    return 0;
  } catch (...) {
    return catch_all();
  }
}
// prove_batch(): `count` states of one key (pss), publics count x npub words, one tape per proof (tapes[k]: tape_blocks[k] blocks of 64 bytes), out_words
// count x out_cap_each words (proof k at k * out_cap_each, ss_proof_words(pk) words long), tape_used[k] = blocks proof k consumed; phase_ms[7]: the
// batch's wall-clock per phase, in ss_prove's slots; flags: SS_BATCH_PER_PROOF_OPENING = the openings as `count` sp_hyrax_prove calls (same proofs);
// SS_BATCH_OPENING_AHEAD / SS_BATCH_OPENING_BEHIND = the batched opening begun ahead of the sum-checks / called behind them (same proofs; prove_batch_chunk)
int ss_prove_batch_opts(void* pk, void* const* pss, size_t count, const uint64_t* publics_u64, size_t npub, const uint8_t* const* tapes, const size_t* tape_blocks,
                        size_t* tape_used, uint64_t* out_words, size_t out_cap_each, double* phase_ms, unsigned flags) {
  try {
    if (!pk || !tapes || !tape_blocks || !out_words) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: null argument");
    std::vector<Tape> ts;
    for (size_t k = 0; k < count; ++k) ts.push_back(Tape{tapes[k], tape_blocks[k]});
    PhaseTimes pt;
    std::vector<ProofBuf> pf = prove_batch(prover_key(pk, "ss_prove_batch"), (SpartanPrepSNARK* const*)pss, count, publics_u64, npub, ts.data(), &pt, flags);
    for (size_t k = 0; k < count; ++k) {
      if (pf[k].words.size() > out_cap_each) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "proof buffer too small");
      memcpy(out_words + k * out_cap_each, pf[k].words.data(), pf[k].words.size() * 8);
      if (tape_used) tape_used[k] = ts[k].pos;
    }
    if (phase_ms) memcpy(phase_ms, pt.ms, 7 * sizeof(double));
    return 0;
  } catch (...) {
    return catch_all();
  }
}
int ss_prove_batch(void* pk, void* const* pss, size_t count, const uint64_t* publics_u64, size_t npub, const uint8_t* const* tapes, const size_t* tape_blocks,
                   size_t* tape_used, uint64_t* out_words, size_t out_cap_each, double* phase_ms) {
  return ss_prove_batch_opts(pk, pss, count, publics_u64, npub, tapes, tape_blocks, tape_used, out_words, out_cap_each, phase_ms, 0);
}
// ---- several proofs in flight on ONE thread ------------------------------------------------------------------------------------------------------
// A prove is a chain of ~41 host <-> device round trips whose host side is a few microseconds of hashing and two kernel launches: one CPU spinning
// per proof in flight wastes the CPU and, under a CPU quota, caps the number of proofs in flight. Here every proof runs on a stack of its own
// (ucontext) and the library's wait hook (sp_set_wait_hook) hands the thread to the next proof at every poll: `threads` OS threads keep
// n_ctx proofs in flight, the GPU sees the same launches. The prove code itself is untouched — it blocks, its stack waits.
}  // extern "C"
#include <ucontext.h>
namespace {
struct Fiber {
  ucontext_t uc;
  std::unique_ptr<char[]> stack;
  std::function<void()> body;
  bool done = false;
  std::exception_ptr err;
};
struct Scheduler {
  ucontext_t main;
  std::vector<Fiber*> fibers;
  Fiber* cur = nullptr;
  uint64_t switches = 0;
  double wait_s = 0;  // wall time the thread's proofs spent in polls (summed over the proofs: what is left of the batch's time is host work)
  static void hook(void* u) {
    Scheduler* s = (Scheduler*)u;
    ++s->switches;
    const auto t0 = std::chrono::steady_clock::now();
    swapcontext(&s->cur->uc, &s->main);
    s->wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  static void entry(unsigned lo, unsigned hi) {
    Fiber* f = (Fiber*)(((uintptr_t)hi << 32) | (uintptr_t)lo);
    try {
      f->body();
    } catch (...) {
      f->err = std::current_exception();
    }
    f->done = true;  // returning resumes uc_link = the scheduler
  }
  void add(Fiber* f, size_t stack_bytes) {
    f->stack.reset(new char[stack_bytes]);
    getcontext(&f->uc);
    f->uc.uc_stack.ss_sp = f->stack.get();
    f->uc.uc_stack.ss_size = stack_bytes;
    f->uc.uc_link = &main;
    const uintptr_t p = (uintptr_t)f;
    makecontext(&f->uc, (void (*)())entry, 2, (unsigned)(p & 0xffffffffu), (unsigned)(p >> 32));
    fibers.push_back(f);
  }
  void run() {
    sp_set_wait_hook(&Scheduler::hook, this);
    size_t live = fibers.size();
    while (live) {
      for (Fiber* f : fibers) {
        if (f->done) continue;
        cur = f;
        swapcontext(&main, &f->uc);
        if (f->done) --live;
      }
    }
    sp_set_wait_hook(nullptr, nullptr);
  }
};
}  // namespace
extern "C" {
// n_ctx prepared states (pks[i], pss[i]: one context each, all on one device) prove `proofs_each` times each, multiplexed over `threads` OS threads.
// out_words: n_ctx x words_cap, the LAST proof of every state; out_stats: seconds of the whole batch, context switches, proofs, seconds spent inside polls summed over the proofs.
int ss_prove_multiplexed(void** pks, void** pss, size_t n_ctx, const uint64_t* publics_u64, size_t npub, const uint8_t* tape, size_t tape_blocks, size_t proofs_each,
                         size_t threads, uint64_t* out_words, size_t words_cap, double out_stats[4]) {
  try {
    if (n_ctx == 0 || threads == 0 || proofs_each == 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "ss_prove_multiplexed: nothing to do");
    if (threads > n_ctx) threads = n_ctx;
    std::vector<Fiber> fibers(n_ctx);
    std::vector<Scheduler> sched(threads);
    for (size_t i = 0; i < n_ctx; ++i) {
      auto* pk = &prover_key(pks[i], "ss_prove_multiplexed");
      auto* ps = (SpartanPrepSNARK*)pss[i];
      uint64_t* dst = out_words + i * words_cap;
      fibers[i].body = [=] {
        for (size_t k = 0; k < proofs_each; ++k) {
          Tape t{tape, tape_blocks};
          ProofBuf pf = prove(*pk, *ps, publics_u64, npub, t, nullptr, nullptr, nullptr);
          if (pf.words.size() > words_cap) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "proof buffer too small");
          if (k + 1 == proofs_each) memcpy(dst, pf.words.data(), pf.words.size() * 8);
        }
      };
      sched[i % threads].add(&fibers[i], (size_t)1 << 20);
    }
    std::atomic<int> ready{0};
    std::atomic<bool> go{false};
    std::vector<std::thread> th;
    std::vector<int> rc(threads, 0);
    for (size_t t = 0; t < threads; ++t)
      th.emplace_back([&, t] {
        rc[t] = sp_ctx_bind_thread(((SpartanProverKey*)pks[t])->ctx);
        ready.fetch_add(1);
        while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
        if (rc[t] == 0) sched[t].run();
      });
    while (ready.load() < (int)threads) std::this_thread::yield();
    const auto t0 = std::chrono::steady_clock::now();
    go.store(true, std::memory_order_release);
    for (auto& x : th) x.join();
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t sw = 0;
    double waited = 0;
    for (auto& s : sched) sw += s.switches, waited += s.wait_s;
    if (out_stats) {
      out_stats[0] = secs;
      out_stats[1] = (double)sw;
      out_stats[2] = (double)(n_ctx * proofs_each);
      out_stats[3] = waited;
    }
    for (size_t t = 0; t < threads; ++t)
      if (rc[t]) throw Error(rc[t], "ss_prove_multiplexed: could not bind a poller thread to the device");
    for (auto& f : fibers)
      if (f.err) std::rethrow_exception(f.err);
    return 0;
  } catch (...) {
    return catch_all();
  }
}
}
