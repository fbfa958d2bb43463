// NeutronNovaZkSNARK::{setup, prep_prove, prove, verify} (src/neutronnova_zk.rs:1394-2343) above the C ABI — SURVEY.md 8(f) rank 1, BASELINE config 3 as a real
// prove(): rerandomization, the step / core instances, NeutronNovaNIFS::prove with the verifier circuit's `process_round` as its round hook, the batched
// outer and inner sum-checks (process_round again), the verifier-circuit instance folded with a fresh random relaxed instance (NovaNIFS::prove,
// src/nifs.rs:34-61 + commit_T, src/r1cs/folds.rs:28-88), RelaxedR1CSSpartanProof::prove (src/spartan_relaxed.rs:98-213) and the folded Hyrax opening.
// Everything that scales with the step instances runs on the device through include/spartan_hip.h; the verifier-circuit instance (a few hundred
// constraints, ~1.3 k variables) is host-side algebra except its commitments (sp_hyrax_commit_small / sp_hyrax_commit on the width-32 key) and its
// two sum-checks (sp_sumcheck_cubic3 / sp_sumcheck_quad).
// Scope = the bench circuits' class: step and core circuits without rest variables and without verifier challenges (`can_cache_matvec`, :1520).
// The proof layout is the oracle's NNProof::serialize (oracle/neutronnova_zk.hpp); parity = word-for-word equality on the same inputs and tape.
#include <deque>
#include <future>
#include <memory>

#include "neutronnova_nifs.hpp"
#include "proof_layout.hpp"

namespace spartan2 {

// One helper thread taking jobs in order (FIFO). submit() never blocks; a job's failure is kept for the next wait() and does not stop the jobs behind it.
class Worker {
  std::thread th_;
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
  bool stop_ = false;
  size_t submitted_ = 0;  // written by the submitting thread only
  std::atomic<size_t> done_{0};
  std::exception_ptr err_;
  void loop() {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return stop_ || !q_.empty(); });
        if (q_.empty()) return;
        f = std::move(q_.front());
        q_.pop_front();
      }
      try {
        f();
      } catch (...) {
        std::lock_guard<std::mutex> l(m_);
        if (!err_) err_ = std::current_exception();
      }
      done_.fetch_add(1, std::memory_order_release);
    }
  }

 public:
  Worker() = default;
  Worker(const Worker&) = delete;
  Worker& operator=(const Worker&) = delete;
  ~Worker() {
    if (!th_.joinable()) return;
    drain();
    {
      std::lock_guard<std::mutex> l(m_);
      stop_ = true;
    }
    cv_.notify_one();
    th_.join();
  }
  size_t submit(std::function<void()> f) {  // returns the ticket to wait for
    size_t t;
    {
      std::lock_guard<std::mutex> l(m_);
      q_.push_back(std::move(f));
      t = ++submitted_;
    }
    if (!th_.joinable()) th_ = std::thread([this] { loop(); });
    cv_.notify_one();
    return t;
  }
  void drain() {  // every job submitted so far has run; drops what they threw (exit paths)
    while (done_.load(std::memory_order_acquire) < submitted_) sp_relax();
    std::lock_guard<std::mutex> l(m_);
    err_ = nullptr;
  }
  void wait(size_t ticket) {  // jobs up to `ticket` have run; rethrows the first failure
    while (done_.load(std::memory_order_acquire) < ticket) sp_relax();
    std::exception_ptr e;
    {
      std::lock_guard<std::mutex> l(m_);
      e = err_;
      err_ = nullptr;
    }
    if (e) std::rethrow_exception(e);
  }
};

struct NNZkKey {
  sp_ctx* ctx = nullptr;
  sp_shape *S_step = nullptr, *S_core = nullptr;
  sp_dims dims, dims_core;
  sp_ck *ck = nullptr, *vc_ck = nullptr;
  std::vector<aff_t> gens;  // "ck": 2048 bases + h; the width-32 key is its first 32 bases with gens[32] as h (PCS::setup(b"ck", ., 32), src/r1cs/mod.rs:1690-1693)
  vcirc::Shape vc;
  NNLayout layout;  // of a proof under this key (proof_layout.hpp)
  size_t nb = 0, nx = 0, ny = 0, num_steps = 0, num_vars = 0;
  uint8_t vk_digest[32];
  // a key loaded from its bytes (nn_key_from_bytes): a verifier's holds row-only shapes and is refused by every prover entry point; both keep the width-32
  // key's generators as the bytes gave them (vc_gens: 32 bases + h) and are refused by the writers
  bool verifier_only = false, from_bytes = false;
  std::vector<aff_t> vc_gens;
  // verify(): eq tables and the three M * T_y products of the matrix evaluations, allocated on first use
  mutable sp_table *v_Tx = nullptr, *v_Ty = nullptr, *v_mv[3] = {nullptr, nullptr, nullptr};
  // r_b, r_x and r_y are fields of the proof, so the commitment fold and the matrix evaluations can start before the transcript has been replayed:
  // they run as jobs on a second context of the same GPU beside the replay, NovaNIFS::verify and the relaxed Spartan check
  mutable sp_ctx* v_ctx2 = nullptr;
  mutable Worker v_wk;
  mutable std::vector<sp_table*> vb_Tx, vb_Ty;  // verify_batch()'s (T_x, T_y) pairs of one chunk of proofs, kept like the above
  ~NNZkKey() {
    v_wk.drain();
    sp_ctx_destroy(v_ctx2);
    for (sp_table* t : vb_Tx) sp_table_free(t);
    for (sp_table* t : vb_Ty) sp_table_free(t);
    sp_table_free(v_Tx);
    sp_table_free(v_Ty);
    for (sp_table* t : v_mv) sp_table_free(t);
    sp_shape_free(S_step);
    sp_shape_free(S_core);
    sp_ck_free(ck);
    sp_ck_free(vc_ck);
  }
};

struct NNPre {  // PrecommittedState, values only
  sp_table* W = nullptr;
  std::vector<aff_t> comm_pre;
  std::vector<fe_t> r_pre, publics;
};
struct NNZkPrep {
  std::vector<NNPre> steps;
  NNPre core;
  std::vector<aff_t> comm_shared;
  std::vector<fe_t> r_shared;
  bool is_small = true;
  // cached_step_matvec / cached_step_i64 (:1520-1590): the step instances' (Az, Bz, Cz) layers and their i64 mirrors; the rounds only read them
  sp_nifs* nifs_cached = nullptr;
  // small device tables reused by every prove (the verifier-circuit instance is a few thousand elements: its commits and two sum-checks would
  // otherwise pay eight hipMalloc / hipFree pairs per prove)
  sp_table* vws[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t vws_cap[5] = {0, 0, 0, 0, 0};
  // Two pieces of prove() read nothing the transcript produces before they are needed: the random relaxed instance of the verifier circuit with its
  // two commitments (values from the randomness tape only, src/r1cs/mod.rs:474-531) and the fold of the step instances' commitments (read first by the
  // opening, :2019-2065). They run as jobs of one helper thread on a SECOND context of the same GPU (own streams and workspaces), under the NIFS rounds
  // and the two batched sum-checks, instead of 0.8 ms each on the critical path.
  // the sixteen working tables of a prove (layers out of the NIFS, core products, pow / eq tables, both poly_ABC and z pairs, the folded witnesses):
  // their sizes are the key's, so they are allocated once (a prove used to pay sixteen hipMalloc / hipFree pairs, the frees after its last phase)
  sp_table* work[16] = {};
  size_t work_cap[16] = {};
  sp_table* rest_stage = nullptr;  // rest segments of several instances side by side (one commitment call for all of them)
  size_t rest_stage_cap = 0;
  sp_ctx* ctx2 = nullptr;
  Worker wk;
  sp_table* bws[2] = {nullptr, nullptr};
  size_t bws_cap[2] = {0, 0};
  struct RandomInstance {
    std::vector<fe_t> Z, rW, rE, E;
    std::vector<aff_t> comm_W, comm_E;
    size_t tape_from = 0, tape_count = 0;
    bool valid = false;
  } rnd;
  // two more jobs of the same kind for the opening (hyrax_pc.rs:387-478, ipa.rs:125-170): `delta`, the commitment of the IPA's mask (tape values only), and
  // - once r_y is known - P_f = <L, folded rows>, P_c = <L, core rows> and beta: comm_LZ = commit(L^T W; <L, blinds>) is the same group element as
  // P_f + c_eval * P_c (W = folded W + c_eval * core W row by row), so the 2048-point MSM behind the last challenge becomes one scalar multiplication
  struct OpeningAhead {
    std::vector<fe_t> dv;
    fe_t r_delta, r_beta;
    aff_t delta, beta, P_f, P_c;
    size_t tape_from = 0, tape_count = 0;
    bool delta_valid = false, points_valid = false;
    sp_fold2_job* lz_fold = nullptr;  // comm_LZ = P_f + c_eval P_c: P_c's doubling ladder, begun by the helper when it has the point

  } open;
  ~NNZkPrep() {
    wk.drain();
    sp_fold_commitments2_drop(open.lz_fold);
    for (sp_table* t : bws) sp_table_free(t);
    for (sp_table* t : work) sp_table_free(t);
    sp_table_free(rest_stage);
    sp_ctx_destroy(ctx2);
    for (auto& s : steps) sp_table_free(s.W);
    sp_table_free(core.W);
    sp_nifs_free(nifs_cached);
    for (sp_table* t : vws) sp_table_free(t);
  }
};

static NNZkKey* nn_setup(sp_ctx* ctx, const R1CSIntView& Rs, const R1CSIntView& Rc, size_t num_steps) {
  auto* pk = new NNZkKey();
  try {
    pk->ctx = ctx;
    pk->num_steps = num_steps;
    // one step means zero NIFS rounds, and the reference's verifier circuit then reads prior_round_vars[round_index - 1] at round 0 (src/zk.rs:637-641):
    // NeutronNovaZkSNARK::setup panics there, this driver refuses
    if (num_steps < 2) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "NeutronNova: at least two step circuits (the verifier circuit has no NIFS round to take its claim from)");
    PaddedShape Ps = pad_shape(Rs), Pc = pad_shape(Rc);
    equalize(Ps, Pc);  // src/neutronnova_zk.rs:1413
    // equalize leaves the shared and precommitted segments alone. Step and core may split their variables into precommitted | rest differently (the folds and
    // the opening work on the combined rows, whose number equalize has made equal); the SHARED segment is one commitment for every circuit (comm_W_shared of
    // the proof is checked against S_step and S_core alike, src/neutronnova_zk.rs:2112-2158), so its padded size has to agree
    if (Ps.dims.num_shared != Pc.dims.num_shared)
      throw Error(SP_ERR_INVALID_INPUT_LENGTH, "NeutronNova: step and core circuits with different padded shared segments (one shared commitment serves both)");
    if (Ps.dims.num_challenges || Pc.dims.num_challenges) throw Error(SP_ERR_INTERNAL, "NeutronNova: step / core circuits with verifier challenges are not driven by this layer");
    // Rest variables (SpartanCircuit::synthesize; the reference's own test circuit is nothing else, src/neutronnova_zk.rs:2357-2418) come with the witness:
    // without challenges, what prove() re-synthesizes (bellpepper/r1cs.rs:443-461) is a function of the circuit alone. BESIDE shared / precommitted variables
    // they cannot be driven: NeutronNovaNIFS::prove folds only that prefix of the step witnesses when it is non-empty and takes the folded rest rows from the
    // blinds ("the rest portion is all zero for step circuits", :1215-1261), so the reference's own proof of such a shape does not verify.
    if (Ps.dims.num_rest_unpadded && Ps.dims.num_shared + Ps.dims.num_precommitted)
      throw Error(SP_ERR_INVALID_INPUT_LENGTH, "NeutronNova: step circuits with rest variables beside shared / precommitted ones (the reference's fold drops the rest segment)");
    pk->dims = Ps.dims;
    pk->dims_core = Pc.dims;
    pk->num_vars = Ps.num_vars();
    auto mk = [&](const PaddedShape& P, sp_shape** out) {
      sp_csr cs[3];
      for (int m = 0; m < 3; ++m) cs[m] = sp_csr{u64p(P.data[m].data()), P.idx[m].data(), P.ptr[m].data()};
      ck(sp_shape_from_csr(ctx, &cs[0], &cs[1], &cs[2], &P.dims, out), "shape_from_csr");
    };
    mk(Ps, &pk->S_step);
    mk(Pc, &pk->S_core);
    pk->gens = from_label("ck", DEFAULT_COMMITMENT_WIDTH + 1);
    ck(sp_ck_create(ctx, u64p(&pk->gens[0].x), DEFAULT_COMMITMENT_WIDTH, u64p(&pk->gens[DEFAULT_COMMITMENT_WIDTH].x), &pk->ck), "ck_create");
    ck(sp_ck_create(ctx, u64p(&pk->gens[0].x), 32, u64p(&pk->gens[32].x), &pk->vc_ck), "vc_ck_create");
    size_t np = 1;
    while (np < num_steps) np <<= 1;
    pk->nb = log2_ceil(np);
    pk->nx = log2_ceil(Ps.dims.num_cons);
    pk->ny = log2_ceil(pk->num_vars) + 1;
    pk->vc = vcirc::Shape::from_circuit(vcirc::Circuit(pk->nb, pk->nx, pk->ny, 32));
    pk->layout = NNLayout(pk->dims, pk->dims_core, num_steps, pk->vc);
    {  // NeutronNovaVerifierKey::write_bytes (src/neutronnova_zk.rs:1305-1333) -> SHA-256 (src/digest.rs:62-76)
      struct Sink {
        sp_wire* w = nullptr;
        ~Sink() { sp_wire_free(w); }
      } sink;
      ck(sp_wire_new(1, &sink.w), "wire sink");
      const uint64_t *g = u64p(&pk->gens[0].x), *h = u64p(&pk->gens[DEFAULT_COMMITMENT_WIDTH].x), *vh = u64p(&pk->gens[32].x);
      ck(sp_wire_hyrax_key(sink.w, g, DEFAULT_COMMITMENT_WIDTH, h), "vk: ck");
      ck(sp_wire_hyrax_key(sink.w, g, DEFAULT_COMMITMENT_WIDTH, h), "vk: vk_ee");  // the same generators (SplitR1CSShape::commitment_key)
      sp_csr cs[3];
      padded_csr(Ps, cs);
      ck(sp_wire_shape(sink.w, &Ps.dims, &cs[0], &cs[1], &cs[2], 1), "vk: S_step");
      padded_csr(Pc, cs);
      ck(sp_wire_shape(sink.w, &Pc.dims, &cs[0], &cs[1], &cs[2], 1), "vk: S_core");
      pk->vc.write_bincode(sink.w, false);  // vc_shape: SplitMultiRoundR1CSShape
      pk->vc.write_bincode(sink.w, true);   // vc_shape_regular: R1CSShape (to_regular_shape)
      ck(sp_wire_hyrax_key(sink.w, g, 32, vh), "vk: vc_ck");
      ck(sp_wire_hyrax_key(sink.w, g, 32, vh), "vk: vc_vk");
      ck(sp_wire_digest(sink.w, pk->vk_digest), "vk digest");
    }
  } catch (...) {
    delete pk;
    throw;
  }
  return pk;
}

// ---- NeutronNovaVerifierKey / NeutronNovaProverKey (src/neutronnova_zk.rs:1276-1303) to and from their bincode bytes -------------------------------------
// Derived field order, little-endian, fixint:
//   verifier: ck, vk_ee, S_step, S_core, vc_shape, vc_shape_regular, vc_ck, vc_vk                        (`digest` is #[serde(skip)])
//   prover:   ck, S_step, S_core, vk_digest (32 raw bytes, no length), vc_shape, vc_shape_regular, vc_ck
// For Hyrax a verifier key serialises as its commitment key does (vk_ee as ck, vc_vk as vc_ck). The shapes are the derived Serialize of SplitR1CSShape
// (sp_wire_shape(.., 0)); the verifier-circuit shapes are vcirc::Shape::write_bincode.
enum : unsigned { SS_PK_TRUST_DIGEST = 1u << 16 };  // the flag of ss_prover_from_bytes (spartan_snark.cpp), with its meaning: take the stored digest as it is
static double nn_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// A bounds-checked walk over key bytes for the digest: it reads lengths and skips arrays, and converts or checks no element.
struct NNKeyWalk {
  const uint8_t *p, *end;
  size_t left() const { return (size_t)(end - p); }
  uint64_t u64() {
    if (left() < 8) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "wire: unexpected end of input");
    uint64_t v;
    memcpy(&v, p, 8);
    p += 8;
    return v;
  }
  const uint8_t* skip(uint64_t count, size_t elem) {  // count elements of elem bytes
    if (elem && count > left() / elem) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "wire: length prefix exceeds the input");
    const uint8_t* at = p;
    p += (size_t)count * elem;
    return at;
  }
  void hyrax_key() {  // num_cols, Vec<Affine>, GE
    u64();
    skip(u64(), 64);
    skip(96, 1);
  }
  void matrix_vecs(const uint8_t* at[3], uint64_t head[4]) {  // SparseMatrix { data, indices, indptr, cols }: where the three arrays lie, and the lengths + cols
    head[0] = u64(), at[0] = skip(head[0], 32);
    head[1] = u64(), at[1] = skip(head[1], 8);
    head[2] = u64(), at[2] = skip(head[2], 8);
    head[3] = u64();
  }
};

// DigestHelperTrait::digest of NeutronNovaVerifierKey (SHA-256 over write_bytes, src/neutronnova_zk.rs:1305-1333) from the key's own serde bytes. write_bytes
// is bincode(ck) || bincode(vk_ee) || S_step.write_bytes() || S_core.write_bytes() || bincode of the last four fields; SplitR1CSShape::write_bytes and
// SparseMatrix::write_digest_bytes write the sequences of the derived Serialize with the three lengths and cols in front of each matrix (as in
// sp_vk_digest_from_wire), so the hash streams slices of the input and transcodes no entry array. `prover`: the bytes are a NeutronNovaProverKey - ck stands
// for vk_ee and vc_ck for vc_vk (each is hashed twice), and the 32 stored digest bytes behind S_core are stepped over (*stored, when asked for).
static void nn_vk_digest_from_bytes(const uint8_t* bytes, size_t n, bool prover, uint8_t out[32], const uint8_t** stored = nullptr) {
  struct Sink {
    sp_wire* w = nullptr;
    ~Sink() { sp_wire_free(w); }
  } sink;
  ck(sp_wire_new(1, &sink.w), "wire sink");
  auto hash = [&](const void* at, size_t len) { ck(sp_wire_raw(sink.w, (const uint8_t*)at, len), "wire_raw"); };
  NNKeyWalk r{bytes, bytes + n};
  r.hyrax_key();
  if (prover) hash(bytes, (size_t)(r.p - bytes));
  else r.hyrax_key();
  hash(bytes, (size_t)(r.p - bytes));
  for (int s = 0; s < 2; ++s) {  // S_step, S_core
    hash(r.skip(80, 1), 80);
    for (int m = 0; m < 3; ++m) {
      const uint8_t* at[3];
      uint64_t head[4];
      r.matrix_vecs(at, head);
      hash(head, sizeof head);
      hash(at[0], 32 * (size_t)head[0]);
      hash(at[1], 8 * (size_t)head[1]);
      hash(at[2], 8 * (size_t)head[2]);
    }
  }
  if (!prover) {  // vc_shape, vc_shape_regular, vc_ck, vc_vk as they stand
    hash(r.p, r.left());
  } else {
    const uint8_t* dig = r.skip(32, 1);
    if (stored) *stored = dig;
    const uint8_t* vc = r.p;
    const uint8_t* at[3];
    uint64_t head[4];
    r.skip(3, 8);  // SplitMultiRoundR1CSShape: num_cons, num_cons_unpadded, num_rounds,
    for (int v = 0; v < 3; ++v) r.skip(r.u64(), 8);  // three Vec<usize>,
    r.skip(2, 8);                                    // num_public, width,
    for (int m = 0; m < 3; ++m) r.matrix_vecs(at, head);
    r.skip(3, 8);  // R1CSShape: num_cons, num_vars, num_io
    for (int m = 0; m < 3; ++m) r.matrix_vecs(at, head);
    hash(vc, (size_t)(r.p - vc));
    const uint8_t* key = r.p;
    r.hyrax_key();
    if (r.left()) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "wire: trailing bytes");
    hash(key, (size_t)(r.p - key));  // vc_ck,
    hash(key, (size_t)(r.p - key));  // and again for vc_vk
  }
  ck(sp_wire_digest(sink.w, out), "vk digest");
}

// Writing: setup keeps neither circuit (its time and memory stay what they were), so the caller hands both again; they are padded and equalized as nn_setup
// does, and the bytes are returned only if they hash to the key's digest - other circuits than those the key was set up from are refused.
static void nn_refuse_loaded(const NNZkKey& pk, const char* who) {
  if (pk.from_bytes) throw Error(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": a key loaded from its bytes (keep those)");
}
static std::vector<uint8_t> nn_key_to_bytes(const NNZkKey& pk, const R1CSIntView& Rs, const R1CSIntView& Rc, bool prover) {
  const char* who = prover ? "pk_to_bytes" : "vk_to_bytes";
  nn_refuse_loaded(pk, who);
  PaddedShape Ps = pad_shape(Rs), Pc = pad_shape(Rc);
  equalize(Ps, Pc);
  sp_wire* w = nullptr;
  ck(sp_wire_new(0, &w), "wire_new");
  std::unique_ptr<sp_wire, void (*)(sp_wire*)> guard(w, sp_wire_free);
  const uint64_t *g = u64p(&pk.gens[0].x), *h = u64p(&pk.gens[DEFAULT_COMMITMENT_WIDTH].x), *vh = u64p(&pk.gens[32].x);
  ck(sp_wire_hyrax_key(w, g, DEFAULT_COMMITMENT_WIDTH, h), "wire ck");
  if (!prover) ck(sp_wire_hyrax_key(w, g, DEFAULT_COMMITMENT_WIDTH, h), "wire vk_ee");
  sp_csr cs[3];
  padded_csr(Ps, cs);
  ck(sp_wire_shape(w, &Ps.dims, &cs[0], &cs[1], &cs[2], 0), "wire S_step");
  padded_csr(Pc, cs);
  ck(sp_wire_shape(w, &Pc.dims, &cs[0], &cs[1], &cs[2], 0), "wire S_core");
  if (prover) ck(sp_wire_raw(w, pk.vk_digest, 32), "wire vk_digest");
  pk.vc.write_bincode(w, false);
  pk.vc.write_bincode(w, true);
  ck(sp_wire_hyrax_key(w, g, 32, vh), "wire vc_ck");
  if (!prover) ck(sp_wire_hyrax_key(w, g, 32, vh), "wire vc_vk");
  std::vector<uint8_t> out(sp_wire_len(w));
  ck(sp_wire_bytes(w, out.data(), out.size()), "wire_bytes");
  uint8_t dig[32];
  nn_vk_digest_from_bytes(out.data(), out.size(), prover, dig);
  if (memcmp(dig, pk.vk_digest, 32) != 0)
    throw Error(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": the circuits are not those this key was set up from (digest mismatch)");
  return out;
}
// the length of that stream from the circuits' sizes alone (the sizing pass of the two-pass protocol)
static size_t nn_key_bytes_len(const NNZkKey& pk, const R1CSIntView& Rs, const R1CSIntView& Rc, bool prover) {
  nn_refuse_loaded(pk, prover ? "pk_to_bytes" : "vk_to_bytes");
  sp_wire* w = nullptr;
  ck(sp_wire_new(0, &w), "wire_new");
  std::unique_ptr<sp_wire, void (*)(sp_wire*)> guard(w, sp_wire_free);
  pk.vc.write_bincode(w, false);
  pk.vc.write_bincode(w, true);
  const size_t rows = std::max(next_pow2(Rs.num_cons), next_pow2(Rc.num_cons)), keys = prover ? 1 : 2;
  size_t n = keys * (16 + 64 * DEFAULT_COMMITMENT_WIDTH + 96) + keys * (16 + 64 * 32 + 96) + sp_wire_len(w) + (prover ? 32 : 0);
  for (const R1CSIntView* R : {&Rs, &Rc}) {
    n += 80;
    for (int m = 0; m < 3; ++m) n += 8 + 40 * (size_t)R->m[m].indptr[R->num_cons] + 8 + 8 + 8 * (rows + 1) + 8;
  }
  return n;
}

// Reading: ONE loader behind both keys, as key_from_bytes is for Spartan's. ck through sp_unwire_hyrax_key (DEFAULT_COMMITMENT_WIDTH wide); a verifier's
// vk_ee must be ck byte for byte; S_step and S_core through sp_shape_from_wire, twice on the one cursor - row-only for a verifier (verify and verify_batch
// read the shapes through sp_shape_matrix_evals_batched alone), full for a prover, the decode form by `flags` = SP_SHAPE_WIRE_* under the exclusions of the
// Spartan loaders; a prover's stored digest; the two verifier-circuit shapes, which are a function of (nb, nx, ny, width): they are rebuilt from
// nb = ceil(log2 num_steps) and S_step's nx and ny and compared byte for byte, never parsed into matrices - so one key serves every step count with the same
// nb, as the reference's does (it fixes num_rounds_b alone); vc_ck (32 wide; a verifier's vc_vk equal to it), whose generators the key keeps as the bytes
// give them; no trailing bytes. The checks are the post-conditions of SplitR1CSShape::equalize and the refusals of nn_setup. The digest is hashed from the
// bytes on a helper thread under the device work; a prover compares it with the stored one unless SS_PK_TRUST_DIGEST takes that as the reference's
// Deserialize does. Every refusal frees what the load had allocated (the key's destructor).
// which form of the row-only / full shapes a load without a forcing flag takes: measured at config 3's shapes (profiles/nn_keys.md) by the rule of
// profiles/verifier_key.md - the device form only if its median lies below the host form's minimum
static constexpr bool NN_VK_DEVICE_DEFAULT = true;
static constexpr bool NN_PK_FULL_DEVICE_DEFAULT = true;
// host wall-clock of the calling thread's last load, ms (nnz_key_stages): ck (and vk_ee) read, S_step, S_core, the verifier-circuit shapes rebuilt and
// compared + vc_ck read, the two sp_ck_create, the digest on its helper thread, the wait for it behind everything else, the whole call
static thread_local double g_nn_key_stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};

static NNZkKey* nn_key_from_bytes(sp_ctx* ctx, const uint8_t* bytes, size_t n, size_t num_steps, unsigned flags, bool prover) {
  const std::string who_s = prover ? "nnz_prover_from_bytes" : "nnz_verifier_from_bytes";
  auto refuse = [&](const std::string& what) -> Error { return Error(SP_ERR_INVALID_INPUT_LENGTH, who_s + ": " + what); };
  for (double& x : g_nn_key_stage_ms) x = 0;
  const double t_start = nn_now_ms();
  if (!ctx || !bytes || n == 0) throw refuse("null context, null bytes or no bytes");
  if (num_steps < 2) throw refuse("num_steps: at least two step circuits (the verifier circuit has no NIFS round to take its claim from)");
  bool trust_digest = false;
  if (!prover) {
    if (flags & (SP_SHAPE_WIRE_FULL | SP_SHAPE_WIRE_FULL_DEVICE)) throw refuse("a verifier's key holds the row-only shapes");
    if (!(flags & (SP_SHAPE_WIRE_DEVICE | SP_SHAPE_WIRE_HOST))) flags |= NN_VK_DEVICE_DEFAULT ? SP_SHAPE_WIRE_DEVICE : SP_SHAPE_WIRE_HOST;
  } else {
    trust_digest = flags & SS_PK_TRUST_DIGEST;
    flags &= ~(unsigned)SS_PK_TRUST_DIGEST;
    if (flags & (SP_SHAPE_WIRE_DEVICE | SP_SHAPE_WIRE_HOST)) throw refuse("a prover's key holds the full shapes (SP_SHAPE_WIRE_FULL_DEVICE or SP_SHAPE_WIRE_FULL)");
    if (!(flags & (SP_SHAPE_WIRE_FULL_DEVICE | SP_SHAPE_WIRE_FULL))) flags |= NN_PK_FULL_DEVICE_DEFAULT ? SP_SHAPE_WIRE_FULL_DEVICE : SP_SHAPE_WIRE_FULL;
  }
  auto pk = std::make_unique<NNZkKey>();
  pk->ctx = ctx;
  pk->num_steps = num_steps;
  pk->verifier_only = !prover;
  pk->from_bytes = true;
  ck(sp_ctx_bind_thread(ctx), "device");
  sp_unwire* r = nullptr;
  ck(sp_unwire_new(bytes, n, &r), "unwire_new");
  std::unique_ptr<sp_unwire, void (*)(sp_unwire*)> guard(r, sp_unwire_free);
  auto at = [&] { return n - sp_unwire_left(r); };  // the cursor's offset
  auto named = [&](int rc, const char* field) {
    if (rc != SP_OK) throw Error(rc, who_s + ": " + field + ": " + sp_last_error());
  };
  auto read_key = [&](std::vector<aff_t>& gens, size_t want_cols, const char* field) {
    size_t nc = 0;
    named(sp_unwire_hyrax_key(r, nullptr, 0, &nc, nullptr), field);
    if (nc != want_cols) throw refuse(std::string(field) + ": num_cols is " + std::to_string(nc) + ", this build's is " + std::to_string(want_cols));
    gens.resize(nc + 1);
    named(sp_unwire_hyrax_key(r, u64p(&gens[0].x), nc, &nc, u64p(&gens[nc].x)), field);
  };
  auto same_key_again = [&](size_t from, const char* field, const char* as) {  // the next `len` bytes are the key at `from` once more
    const size_t len = at() - from;
    if (sp_unwire_left(r) < len) throw refuse(std::string(field) + ": wire: unexpected end of input");
    if (memcmp(bytes + from, bytes + from + len, len) != 0) throw refuse(std::string(field) + " is not " + as + " (for Hyrax the two are the same generators)");
    std::vector<uint64_t> over(len / 8);
    named(sp_unwire_u64s(r, over.size(), over.data()), field);
  };
  read_key(pk->gens, DEFAULT_COMMITMENT_WIDTH, "ck");
  if (!prover) same_key_again(0, "vk_ee", "ck");
  const double t_keys = nn_now_ms();
  // the digest needs the bytes alone
  double digest_ms = 0;
  const uint8_t* stored_digest = nullptr;
  std::future<void> digest = std::async(trust_digest ? std::launch::deferred : std::launch::async, [&] {
    if (trust_digest) return;
    const double t0 = nn_now_ms();
    nn_vk_digest_from_bytes(bytes, n, prover, pk->vk_digest);
    digest_ms = nn_now_ms() - t0;
  });
  struct Join {
    std::future<void>& f;
    ~Join() {
      if (f.valid()) f.wait();
    }
  } join{digest};
  named(sp_shape_from_wire(ctx, r, flags, &pk->dims, &pk->S_step), "S_step");
  const double t_step = nn_now_ms();
  named(sp_shape_from_wire(ctx, r, flags, &pk->dims_core, &pk->S_core), "S_core");
  const double t_core = nn_now_ms();
  if (prover) {
    if (sp_unwire_left(r) < 32) throw refuse("vk_digest: wire: unexpected end of input");
    stored_digest = bytes + at();
    uint64_t over[4];
    named(sp_unwire_u64s(r, 4, over), "vk_digest");
  }
  const sp_dims &d = pk->dims, &dc = pk->dims_core;
  const size_t nv = d.num_shared + d.num_precommitted + d.num_rest, nvc = dc.num_shared + dc.num_precommitted + dc.num_rest;
  // SplitR1CSShape::new pads to powers of two (the sum-checks and the layout count rounds from them) ...
  if (next_pow2(d.num_cons) != d.num_cons || next_pow2(nv) != nv) throw refuse("S_step: num_cons or the padded variable total is no power of two");
  // ... and equalize (src/r1cs/mod.rs:913-971) leaves both shapes with the larger constraint count and the larger variable total
  if (d.num_cons != dc.num_cons) throw refuse("S_core: num_cons is " + std::to_string(dc.num_cons) + ", S_step's is " + std::to_string(d.num_cons) + " (the shapes are not equalized)");
  if (nv != nvc) throw refuse("S_core: the padded variable total is " + std::to_string(nvc) + ", S_step's is " + std::to_string(nv) + " (the shapes are not equalized)");
  // the refusals of nn_setup
  if (d.num_shared != dc.num_shared) throw refuse("S_core: num_shared: step and core circuits with different padded shared segments (one shared commitment serves both)");
  if (d.num_challenges || dc.num_challenges) throw refuse(std::string(d.num_challenges ? "S_step" : "S_core") + ": num_challenges: step / core circuits with verifier challenges are not driven by this layer");
  if (d.num_rest_unpadded && d.num_shared + d.num_precommitted)
    throw refuse("S_step: num_rest_unpadded: step circuits with rest variables beside shared / precommitted ones (the reference's fold drops the rest segment)");
  pk->num_vars = nv;
  pk->nb = log2_ceil(next_pow2(num_steps));
  pk->nx = log2_ceil(d.num_cons);
  pk->ny = log2_ceil(nv) + 1;
  pk->vc = vcirc::Shape::from_circuit(vcirc::Circuit(pk->nb, pk->nx, pk->ny, 32));
  {
    sp_wire* w = nullptr;
    ck(sp_wire_new(0, &w), "wire_new");
    std::unique_ptr<sp_wire, void (*)(sp_wire*)> wguard(w, sp_wire_free);
    size_t from = 0;
    for (int regular = 0; regular < 2; ++regular) {
      const char* field = regular ? "vc_shape_regular" : "vc_shape";
      pk->vc.write_bincode(w, regular != 0);
      std::vector<uint8_t> want(sp_wire_len(w));
      ck(sp_wire_bytes(w, want.data(), want.size()), "wire_bytes");
      const size_t len = want.size() - from;
      if (sp_unwire_left(r) < len) throw refuse(std::string(field) + ": wire: unexpected end of input");
      if (memcmp(bytes + at(), want.data() + from, len) != 0)
        throw refuse(std::string(field) + ": not the verifier circuit of nb = " + std::to_string(pk->nb) + " (num_steps = " + std::to_string(num_steps) + "), nx = " +
                     std::to_string(pk->nx) + ", ny = " + std::to_string(pk->ny) + ", width 32");
      std::vector<uint64_t> over(len / 8);
      named(sp_unwire_u64s(r, over.size(), over.data()), field);
      from = want.size();
    }
  }
  const size_t vc_ck_at = at();
  read_key(pk->vc_gens, 32, "vc_ck");
  if (!prover) same_key_again(vc_ck_at, "vc_vk", "vc_ck");
  named(sp_unwire_done(r), prover ? "behind vc_ck" : "behind vc_vk");
  pk->layout = NNLayout(pk->dims, pk->dims_core, num_steps, pk->vc);
  const double t_vc = nn_now_ms();
  ck(sp_ck_create(ctx, u64p(&pk->gens[0].x), DEFAULT_COMMITMENT_WIDTH, u64p(&pk->gens[DEFAULT_COMMITMENT_WIDTH].x), &pk->ck), "ck_create");
  ck(sp_ck_create(ctx, u64p(&pk->vc_gens[0].x), 32, u64p(&pk->vc_gens[32].x), &pk->vc_ck), "vc_ck_create");
  const double t_ck = nn_now_ms();
  try {
    digest.get();
  } catch (const Error& e) {
    throw Error(e.code, who_s + ": the digest pass could not walk the bytes: " + e.what());
  }
  if (trust_digest) memcpy(pk->vk_digest, stored_digest, 32);
  else if (prover && memcmp(pk->vk_digest, stored_digest, 32) != 0)
    throw refuse("vk_digest: the stored digest is not the digest of the key's bytes (a prover under it makes proofs no verifier accepts)");
  const double t_end = nn_now_ms();
  const double st[8] = {t_keys - t_start, t_step - t_keys, t_core - t_step, t_vc - t_core, t_ck - t_vc, digest_ms, t_end - t_ck, t_end - t_start};
  std::copy(st, st + 8, g_nn_key_stage_ms);
  return pk.release();
}
// the prover entry points take the key through this: a verifier's key holds row-only shapes
static NNZkKey& nn_prover_key(void* pk, const char* who) {
  auto* k = (NNZkKey*)pk;
  if (k && k->verifier_only)
    throw Error(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": verifier-only key (loaded by nnz_verifier_from_bytes; proving takes the key of nnz_setup or nnz_prover_from_bytes)");
  return *k;
}

// The witness of one circuit as a device table [shared | precommitted | rest] at the padded offsets (bellpepper/r1cs.rs:306-409): the machine words cross the bus
// as they are and become Montgomery-form elements on the device (sp_table_write_u64). `shared_words`: step 0's shared segment - every circuit of a batch
// carries it (src/neutronnova_zk.rs:1485-1488).
static void upload_witness(sp_ctx* ctx, const sp_dims& d, const uint64_t* w, const uint64_t* shared_words, size_t shared_count, sp_table* out) {
  ck(sp_table_write_u64(ctx, out, 0, shared_words, shared_count), "upload W (shared)");
  ck(sp_table_write_u64(ctx, out, d.num_shared, w + d.num_shared_unpadded, d.num_precommitted_unpadded), "upload W (precommitted)");
  ck(sp_table_write_u64(ctx, out, d.num_shared + d.num_precommitted, w + d.num_shared_unpadded + d.num_precommitted_unpadded, d.num_rest_unpadded), "upload W (rest)");
}

// prep_prove (:1477-1603) behind its witness source: shared commitment from step 0's shared segment (`shared_words`), one precommitted commitment per step
// and for the core. `fill_W(Ws)` writes the witnesses into the zeroed tables Ws[0 .. n) (the steps) and Ws[n] (the core); the blinds are drawn from the
// tape in the same order whichever source fills them: machine words from the frontend (nn_prep_prove) or the SHA-256 witness kernel (nn_prep_prove_sha256).
static NNZkPrep* nn_prep_prove_from(const NNZkKey& pk, size_t n, const uint64_t* shared_words, const uint64_t* step_pub, size_t npub, const uint64_t* core_pub, bool is_small,
                                    Tape& tape, const std::function<void(sp_table* const* Ws)>& fill_W) {
  const sp_dims& d = pk.dims;
  auto* ps = new NNZkPrep();
  try {
    sp_ctx* ctx = pk.ctx;
    const size_t CW = DEFAULT_COMMITMENT_WIDTH, rows_sh = d.num_shared / CW;
    ps->is_small = is_small;
    ps->steps.resize(n);
    if (d.num_shared_unpadded) {
      ps->r_shared.resize(rows_sh);
      for (auto& b : ps->r_shared) b = tape.next();
      sp_table* t = nullptr;
      ck(sp_table_zeros(ctx, d.num_shared, (size_t)-1, (size_t)-1, &t), "alloc shared");
      int rc = sp_table_write_u64(ctx, t, 0, shared_words, d.num_shared_unpadded);
      ps->comm_shared.resize(rows_sh);
      if (!rc) rc = sp_hyrax_commit(ctx, pk.ck, t, 0, d.num_shared, u64p(ps->r_shared.data()), is_small ? 1 : 0, u64p(&ps->comm_shared[0].x));
      sp_table_free(t);
      ck(rc, "commit shared");
    }
    {
      std::vector<sp_table*> Ws(n + 1);
      for (size_t i = 0; i <= n; ++i) {
        const sp_dims& dd = i < n ? d : pk.dims_core;
        NNPre* p = i < n ? &ps->steps[i] : &ps->core;
        ck(sp_table_zeros(ctx, dd.num_shared + dd.num_precommitted + dd.num_rest, (size_t)-1, (size_t)-1, &p->W), "alloc W");
        Ws[i] = p->W;
      }
      fill_W(Ws.data());
    }
    auto precommit = [&](const sp_dims& dd, const uint64_t* pub, NNPre* p) {
      p->publics.resize(dd.num_public);
      for (size_t i = 0; i < dd.num_public; ++i) p->publics[i] = fe_from_u64<S>(pub[i]);
      if (dd.num_precommitted_unpadded) {
        const size_t rows_pre = dd.num_precommitted / CW;
        p->r_pre.resize(rows_pre);
        for (auto& b : p->r_pre) b = tape.next();
        p->comm_pre.resize(rows_pre);
        ck(sp_hyrax_commit(ctx, pk.ck, p->W, dd.num_shared, dd.num_precommitted, u64p(p->r_pre.data()), is_small ? 1 : 0, u64p(&p->comm_pre[0].x)), "commit precommitted");
      }
    };
    for (size_t i = 0; i < n; ++i) precommit(d, step_pub + i * npub, &ps->steps[i]);
    precommit(pk.dims_core, core_pub, &ps->core);
    {  // can_cache_matvec (:1523) always holds here: nn_setup rejects rest variables and challenges, so z = [W | 1 | X] is fully known
      std::vector<fe_t> X(n * d.num_public);
      std::vector<const sp_table*> Ws(n);
      for (size_t i = 0; i < n; ++i) {
        std::copy(ps->steps[i].publics.begin(), ps->steps[i].publics.end(), X.begin() + i * d.num_public);
        Ws[i] = ps->steps[i].W;
      }
      ps->nifs_cached = nifs_prepare(ctx, pk.S_step, d, n, X.data(), Ws.data(), true);
    }
  } catch (...) {
    delete ps;
    throw;
  }
  return ps;
}

static NNZkPrep* nn_prep_prove(const NNZkKey& pk, size_t n, const uint64_t* step_wit, size_t wit_len, const uint64_t* step_pub, size_t npub, const uint64_t* core_wit,
                               const uint64_t* core_pub, bool is_small, Tape& tape) {
  const sp_dims& d = pk.dims;
  if (n != pk.num_steps || wit_len != d.num_shared_unpadded + d.num_precommitted_unpadded + d.num_rest_unpadded || npub != d.num_public)
    throw Error(SP_ERR_INVALID_WITNESS_LENGTH, "InvalidWitnessLength");
  sp_ctx* ctx = pk.ctx;
  return nn_prep_prove_from(pk, n, step_wit, step_pub, npub, core_pub, is_small, tape, [&](sp_table* const* Ws) {
    // every circuit shares step 0's shared witness (:1485-1488)
    for (size_t i = 0; i < n; ++i) upload_witness(ctx, d, step_wit + i * wit_len, step_wit, d.num_shared_unpadded, Ws[i]);
    upload_witness(ctx, pk.dims_core, core_wit, step_wit, d.num_shared_unpadded, Ws[n]);
  });
}

// prep_prove for Sha256StepCircuit / CoreCircuit (benches/sha256_neutronnova.rs:49-183) with the witnesses generated on the device: the reference synthesises
// every step inside prep_prove (src/neutronnova_zk.rs:1487-1518); here all n step witnesses and the core circuit's (the same plan on the zero block, :161-182)
// are ONE sp_sha256_witness launch. blocks = n x 64 bytes; the circuits' one public value is x = 0.
// the key is a Sha256StepCircuit / CoreCircuit key of `n` steps and `plan` the step circuit's witness plan
static void check_sha256_step_key(const NNZkKey& pk, const sp_sha256_plan* plan, size_t n) {
  const sp_dims &d = pk.dims, &dc = pk.dims_core;
  uint64_t info[5];
  ck(sp_sha256_plan_info(plan, info), "plan info");
  if (n != pk.num_steps || d.num_shared_unpadded != 0 || d.num_rest_unpadded != 0 || dc.num_shared_unpadded != 0 || dc.num_rest_unpadded != 0 ||
      info[0] != d.num_precommitted_unpadded || info[0] != dc.num_precommitted_unpadded)
    throw Error(SP_ERR_INVALID_WITNESS_LENGTH, "InvalidWitnessLength: the plan's variable count is not the key's");
  if (info[3] != 64 || info[4] || d.num_public != 1 || dc.num_public != 1 || d.num_shared != dc.num_shared)
    throw Error(SP_ERR_INVALID_INPUT_LENGTH, "not the step circuit's plan / key");
}
static NNZkPrep* nn_prep_prove_sha256(const NNZkKey& pk, const sp_sha256_plan* plan, const uint8_t* blocks, size_t n, bool is_small, Tape& tape) {
  const sp_dims& d = pk.dims;
  check_sha256_step_key(pk, plan, n);
  sp_ctx* ctx = pk.ctx;
  const std::vector<uint64_t> zeros(n + 1, 0);  // x = 0 for every step and the core
  return nn_prep_prove_from(pk, n, nullptr, zeros.data(), 1, zeros.data(), is_small, tape, [&](sp_table* const* Ws) {
    std::vector<uint8_t> msgs(64 * (n + 1), 0);  // the core circuit: the zero block
    memcpy(msgs.data(), blocks, 64 * n);
    ck(sp_sha256_witness(ctx, plan, msgs.data(), 64, n + 1, Ws, d.num_shared, nullptr), "sha256 witness");
  });
}

// prep_prove (:1477-1603) for `count` states of one key, phase by phase over all of them (one state included): state k is word for word the state
// nn_prep_prove_from makes of input k with tape k - the same blinds in the same order (shared, step 0 .. n-1, core), the same commitments (canonical affine
// points), the same layers (exact field sums) and mirrors, the same tape blocks used - because none of them depends on how the work was grouped.
//   blinds       all of state k's, from tape k, before any device work
//   witnesses    fill_W(Ws): the zeroed tables of state k are Ws[k (n + 1) .. + n) (its steps) and Ws[k (n + 1) + n] (its core)
//   commitments  sp_hyrax_commit_batch over the K shared segments (step 0's table of every state), over the K n step tables' precommitted segment and
//                over the K core tables' - the cores ride in the step call when both circuits pad the segments alike (the (2, 30, 2) key does not)
//   layers       one sp_nifs_create per state, ONE sp_nifs_layers_batch for all states (no z is assembled), sp_nifs_prepare_small per state
//   one synchronise
// flags: NNZ_PREP_PER_STATE_COMMIT = one sp_hyrax_commit per polynomial, NNZ_PREP_PER_STATE_LAYERS = nifs_prepare per state - nn_prep_prove_from's calls;
// NNZ_PREP_SHARED_COMMIT / NNZ_PREP_SHARED_LAYERS ask for the shared stage whatever the default is (a per-state flag wins over them) - there so that one
// process can compare the forms (tools/nn_prep_batch_timing.py). What the driver takes by default - the shared stage from NN_PREP_SHARED_*_MIN states
// on - was measured: profiles/nn_prep_prove_batch.md.
// step_pub(k) / core_pub(k): the public values of state k (n x npub and the core's) as machine words. An error names the state at fault; every state made
// so far goes with it. phase_ms (8, optional): blinds + allocations, witnesses, commitments, layers, mirrors, synchronise, total.
enum : unsigned { NNZ_PREP_PER_STATE_COMMIT = 1, NNZ_PREP_PER_STATE_LAYERS = 2, NNZ_PREP_SHARED_COMMIT = 4, NNZ_PREP_SHARED_LAYERS = 8 };
// Measured at config 3 (32 steps + core), one process, legs alternating, ms a batch: with both stages shared 0.86 / 3.50 / 14.49 (median) at K = 1 / 4 / 16;
// with one sp_hyrax_commit per polynomial 7.80 / 31.33 / 125.56 (minimum), with nifs_prepare per state 1.64 / 6.48 / 26.03 (minimum); the loop of single
// calls 8.62 / 34.99 / 141.80. Both shared stages are below the per-state forms' minima at every K, one state included (it is a batch of n + 1 polynomials
// and n_padded layers already): both are the default from one state on.
static constexpr size_t NN_PREP_SHARED_COMMIT_MIN = 1, NN_PREP_SHARED_LAYERS_MIN = 1;  // (size_t)-1 = never by default
static std::vector<NNZkPrep*> nn_prep_prove_batch_from(const NNZkKey& pk, size_t count, bool is_small, Tape* tapes, unsigned flags,
                                                       const std::function<const uint64_t*(size_t)>& step_pub, const std::function<const uint64_t*(size_t)>& core_pub,
                                                       const std::function<void(sp_table* const* Ws)>& fill_W, double* phase_ms) {
  const sp_dims &d = pk.dims, &dc = pk.dims_core;
  const size_t n = pk.num_steps, CW = DEFAULT_COMMITMENT_WIDTH;
  std::vector<std::unique_ptr<NNZkPrep>> st(count);
  size_t at = (size_t)-1;  // the state a per-state step is working on (names the state in an error)
  try {
    sp_ctx* ctx = pk.ctx;
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    double t_last = t_begin;
    auto phase = [&](int k) {
      const double t = now();
      ms[k] += t - t_last;
      t_last = t;
    };
    const bool batch_commit = !(flags & NNZ_PREP_PER_STATE_COMMIT) && ((flags & NNZ_PREP_SHARED_COMMIT) || count >= NN_PREP_SHARED_COMMIT_MIN);
    const bool batch_layers = !(flags & NNZ_PREP_PER_STATE_LAYERS) && ((flags & NNZ_PREP_SHARED_LAYERS) || count >= NN_PREP_SHARED_LAYERS_MIN);
    // 1. blinds (PCS::blind, hyrax_pc.rs:192-205) and public values
    const size_t rows_sh = d.num_shared_unpadded ? d.num_shared / CW : 0, rows_step = d.num_precommitted_unpadded ? d.num_precommitted / CW : 0,
                 rows_core = dc.num_precommitted_unpadded ? dc.num_precommitted / CW : 0;
    for (at = 0; at < count; ++at) {
      st[at].reset(new NNZkPrep());
      NNZkPrep* ps = st[at].get();
      ps->is_small = is_small;
      ps->steps.resize(n);
      ps->r_shared.resize(rows_sh);
      for (auto& b : ps->r_shared) b = tapes[at].next();
      ps->comm_shared.resize(rows_sh);
      const uint64_t *sp = step_pub(at), *cp = core_pub(at);
      for (size_t i = 0; i <= n; ++i) {
        NNPre& p = i < n ? ps->steps[i] : ps->core;
        const sp_dims& dd = i < n ? d : dc;
        p.publics.resize(dd.num_public);
        for (size_t j = 0; j < dd.num_public; ++j) p.publics[j] = fe_from_u64<S>(i < n ? sp[i * d.num_public + j] : cp[j]);
        p.r_pre.resize(i < n ? rows_step : rows_core);
        for (auto& b : p.r_pre) b = tapes[at].next();
        p.comm_pre.resize(p.r_pre.size());
      }
    }
    std::vector<sp_table*> Ws(count * (n + 1));
    for (at = 0; at < count; ++at)
      for (size_t i = 0; i <= n; ++i) {
        const sp_dims& dd = i < n ? d : dc;
        NNPre& p = i < n ? st[at]->steps[i] : st[at]->core;
        ck(sp_table_zeros(ctx, dd.num_shared + dd.num_precommitted + dd.num_rest, (size_t)-1, (size_t)-1, &p.W), "alloc W");
        Ws[at * (n + 1) + i] = p.W;
      }
    at = (size_t)-1;
    phase(0);
    // 2. witnesses
    fill_W(Ws.data());
    phase(1);
    // 3. commitments
    struct Poly {
      const sp_table* W;
      const fe_t* blinds;
      aff_t* out;
      size_t state;
    };
    auto commit = [&](const std::vector<Poly>& ps, size_t off, size_t len, const char* what) {
      if (ps.empty() || !len) return;
      if (batch_commit) {
        std::vector<const sp_table*> v(ps.size());
        std::vector<const uint64_t*> bl(ps.size());
        std::vector<uint64_t*> out(ps.size());
        for (size_t j = 0; j < ps.size(); ++j) v[j] = ps[j].W, bl[j] = u64p(ps[j].blinds), out[j] = u64p(&ps[j].out[0].x);
        ck(sp_hyrax_commit_batch(ctx, pk.ck, ps.size(), v.data(), off, len, bl.data(), out.data()), what);
        return;
      }
      for (const Poly& p : ps) {
        at = p.state;
        ck(sp_hyrax_commit(ctx, pk.ck, p.W, off, len, u64p(p.blinds), is_small ? 1 : 0, u64p(&p.out[0].x)), what);
      }
      at = (size_t)-1;
    };
    std::vector<Poly> shared, steps, cores;
    for (size_t k = 0; k < count; ++k) {
      NNZkPrep* ps = st[k].get();
      if (rows_sh) shared.push_back(Poly{ps->steps[0].W, ps->r_shared.data(), ps->comm_shared.data(), k});  // every circuit carries step 0's shared segment
      if (rows_step)
        for (NNPre& p : ps->steps) steps.push_back(Poly{p.W, p.r_pre.data(), p.comm_pre.data(), k});
      if (rows_core) cores.push_back(Poly{ps->core.W, ps->core.r_pre.data(), ps->core.comm_pre.data(), k});
    }
    if (batch_commit && rows_step && dc.num_shared == d.num_shared && dc.num_precommitted == d.num_precommitted) {
      steps.insert(steps.end(), cores.begin(), cores.end());
      cores.clear();
    }
    commit(shared, 0, d.num_shared, "commit shared");
    commit(steps, d.num_shared, d.num_precommitted, "commit precommitted");
    commit(cores, dc.num_shared, dc.num_precommitted, "commit precommitted (core)");
    phase(2);
    // 4. layers: can_cache_matvec (:1523) always holds here (nn_setup rejects rest variables beside committed ones and challenges): z = [W | 1 | X] is known
    std::vector<fe_t> X(count * n * d.num_public);
    std::vector<const sp_table*> Wsteps(count * n);
    for (size_t k = 0; k < count; ++k)
      for (size_t i = 0; i < n; ++i) {
        std::copy(st[k]->steps[i].publics.begin(), st[k]->steps[i].publics.end(), X.begin() + (k * n + i) * d.num_public);
        Wsteps[k * n + i] = st[k]->steps[i].W;
      }
    if (batch_layers) {
      size_t n_padded = 2, ell_cons, left, right;
      while (n_padded < n) n_padded <<= 1;
      compute_tensor_decomp(d.num_cons, &ell_cons, &left, &right);
      std::vector<sp_nifs*> nifs(count);
      for (at = 0; at < count; ++at) {
        ck(sp_nifs_create(ctx, n_padded, left, right, &st[at]->nifs_cached), "nifs_create");
        nifs[at] = st[at]->nifs_cached;
      }
      at = (size_t)-1;
      ck(sp_nifs_layers_batch(ctx, pk.S_step, count, nifs.data(), n, Wsteps.data(), u64p(X.data())), "nifs layers");
      phase(3);
      for (at = 0; at < count; ++at) ck(sp_nifs_prepare_small(nifs[at]), "prepare_small");
      phase(4);
    } else {
      for (at = 0; at < count; ++at) st[at]->nifs_cached = nifs_prepare(ctx, pk.S_step, d, n, X.data() + at * n * d.num_public, Wsteps.data() + at * n, true);
      phase(3);
    }
    at = (size_t)-1;
    ck(sp_ctx_synchronize(ctx), "sync");
    phase(5);
    ms[6] = now() - t_begin;
    if (phase_ms) memcpy(phase_ms, ms, sizeof ms);
  } catch (const Error& e) {
    // every state made so far goes with `st`
    throw Error(e.code, std::string("prep_prove_batch: ") + (at == (size_t)-1 ? std::string() : "state " + std::to_string(at) + ": ") + e.what());
  }
  std::vector<NNZkPrep*> out(count);
  for (size_t k = 0; k < count; ++k) out[k] = st[k].release();
  return out;
}

// the batch from the frontend's machine words: state k = n x wit_len step words, the core's words, the public values
static std::vector<NNZkPrep*> nn_prep_prove_batch(const NNZkKey& pk, size_t count, const size_t* n, const uint64_t* const* step_wit, const size_t* wit_len,
                                                  const uint64_t* const* step_pub, size_t npub, const uint64_t* const* core_wit, const uint64_t* const* core_pub, bool is_small,
                                                  Tape* tapes, unsigned flags, double* phase_ms) {
  const sp_dims& d = pk.dims;
  const size_t want = d.num_shared_unpadded + d.num_precommitted_unpadded + d.num_rest_unpadded, ns = pk.num_steps;
  for (size_t k = 0; k < count; ++k) {
    if (n[k] != ns || wit_len[k] != want || npub != d.num_public)
      throw Error(SP_ERR_INVALID_WITNESS_LENGTH, "prep_prove_batch: state " + std::to_string(k) + ": InvalidWitnessLength");
    if (!step_wit[k] || !core_wit[k] || (npub && !step_pub[k]) || (pk.dims_core.num_public && !core_pub[k]))
      throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: state " + std::to_string(k) + ": null witness");
  }
  sp_ctx* ctx = pk.ctx;
  return nn_prep_prove_batch_from(
      pk, count, is_small, tapes, flags, [&](size_t k) { return step_pub[k]; }, [&](size_t k) { return core_pub[k]; },
      [&](sp_table* const* Ws) {
        for (size_t k = 0; k < count; ++k) {  // every circuit of a state shares its step 0's shared witness (:1485-1488)
          for (size_t i = 0; i < ns; ++i) upload_witness(ctx, d, step_wit[k] + i * want, step_wit[k], d.num_shared_unpadded, Ws[k * (ns + 1) + i]);
          upload_witness(ctx, pk.dims_core, core_wit[k], step_wit[k], d.num_shared_unpadded, Ws[k * (ns + 1) + ns]);
        }
      },
      phase_ms);
}

// the batch for Sha256StepCircuit / CoreCircuit keys: blocks[k] = the n[k] 64-byte blocks of state k; the witnesses of all K (n + 1) circuits - every state's
// core is the zero block - are ONE sp_sha256_witness launch
static std::vector<NNZkPrep*> nn_prep_prove_sha256_batch(const NNZkKey& pk, const sp_sha256_plan* plan, size_t count, const uint8_t* const* blocks, const size_t* n, bool is_small,
                                                         Tape* tapes, unsigned flags, double* phase_ms) {
  const size_t ns = pk.num_steps;
  for (size_t k = 0; k < count; ++k) {
    if (n[k] != ns) throw Error(SP_ERR_INVALID_WITNESS_LENGTH, "prep_prove_batch: state " + std::to_string(k) + ": InvalidWitnessLength");
    if (!blocks[k]) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: state " + std::to_string(k) + ": null blocks");
  }
  check_sha256_step_key(pk, plan, ns);
  const std::vector<uint64_t> zeros(ns + 1, 0);  // x = 0 for every step and the core
  auto pub = [&](size_t) { return zeros.data(); };
  return nn_prep_prove_batch_from(
      pk, count, is_small, tapes, flags, pub, pub,
      [&](sp_table* const* Ws) {
        std::vector<uint8_t> msgs(64 * count * (ns + 1), 0);
        for (size_t k = 0; k < count; ++k) memcpy(msgs.data() + 64 * k * (ns + 1), blocks[k], 64 * ns);
        ck(sp_sha256_witness(pk.ctx, plan, msgs.data(), 64, count * (ns + 1), Ws, pk.dims.num_shared, nullptr), "sha256 witness");
      },
      phase_ms);
}

static void absorb_instance(Tr& tr, const char* label, const std::vector<aff_t>& comm, const std::vector<fe_t>& X) {  // R1CSInstance bytes (src/r1cs/mod.rs:728-736)
  std::vector<uint8_t> b = commitment_bytes(comm.data(), comm.size());
  const size_t off = b.size();
  b.resize(off + 32 * X.size());
  for (size_t j = 0; j < X.size(); ++j) sp::fe_to_be_bytes<S>(X[j], b.data() + off + 32 * j);
  tr.absorb(label, b.data(), b.size());
}
// the transcript's head, as the prover and the verifier absorb it: the key's digest and the core instance
static void absorb_head(Tr& tr, const NNZkKey& pk, const std::vector<aff_t>& core_comm, const std::vector<fe_t>& core_X) {
  tr.absorb("vk", pk.vk_digest, 32);
  absorb_instance(tr, "core_instance", core_comm, core_X);
}
// NovaNIFS (src/nifs.rs:34-77), both sides: U1, the random relaxed instance (comm_W, comm_E, u, X) ...
static void absorb_U1(Tr& tr, const aff_t* comm_W, size_t rows_W, const aff_t* comm_E, size_t rows_E, const fe_t& u, const fe_t* X, size_t nX) {
  std::vector<uint8_t> b = commitment_bytes(comm_W, rows_W), e = commitment_bytes(comm_E, rows_E);
  b.insert(b.end(), e.begin(), e.end());
  const size_t off = b.size();
  b.resize(off + 32 * (1 + nX));
  sp::fe_to_be_bytes<S>(u, b.data() + off);
  for (size_t j = 0; j < nX; ++j) sp::fe_to_be_bytes<S>(X[j], b.data() + off + 32 * (1 + j));
  tr.absorb("U1", b.data(), b.size());
}
// ... and the commitment of the cross term
static void absorb_comm_T(Tr& tr, const aff_t* comm_T, size_t rows_T) {
  const std::vector<uint8_t> b = commitment_bytes(comm_T, rows_T);
  tr.absorb("comm_T", b.data(), b.size());
}
// SPARTAN_HOST_LAPS=1 (read once per process): one stderr line per lap of a prove or a verify, "<who> lap <what> <ms since the last lap>"
struct NNLaps {
  const char* who;
  bool on = false;
  double t_lap = 0;
  static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void start(double t) {
    static const bool laps = [] {
      const char* e = getenv("SPARTAN_HOST_LAPS");
      return e && e[0] == '1';
    }();
    on = laps;
    t_lap = t;
  }
  void lap(const char* what) {
    if (!on) return;
    const double t = now();
    fprintf(stderr, "%s lap %-28s %8.3f ms\n", who, what, t - t_lap);
    t_lap = t;
  }
};
// a grow-only device table of a prep state with `len` elements: when `len` outgrows it, it is allocated again - with room to spare (at least 4096, else
// twice `len`: the scratch slots, whose users differ in size) or exactly - and its length is set. Contents are whatever its last user left.
static sp_table* grown_slot(sp_ctx* ctx, sp_table*& t, size_t& cap, size_t len, bool spare, const char* what, const char* what_len) {
  if (len > cap) {  // per slot: other slots may be in use by the caller
    sp_table_free(t);
    t = nullptr;
    cap = !spare ? len : len < 4096 ? 4096 : 2 * len;
  }
  if (!t) ck(sp_table_zeros(ctx, cap, (size_t)-1, (size_t)-1, &t), what);
  ck(sp_table_set_len(t, len, (size_t)-1, (size_t)-1), what_len);
  return t;
}
// slot `i` of the prep state's scratch tables holding `n` elements of host data
static sp_table* stage(sp_ctx* ctx, NNZkPrep& ps, int i, const fe_t* data, size_t n) {
  sp_table* t = grown_slot(ctx, ps.vws[i], ps.vws_cap[i], n, true, "scratch table", "scratch len");
  ck(sp_table_write(ctx, t, 0, u64p(data), n), "upload");
  return t;
}
// working table `i` of the prep state with `len` elements (every user writes what it reads)
static sp_table* work_table(sp_ctx* ctx, NNZkPrep& ps, int i, size_t len) { return grown_slot(ctx, ps.work[i], ps.work_cap[i], len, false, "working table", "working table len"); }
// rows of host scalars committed with the width-32 key in one device call (many rows: T, the random instance) ...
// ... by the helper thread's jobs: tables of their own, on the second context
static std::vector<aff_t> commit_rows32_side(NNZkPrep& ps, int slot, const sp_ck* vc_ck, const std::vector<fe_t>& v, const std::vector<fe_t>& blinds) {
  sp_ctx* ctx = ps.ctx2;
  sp_table* t = grown_slot(ctx, ps.bws[slot], ps.bws_cap[slot], v.size(), true, "scratch table", "scratch len");
  ck(sp_table_write(ctx, t, 0, u64p(v.data()), v.size()), "upload");
  std::vector<aff_t> out(blinds.size());
  ck(sp_hyrax_commit(ctx, vc_ck, t, 0, v.size(), u64p(blinds.data()), 0, u64p(&out[0].x)), "commit (width 32)");
  return out;
}
// ... and on the caller's context
static std::vector<aff_t> commit_rows32(sp_ctx* ctx, NNZkPrep& ps, const sp_ck* vc_ck, const std::vector<fe_t>& v, const std::vector<fe_t>& blinds, bool latency = false) {
  std::vector<aff_t> out(blinds.size());
  // the latency form (one launch through mapped memory, the rows added by the library's polling threads) where the commitment sits in the transcript chain
  if (latency && sp_walkers() > 0 && v.size() <= 32 * blinds.size() && blinds.size() * 33 <= 640 &&
      sp_hyrax_commit_rows_host(ctx, vc_ck, u64p(v.data()), v.size(), u64p(blinds.data()), u64p(&out[0].x)) == SP_OK)
    return out;
  sp_table* t = stage(ctx, ps, 0, v.data(), v.size());
  ck(sp_hyrax_commit(ctx, vc_ck, t, 0, v.size(), u64p(blinds.data()), 0, u64p(&out[0].x)), "commit (width 32)");
  return out;
}
// prove_direct (hyrax_pc.rs:609-652) on host vectors
static void prove_direct(size_t num_cols, const std::vector<fe_t>& poly, const std::vector<fe_t>& blind, const fe_t* point, size_t npoint, std::vector<fe_t>* v, fe_t* cb) {
  const size_t n = (size_t)1 << npoint, rows = (n + num_cols - 1) / num_cols;
  if (rows == 1) {
    *v = poly;
    v->resize(num_cols, fe_zero());
    *cb = blind[0];
    return;
  }
  const size_t nvr = log2_ceil(rows);
  const std::vector<fe_t> L = eq_evals_host(point, nvr);
  v->assign(num_cols, fe_zero());
  for (size_t j = 0; j < L.size(); ++j)
    for (size_t i = 0; i < num_cols; ++i) {
      const size_t k = j * num_cols + i;
      if (k < poly.size()) (*v)[i] = fe_add<S>((*v)[i], fe_mul<S>(L[j], poly[k]));
    }
  *cb = fe_zero();
  for (size_t i = 0; i < blind.size() && i < L.size(); ++i) *cb = fe_add<S>(*cb, fe_mul<S>(L[i], blind[i]));
}

// the evaluation of [1 | X | 0 ..] at r_y[1..] (the X part of z, :1921-1935 and :2290-2300)
static fe_t nn_eval_X(size_t ny, const fe_t* X, size_t cnt, const fe_t* r_y) {
  std::vector<fe_t> v{fe_one<S>()};
  v.insert(v.end(), X, X + cnt);
  return sparse_poly_evaluate(ny - 1, v, r_y + 1);
}
// out = a + w * b over n points: the fold begun on b's doubling ladders is finished (and the job consumed), else it is one call
static void fold2_finish_or_call(sp_ctx* ctx, sp_fold2_job*& job, const aff_t* a, const aff_t* b, size_t n, const fe_t& w, aff_t* out, const char* what) {
  if (job) {
    sp_fold2_job* j = job;
    job = nullptr;
    ck(sp_fold_commitments2_finish(ctx, j, u64p(&a->x), u64p(&w), u64p(&out->x)), what);
  } else {
    ck(sp_fold_commitments2(ctx, u64p(&a->x), u64p(&b->x), n, u64p(&w), u64p(&out->x)), what);
  }
}
// sample_random_instance_witness (src/r1cs/mod.rs:474-531) on the verifier-circuit shape: Z = [W | u | X] and the blinds from `tape`, E = Az o Bz - u Cz, the
// two width-32 commitments through commit(slot, values, blinds). Values from the randomness tape only.
template <class Commit>
static void sample_random_instance(const vcirc::Shape& vs, Tape& tape, NNZkPrep::RandomInstance& R, Commit commit) {
  const size_t vnv = vs.total_vars, vcons = vs.num_cons, vio = vs.num_io();
  R.tape_from = tape.pos;
  R.Z.resize(vnv + vio + 1);
  for (auto& z : R.Z) z = tape.next();
  R.rW.resize(vnv / 32);
  R.rE.resize(vcons / 32);
  for (auto& b : R.rW) b = tape.next();
  for (auto& b : R.rE) b = tape.next();
  R.tape_count = tape.pos - R.tape_from;
  std::vector<fe_t> mv[3];
  vs.multiply_vec(R.Z, mv);
  const fe_t u = R.Z[vnv];
  R.E.resize(vcons);
  for (size_t i = 0; i < vcons; ++i) R.E[i] = fe_sub<S>(fe_mul<S>(mv[0][i], mv[1][i]), fe_mul<S>(u, mv[2][i]));
  R.comm_W = commit(0, std::vector<fe_t>(R.Z.begin(), R.Z.begin() + vnv), R.rW);
  R.comm_E = commit(1, R.E, R.rE);
}

// ---- the helper's jobs and the guards of a prove: members of NNProveState (below), which states when they end ------------------------------------------
// The random relaxed instance ahead of its place: its values sit at a position of the tape that only the shapes determine; checked again where it is used
struct NNRandomInstanceJob {
  const NNZkKey* pk = nullptr;
  NNZkPrep* ps = nullptr;
  Tape ahead{nullptr, 0};
  void run() {
    NNZkPrep::RandomInstance& R = ps->rnd;
    try {
      ck(sp_ctx_bind_thread(ps->ctx2), "device");
      sample_random_instance(pk->vc, ahead, R, [&](int slot, const std::vector<fe_t>& v, const std::vector<fe_t>& bl) { return commit_rows32_side(*ps, slot, pk->vc_ck, v, bl); });
      R.valid = true;
    } catch (...) {
      R.valid = false;  // the prover computes it inline when it gets there (and reports what fails, if it fails again)
    }
  }
};
// the fold of the step instances' commitments, handed over by nifs_prove (it writes the state's f_comm)
struct NNFoldJob {
  NNZkPrep* ps = nullptr;
  std::function<void(sp_ctx*)> job;
  void run() {
    ck(sp_ctx_bind_thread(ps->ctx2), "device");
    job(ps->ctx2);
  }
};
// delta (ipa.rs:139-147): the mask and its blinds follow the random instance and NovaNIFS's r_T on the tape
struct NNDeltaJob {
  const NNZkKey* pk = nullptr;
  NNZkPrep* ps = nullptr;
  Tape ahead{nullptr, 0};
  void run() {
    NNZkPrep::OpeningAhead& O = ps->open;
    try {
      O.tape_from = ahead.pos;
      O.dv.resize(DEFAULT_COMMITMENT_WIDTH);
      for (auto& x : O.dv) x = ahead.next();
      O.r_delta = ahead.next();
      O.r_beta = ahead.next();
      O.tape_count = ahead.pos - O.tape_from;
      ck(sp_msm_ck(ps->ctx2, pk->ck, u64p(O.dv.data()), O.dv.size(), u64p(&O.r_delta), u64p(&O.delta.x)), "delta");
      O.delta_valid = true;
    } catch (...) {
      O.delta_valid = false;
    }
  }
};
// r_y is known: the halves of comm_LZ and beta, under the verifier-circuit phase (reads the state's f_comm and core_comm)
struct NNOpeningPointsJob {
  const NNZkKey* pk = nullptr;
  NNZkPrep* ps = nullptr;
  const std::vector<aff_t>*f_comm = nullptr, *core_comm = nullptr;
  size_t rows = 0;
  std::vector<fe_t> L, Rv;
  void run() {
    NNZkPrep::OpeningAhead& O = ps->open;
    try {
      if (!O.delta_valid || Rv.size() != O.dv.size() || L.size() > rows) return;
      ck(sp_ctx_bind_thread(ps->ctx2), "device");
      ck(sp_msm(ps->ctx2, u64p(L.data()), u64p(&(*f_comm)[0].x), L.size(), u64p(&O.P_f.x)), "<L, folded rows>");
      ck(sp_msm(ps->ctx2, u64p(L.data()), u64p(&(*core_comm)[0].x), L.size(), u64p(&O.P_c.x)), "<L, core rows>");
      fe_t ip = fe_zero();
      for (size_t i = 0; i < Rv.size(); ++i) ip = fe_add<S>(ip, fe_mul<S>(Rv[i], O.dv[i]));
      ck(sp_hyrax_commit_small(ps->ctx2, pk->vc_ck, u64p(&ip), 1, u64p(&O.r_beta), u64p(&O.beta.x)), "beta");
      sp_fold_commitments2_drop(O.lz_fold);
      O.lz_fold = nullptr;
      if (sp_fold_commitments2_begin(ps->ctx2, u64p(&O.P_c.x), 1, &O.lz_fold) != SP_OK) O.lz_fold = nullptr;
      O.points_valid = true;
    } catch (...) {
      O.points_valid = false;
    }
  }
};
// The opening's W = folded_W + c_eval core_W exists only once c_eval is drawn, at the very end - but L^T W (bind_with_delayed, hyrax_pc.rs:38-54) is linear in
// the table: LZ = L^T folded_W + c_eval L^T core_W, and L = eq(r_y[1..]) is known behind the inner sum-check. The two products run as jobs of the library's
// vector stream under the verifier-circuit phase (one job at a time: the second is begun where the first is collected).
struct NNLzAhead {
  sp_vec_job* job = nullptr;
  size_t cols = 0;
  std::vector<fe_t> f, c;
  int have = 0;  // 1: f, 2: f and c
  void begin(sp_ctx* ctx, const sp_table* W, const fe_t* r_y, size_t nvr) {
    if (sp_rowmat_vec_eq_begin(ctx, W, u64p(r_y + 1), nvr, cols, &job) != SP_OK) job = nullptr;
  }
  void step(sp_ctx* ctx, const sp_table* next_W, const fe_t* r_y, size_t nvr) {  // collect the product in flight, begin the next
    if (!job) return;
    std::vector<fe_t>& dst = have == 0 ? f : c;
    dst.resize(cols);
    sp_vec_job* j = job;
    job = nullptr;
    if (sp_rowmat_vec_eq_finish(ctx, j, u64p(dst.data())) != SP_OK) return;
    if (++have == 1) begin(ctx, next_W, r_y, nvr);
  }
  void collect(sp_ctx* ctx) {  // an exit path: the job owns device work
    if (!job) return;
    std::vector<fe_t> sink(cols);
    (void)sp_rowmat_vec_eq_finish(ctx, job, u64p(sink.data()));
    job = nullptr;
  }
};
// the opening folds comm = folded + c_eval * core rows and comm_eval = eW_step + c_eval * eW_core with a weight drawn at the very end: the doubling
// ladders of the core rows (behind the instances) and of the core evaluation's commitment (behind its round) are built on the library's polling threads meanwhile
struct NNFold2Jobs {
  sp_fold2_job *rows = nullptr, *eval = nullptr;
  void drop() {
    sp_fold_commitments2_drop(rows);
    sp_fold_commitments2_drop(eval);
    rows = eval = nullptr;
  }
};
// what the round hooks of nifs_prove and of the two batched sum-checks reach: process_round on the verifier circuit's state
struct NNHookCtx {
  const NNZkKey* pk;
  vcirc::Circuit* vc;
  vcirc::State* st;
  Tr* tr;
  Tape* tape;
  size_t outer_start, inner_start;
  std::exception_ptr err;
};
// NIFS (:1770-1783): finish_round! = vc.nifs_polys[t] <- coefficients, then process_round (:703-735); once more after the rounds (:1207-1210)
static void nn_nifs_hook(void* u, size_t t, const uint64_t* co, uint64_t* r_b) {
  NNHookCtx* h = (NNHookCtx*)u;
  if (h->err) return;
  try {
    if (t < h->pk->nb) {
      for (int q = 0; q < 4; ++q) memcpy(&h->vc->nifs_polys[t][q], co + 4 * q, 32);
      const fe_t r = vcirc::process_round(h->pk->ctx, *h->st, h->pk->vc, h->pk->vc_ck, *h->vc, t, *h->tr, *h->tape)[0];
      memcpy(r_b, &r, 32);
    } else {
      memcpy(&h->vc->t_out_step, co, 32);
      memcpy(&h->vc->eq_rho_at_rb, co + 4, 32);
      vcirc::process_round(h->pk->ctx, *h->st, h->pk->vc, h->pk->vc_ck, *h->vc, t, *h->tr, *h->tape);
    }
  } catch (...) {
    h->err = std::current_exception();
  }
}
// a round of the batched outer (4 coefficients) or inner (3) sum-check: the step and the core polynomial into the circuit, then process_round
static int nn_batched_hook(void* u, size_t round, const uint64_t* cs_, const uint64_t* cc_, size_t ncoeffs, uint64_t r_out[4]) {
  NNHookCtx* h = (NNHookCtx*)u;
  try {
    if (ncoeffs == 4) {
      const size_t i = round - h->outer_start;
      for (int q = 0; q < 4; ++q) {
        memcpy(&h->vc->outer_step[i][q], cs_ + 4 * q, 32);
        memcpy(&h->vc->outer_core[i][q], cc_ + 4 * q, 32);
      }
    } else {
      const size_t j = round - h->inner_start;
      for (int q = 0; q < 3; ++q) {
        memcpy(&h->vc->inner_step[j][q], cs_ + 4 * q, 32);
        memcpy(&h->vc->inner_core[j][q], cc_ + 4 * q, 32);
      }
    }
    const fe_t r = vcirc::process_round(h->pk->ctx, *h->st, h->pk->vc, h->pk->vc_ck, *h->vc, round, *h->tr, *h->tape)[0];
    memcpy(r_out, &r, 32);
    return 0;
  } catch (...) {
    h->err = std::current_exception();
    return SP_ERR_INTERNAL;
  }
}

// ---- prove (:1609-2093) ---------------------------------------------------------------------------------------------------------------------------------
// A sequence of named steps over one NNProveState, in the order of the reference's statements; nn_prove runs them for both drivers:
//   nn_prove_setup             the device, the polling threads, the round-hooks promise; (side) the second context and the random instance's job
//   nn_prove_rerandomize       core (shared, precommitted), then every step's precommitted commitment, one call                  (:1619-1627)
//   nn_prove_rest_commitments  the rest rows' blinds; commit_zeros, or the rest segments of several instances per call           (:1662-1719)
//   nn_prove_instances         the instances' rows and blinds, the proof's header; (side) the core rows' ladders begin           (:1662-1719)
//   nn_prove_nifs              the transcript's head, the hooks, nifs_prove; (side) the fold's and delta's jobs                  (:1770-1783)
//   nn_prove_outer             core products, the batched outer sum-check, the claims' round                                     (:1786-1850)
//   nn_prove_inner             evals_rx, both poly_ABC, the z tables, the batched inner sum-check, the evaluation rounds;        (:1852-1945)
//                              (side) the opening-points job, L^T folded_W begun, the core evaluation's ladder
//   nn_prove_vc_instance       finalize_multiround_witness                                                                       (:1948-1952)
//   nn_prove_random_instance   sample_random_instance_witness: the job's, or inline                                              (src/r1cs/mod.rs:474-531)
//   nn_prove_nova_nifs         NovaNIFS::prove and the fold of instance and witness                                              (src/nifs.rs:34-61)
//   nn_prove_relaxed_spartan   RelaxedR1CSSpartanProof::prove                                                                    (src/spartan_relaxed.rs:98-213)
//   nn_prove_opening           the two evaluation claims folded, then nn_open_reference_order or nn_open_side                    (:2019-2080)
//   nn_prove_emit              the rest of the proof in the canonical layout, the phase times, the layout check
// reference_order: ONE thread, the statements of src/neutronnova_zk.rs:1609-2093 in their order, ABI calls only — no jobs on a second context, the folded
// opening as the single PCS::prove call (sp_hyrax_prove) — what an unchanged neutronnova_zk.rs over the shim of integration/ gets. Same proof.
//
// LIFETIME RULE, stated here once: whatever a job on ps.wk, a begun sp_fold2_job or a begun sp_vec_job reads or writes is a member of this state (or of the
// key / the prep state, which outlive it). ~NNProveState runs on every exit path, exceptions included, and its BODY - which runs before any member is
// destroyed, whatever their declaration order - (1) drains ps.wk, (2) collects the outstanding vector job, (3) drops the fold-2 jobs, (4) resets the
// round-hooks promise. A step must not hand a job the address of one of its locals.
struct NNProveState {
  const NNZkKey& pk;
  NNZkPrep& ps;
  Tape& tape;
  sp_ctx* const ctx;
  const bool reference_order, side;  // side = !reference_order: jobs on the second context (false = everything inline on the caller's context, in the steps' order)
  // row counts and dimensions. The core circuit may split the same number of rows differently (nn_setup: equal shared segment, equal total after equalize)
  const sp_dims &d, &dc;
  const size_t CW = DEFAULT_COMMITMENT_WIDTH, n, nv, N, dpub;
  const size_t rows_sh, rows_pre, rows_rest, rows, rows_pre_c, rows_rest_c, nvr;
  ProofBuf proof;
  // the instances
  std::vector<aff_t> comms, core_comm, all_c_rest;
  std::vector<fe_t> X, r_W, core_rW, all_rest;
  std::vector<const sp_table*> Ws;
  // the transcript, the verifier circuit and what the hooks reach
  std::unique_ptr<Tr> tr;
  std::unique_ptr<vcirc::Circuit> vc;
  std::unique_ptr<vcirc::State> vst;
  NNHookCtx hc{};
  // the NIFS outputs and the working tables
  size_t left = 0, right = 0;
  std::vector<uint64_t> polys, r_bs, E_eq, tail, f_rW, f_X;
  std::vector<aff_t> f_comm;
  sp_table *A = nullptr, *B = nullptr, *C = nullptr, *fW = nullptr, *core_abc[3] = {}, *zc = nullptr, *pl = nullptr, *pr = nullptr, *rx = nullptr;
  sp_table *abc_s = nullptr, *abc_c = nullptr, *zs = nullptr, *zcc = nullptr, *Wf = nullptr;
  // the helper's jobs with their tickets, the begun folds, the product ahead, the promise
  NNRandomInstanceJob rnd_job;
  NNFoldJob fold_job;
  NNDeltaJob delta_job;
  NNOpeningPointsJob points_job;
  size_t t_rnd = 0, t_fold = 0, t_open = 0;
  NNFold2Jobs fold2;
  NNLzAhead lz;
  bool hooks_promised = false;
  // the batched sum-checks
  fe_t r, claims[2], fin[4];
  std::vector<fe_t> r_x, r_y, folded_X;
  size_t inner_final = 0;
  // the verifier-circuit instance, the random one, their fold, the relaxed Spartan proof
  std::vector<fe_t> vpub, Uv_X, Wv_r;
  std::vector<aff_t> Uv_comm;
  NNZkPrep::RandomInstance rnd;
  fe_t rnd_u, ufold;
  std::vector<fe_t> rnd_W, rnd_X, r_T, T, Wfold, Efold, rWfold, rEfold, Xfold;
  std::vector<aff_t> comm_T;
  std::vector<fe_t> v_outer, v_inner, v_W, v_E;
  fe_t v_claims[3], blind_vW, blind_vE;
  // the opening: the folded claim (commitment rows, their blinds, the evaluation's commitment and blind) and the argument's values
  fe_t c_eval, blind_eval;
  std::vector<aff_t> comm;
  std::vector<fe_t> blind;
  aff_t comm_eval, delta, beta;
  std::vector<fe_t> z_vec;
  fe_t z_delta, z_beta;
  // time stamps and laps
  double t_start = 0, t_inst = 0, t_nifs = 0, t_outer = 0, t_inner = 0, t_vc = 0, t_end = 0;
  NNLaps laps{"nn_prove"};

  static size_t seg_rows(size_t unpadded, size_t padded) { return unpadded ? padded / DEFAULT_COMMITMENT_WIDTH : 0; }
  NNProveState(const NNZkKey& pk_, NNZkPrep& ps_, Tape& tape_, bool reference_order_)
      : pk(pk_), ps(ps_), tape(tape_), ctx(pk_.ctx), reference_order(reference_order_), side(!reference_order_), d(pk_.dims), dc(pk_.dims_core), n(ps_.steps.size()),
        nv(pk_.num_vars), N(d.num_cons), dpub(d.num_public), rows_sh(seg_rows(d.num_shared_unpadded, d.num_shared)),
        rows_pre(seg_rows(d.num_precommitted_unpadded, d.num_precommitted)), rows_rest(d.num_rest / CW), rows(rows_sh + rows_pre + rows_rest),
        rows_pre_c(seg_rows(dc.num_precommitted_unpadded, dc.num_precommitted)), rows_rest_c(dc.num_rest / CW), nvr(log2_ceil(rows)) {
    if (rows_sh + rows_pre_c + rows_rest_c != rows) throw Error(SP_ERR_INTERNAL, "NeutronNova: step and core rows differ after equalize");
  }
  NNProveState(const NNProveState&) = delete;
  NNProveState& operator=(const NNProveState&) = delete;
  ~NNProveState() {  // the lifetime rule above
    ps.wk.drain();
    lz.collect(ctx);
    fold2.drop();
    if (hooks_promised) sp_ctx_round_hooks_host_only(ctx, 0);
  }
  template <class Job>
  size_t submit(Job& job) {  // `job` is a member of this state
    return ps.wk.submit([&job] { job.run(); });
  }
  static double now() { return NNLaps::now(); }
};

static void nn_prove_setup(NNProveState& st) {
  const NNZkKey& pk = st.pk;
  NNZkPrep& ps = st.ps;
  ck(sp_ctx_bind_thread(st.ctx), "device");
  ck(sp_walkers_keep_hot(20000), "walkers");  // the round commitments and the host loops of the verifier-circuit instance are spread over them
  // process_round is host work when its commitments go through the walkers: the batched sum-checks may then queue a round's launch ahead of it
  st.hooks_promised = true;
  ck(sp_ctx_round_hooks_host_only(st.ctx, vcirc::split_commitments_on(pk.vc_ck) ? 1 : 0), "round hooks");
  ps.rnd.valid = false;
  ps.open.delta_valid = ps.open.points_valid = false;
  if (!st.side) return;
  if (!ps.ctx2) ck(sp_ctx_create(sp_ctx_device(st.ctx), &ps.ctx2), "second context");
  // the draws in front of the random instance's: the rerandomisation blinds, the rest-row blinds and one blind per committed row of the verifier circuit's rounds
  size_t before = ps.comm_shared.size() + ps.core.comm_pre.size() + st.n * st.rows_rest + st.rows_rest_c + pk.vc.total_vars / 32;
  for (const auto& s : ps.steps) before += s.comm_pre.size();
  st.rnd_job.pk = &pk;
  st.rnd_job.ps = &ps;
  st.rnd_job.ahead = st.tape;
  st.rnd_job.ahead.pos = st.tape.pos + before;
  st.t_rnd = st.submit(st.rnd_job);
}

// rerandomize (:1619-1627, hyrax_pc.rs:321-344): core (shared, precommitted), then every step's precommitted commitment. The new blinds are
// drawn in the reference's order; the row updates are independent, so all of them go through ONE sp_hyrax_rerandomize call.
static void nn_prove_rerandomize(NNProveState& st) {
  NNZkPrep& ps = st.ps;
  std::vector<std::pair<std::vector<aff_t>*, std::vector<fe_t>*>> parts;
  parts.push_back({&ps.comm_shared, &ps.r_shared});
  parts.push_back({&ps.core.comm_pre, &ps.core.r_pre});
  for (auto& s : ps.steps) parts.push_back({&s.comm_pre, &s.r_pre});
  std::vector<aff_t> all_c;
  std::vector<fe_t> all_old, all_new;
  for (auto& pr_ : parts)
    for (size_t i = 0; i < pr_.first->size(); ++i) {
      all_c.push_back((*pr_.first)[i]);
      all_old.push_back((*pr_.second)[i]);
      all_new.push_back(st.tape.next());
    }
  if (all_c.empty()) return;
  std::vector<aff_t> out(all_c.size());
  ck(sp_hyrax_rerandomize(st.ctx, st.pk.ck, u64p(&all_c[0].x), all_c.size(), u64p(all_old.data()), u64p(all_new.data()), u64p(&out[0].x)), "rerandomize_commitment");
  size_t o = 0;
  for (auto& pr_ : parts)
    for (size_t i = 0; i < pr_.first->size(); ++i, ++o) {
      (*pr_.first)[i] = out[o];
      (*pr_.second)[i] = all_new[o];
    }
}

// instances and witnesses (:1662-1719), the rest rows: commit_zeros (h * blind) — one sp_fixed_base_mul_h call for the rest rows of all instances — or, for a
// circuit with rest variables, the commitment of its rest segment under the same blinds (bellpepper/r1cs.rs:463-500); no challenges for these circuits
static void nn_prove_rest_commitments(NNProveState& st) {
  sp_ctx* ctx = st.ctx;
  const NNZkKey& pk = st.pk;
  NNZkPrep& ps = st.ps;
  const sp_dims &d = st.d, &dc = st.dc;
  const size_t n = st.n, rows_rest = st.rows_rest, rows_rest_c = st.rows_rest_c;
  std::vector<fe_t>& all_rest = st.all_rest;
  std::vector<aff_t>& all_c_rest = st.all_c_rest;
  all_rest.resize(n * rows_rest + rows_rest_c);
  for (auto& b : all_rest) b = st.tape.next();  // steps in order, then the core: the reference's call order
  all_c_rest.resize(all_rest.size());
  if (!all_rest.empty() && !(d.num_rest_unpadded && dc.num_rest_unpadded))
    ck(sp_fixed_base_mul_h(ctx, pk.ck, u64p(all_rest.data()), all_rest.size(), u64p(&all_c_rest[0].x)), "commit_zeros");
  // the rest segments of several instances side by side in one table are ONE row-wise commitment (a Hyrax commitment is one MSM per 2048-entry row): a call
  // per instance costs 0.25 ms of fixed work each (64 instances of the reference's two-block test circuit: 15.9 ms of a 23 ms prove)
  struct RestJob {
    const NNPre* p;
    size_t off, len, blind_at, nrows;  // the segment inside p->W, its blinds / rows inside all_rest / all_c_rest
  };
  std::vector<RestJob> todo;
  if (d.num_rest_unpadded)
    for (size_t i = 0; i < n; ++i) todo.push_back({&ps.steps[i], d.num_shared + d.num_precommitted, d.num_rest, i * rows_rest, rows_rest});
  if (dc.num_rest_unpadded) todo.push_back({&ps.core, dc.num_shared + dc.num_precommitted, dc.num_rest, n * rows_rest, rows_rest_c});
  const size_t cap = (size_t)1 << 25;  // <= 1 GiB of staged elements per call
  for (size_t at = 0; at < todo.size();) {
    size_t cnt = 1, elems = todo[at].len;
    while (at + cnt < todo.size() && elems + todo[at + cnt].len <= cap) elems += todo[at + cnt++].len;
    if (cnt == 1) {
      const RestJob& j = todo[at];
      ck(sp_hyrax_commit(ctx, pk.ck, j.p->W, j.off, j.len, u64p(all_rest.data() + j.blind_at), ps.is_small ? 1 : 0, u64p(&all_c_rest[j.blind_at].x)), "commit rest");
      at += 1;
      continue;
    }
    sp_table* staged = grown_slot(ctx, ps.rest_stage, ps.rest_stage_cap, elems, false, "rest staging table", "rest staging len");
    std::vector<fe_t> bl;
    size_t pos = 0;
    for (size_t k = 0; k < cnt; ++k) {
      const RestJob& j = todo[at + k];
      ck(sp_table_copy(ctx, staged, pos, j.p->W, j.off, j.len), "stage rest segment");
      pos += j.len;
      bl.insert(bl.end(), all_rest.begin() + j.blind_at, all_rest.begin() + j.blind_at + j.nrows);
    }
    std::vector<aff_t> out(bl.size());
    ck(sp_hyrax_commit(ctx, pk.ck, staged, 0, elems, u64p(bl.data()), ps.is_small ? 1 : 0, u64p(&out[0].x)), "commit rest (batched)");
    size_t o = 0;
    for (size_t k = 0; k < cnt; ++k) {
      const RestJob& j = todo[at + k];
      std::copy(out.begin() + o, out.begin() + o + j.nrows, all_c_rest.begin() + j.blind_at);
      o += j.nrows;
    }
    at += cnt;
  }
}

// instances and witnesses (:1662-1719), each instance: comm_W = shared | precommitted | rest rows with their blinds, and its fields of the proof
static void nn_prove_instances(NNProveState& st) {
  NNZkPrep& ps = st.ps;
  const size_t n = st.n, rows = st.rows, rows_sh = st.rows_sh;
  st.proof.pc(ps.comm_shared);
  st.comms.resize(n * rows);
  st.X.resize(n * st.dpub);
  st.r_W.resize(n * rows);
  st.Ws.resize(n);
  auto instance = [&](NNPre& p, size_t which, aff_t* comm_out, fe_t* r_out) {
    const size_t my_pre = which == n ? st.rows_pre_c : st.rows_pre, my_rest = which == n ? st.rows_rest_c : st.rows_rest;
    const fe_t* r_rest = st.all_rest.data() + which * st.rows_rest;  // (the core's blinds follow the n steps')
    const aff_t* c_rest = st.all_c_rest.data() + which * st.rows_rest;
    if (p.comm_pre.size() != my_pre) throw Error(SP_ERR_INTERNAL, "NeutronNova: precommitted rows of an instance");
    std::copy(ps.comm_shared.begin(), ps.comm_shared.end(), comm_out);
    std::copy(p.comm_pre.begin(), p.comm_pre.end(), comm_out + rows_sh);
    std::copy(c_rest, c_rest + my_rest, comm_out + rows_sh + my_pre);
    std::copy(ps.r_shared.begin(), ps.r_shared.end(), r_out);
    std::copy(p.r_pre.begin(), p.r_pre.end(), r_out + rows_sh);
    std::copy(r_rest, r_rest + my_rest, r_out + rows_sh + my_pre);
    st.proof.pc(p.comm_pre);
    for (size_t i = 0; i < my_rest; ++i) st.proof.pp(c_rest[i]);
    for (const fe_t& f : p.publics) st.proof.pf(f);
  };
  for (size_t i = 0; i < n; ++i) {
    instance(ps.steps[i], i, &st.comms[i * rows], &st.r_W[i * rows]);
    std::copy(ps.steps[i].publics.begin(), ps.steps[i].publics.end(), st.X.begin() + i * st.dpub);
    st.Ws[i] = ps.steps[i].W;
  }
  st.core_comm.resize(rows);
  st.core_rW.resize(rows);
  instance(ps.core, n, st.core_comm.data(), st.core_rW.data());
  if (st.side) ck(sp_fold_commitments2_begin(st.ctx, u64p(&st.core_comm[0].x), rows, &st.fold2.rows), "fold_commitments (ladders)");
  st.t_inst = st.now();
}

// NeutronNovaNIFS::prove (:1770-1783) with process_round as its round hook; behind it the helper gets the fold of the step commitments and delta
static void nn_prove_nifs(NNProveState& st) {
  sp_ctx* ctx = st.ctx;
  const NNZkKey& pk = st.pk;
  NNZkPrep& ps = st.ps;
  const size_t N = st.N, nv = st.nv, nb = pk.nb, rows = st.rows, dpub = st.dpub;
  st.tr.reset(new Tr(ctx, "neutronnova_prove"));
  absorb_head(*st.tr, pk, st.core_comm, ps.core.publics);
  st.vc.reset(new vcirc::Circuit(pk.nb, pk.nx, pk.ny, 32));
  st.vst.reset(new vcirc::State(pk.vc));
  st.hc = NNHookCtx{&pk, st.vc.get(), st.vst.get(), st.tr.get(), &st.tape, pk.nb + 1, pk.nb + 1 + pk.nx + 1, nullptr};
  size_t ell;
  compute_tensor_decomp(N, &ell, &st.left, &st.right);
  st.polys.resize(16 * std::max<size_t>(nb, 1));
  st.r_bs.resize(4 * std::max<size_t>(nb, 1));
  st.E_eq.resize(4 * (st.left + st.right));
  st.tail.resize(8);
  st.f_rW.resize(4 * rows);
  st.f_X.resize(4 * std::max<size_t>(dpub, 1));
  st.f_comm.resize(rows);
  st.A = work_table(ctx, ps, 0, N), st.B = work_table(ctx, ps, 1, N), st.C = work_table(ctx, ps, 2, N), st.fW = work_table(ctx, ps, 3, nv);
  for (int m = 0; m < 3; ++m) st.core_abc[m] = work_table(ctx, ps, 4 + m, N);
  st.zc = work_table(ctx, ps, 7, nv + 1 + dpub);
  st.pl = work_table(ctx, ps, 8, st.left), st.pr = work_table(ctx, ps, 9, st.right), st.rx = work_table(ctx, ps, 10, N);
  st.abc_s = work_table(ctx, ps, 11, 2 * nv), st.abc_c = work_table(ctx, ps, 12, 2 * nv), st.zs = work_table(ctx, ps, 13, 2 * nv), st.zcc = work_table(ctx, ps, 14, 2 * nv);
  st.Wf = work_table(ctx, ps, 15, nv);
  NifsOutputs no{st.polys.data(), st.r_bs.data(), st.E_eq.data(), st.tail.data(), st.f_rW.data(), st.f_X.data(), (uint64_t*)st.f_comm.data(), st.A, st.B, st.C, st.fW};
  st.fold_job.ps = &ps;
  if (st.side) no.deferred_fold_commitments = &st.fold_job.job;
  nifs_prove(ctx, pk.S_step, st.d, pk.ck, st.n, rows, st.comms.data(), st.X.data(), st.Ws.data(), st.r_W.data(), true, ps.nifs_cached, st.tr->t, nn_nifs_hook, &st.hc, no);
  if (st.hc.err) std::rethrow_exception(st.hc.err);
  if (st.fold_job.job) {
    st.t_fold = st.submit(st.fold_job);
    const vcirc::Shape& vs = pk.vc;
    st.delta_job.pk = &pk;
    st.delta_job.ps = &ps;
    st.delta_job.ahead = st.tape;
    st.delta_job.ahead.pos = st.tape.pos + (pk.vc.total_vars / 32 - st.vst->commits) + (vs.total_vars + vs.num_io() + 1) + vs.total_vars / 32 + 2 * (vs.num_cons / 32);
    st.submit(st.delta_job);
  }
  st.t_nifs = st.now();
}

// z = [W | 1 | X] of a circuit into a working table
static void nn_fill_z(NNProveState& st, sp_table* z, const sp_table* W, const std::vector<fe_t>& Xv) {
  ck(sp_table_copy(st.ctx, z, 0, W, 0, st.nv), "z <- W");
  std::vector<fe_t> tl(1 + Xv.size());
  tl[0] = fe_one<S>();
  std::copy(Xv.begin(), Xv.end(), tl.begin() + 1);
  ck(sp_table_write(st.ctx, z, st.nv, u64p(tl.data()), tl.size()), "z tail");
}

// core products, batched outer sum-check (:1786-1850), in three parts: what stands in front of the sum-check, the sum-check of this proof's (step, core)
// pair, what stands behind it. nn_prove runs them back to back; nn_prove_batch runs ONE lockstep sum-check for the pairs of all its proofs in the middle.
static void nn_prove_outer_before(NNProveState& st) {
  sp_ctx* ctx = st.ctx;
  sp_table** core_abc = st.core_abc;
  nn_fill_z(st, st.zc, st.ps.core.W, st.ps.core.publics);
  ck(sp_multiply_vec(ctx, st.pk.S_core, st.zc, core_abc[0], core_abc[1], core_abc[2]), "multiply_vec (core)");
  ck(sp_table_write(ctx, st.pl, 0, st.E_eq.data(), st.left), "pow left");
  ck(sp_table_write(ctx, st.pr, 0, st.E_eq.data() + 4 * st.left, st.right), "pow right");
  st.r_x.resize(st.pk.nx);
}
static void nn_prove_outer_sumcheck(NNProveState& st) {
  sp_table** core_abc = st.core_abc;
  int rc = sp_sumcheck_cubic_outer_pow_batched(st.ctx, st.pk.nx, st.pl, st.pr, st.A, st.B, st.C, core_abc[0], core_abc[1], core_abc[2], st.tail.data(), st.hc.outer_start,
                                               nn_batched_hook, &st.hc, u64p(st.r_x.data()));
  if (st.hc.err) std::rethrow_exception(st.hc.err);
  ck(rc, "outer sum-check (batched)");
}
static void nn_prove_outer_after(NNProveState& st) {
  sp_ctx* ctx = st.ctx;
  const NNZkKey& pk = st.pk;
  vcirc::Circuit& vc = *st.vc;
  sp_table** core_abc = st.core_abc;
  {
    sp_table* cl[6] = {st.A, st.B, st.C, core_abc[0], core_abc[1], core_abc[2]};
    fe_t v[6];
    for (int q = 0; q < 6; ++q) ck(sp_table_read(ctx, cl[q], 0, 1, u64p(&v[q])), "claims");
    for (int q = 0; q < 3; ++q) {
      vc.claim_step[q] = v[q];
      vc.claim_core[q] = v[3 + q];
    }
    ck(sp_table_read(ctx, st.pl, 0, 1, u64p(&vc.tau_at_rx)), "tau_at_rx");
  }
  st.r = vcirc::process_round(ctx, *st.vst, pk.vc, pk.vc_ck, vc, st.hc.outer_start + pk.nx, *st.tr, st.tape)[0];
  st.t_outer = st.now();
}
static void nn_prove_outer(NNProveState& st) {
  nn_prove_outer_before(st);
  nn_prove_outer_sumcheck(st);
  nn_prove_outer_after(st);
}

// evals_rx, both poly_ABC, the z tables, batched inner sum-check (:1852-1945), in the same three parts. lz_ahead: L^T folded_W goes out as a job of the
// context's vector stream, which carries ONE job at a time - nn_prove_batch, with several states alive on one context, leaves it out (nn_open_side then
// folds W and takes the product where it needs it: same proof).
static void nn_prove_inner_before(NNProveState& st) {
  sp_ctx* ctx = st.ctx;
  const NNZkKey& pk = st.pk;
  NNZkPrep& ps = st.ps;
  vcirc::Circuit& vc = *st.vc;
  const size_t nv = st.nv, dpub = st.dpub;
  const fe_t r = st.r, r2 = fe_mul<S>(r, r);
  st.claims[0] = joint_inner_claim(vc.claim_step, r, r2);
  st.claims[1] = joint_inner_claim(vc.claim_core, r, r2);
  ck(sp_eq_table_into(ctx, u64p(st.r_x.data()), pk.nx, st.rx), "evals_rx");
  ck(sp_poly_abc(ctx, pk.S_step, st.rx, u64p(&r), 2 * nv, st.abc_s), "poly_ABC (step)");
  ck(sp_poly_abc(ctx, pk.S_core, st.rx, u64p(&r), 2 * nv, st.abc_c), "poly_ABC (core)");
  st.folded_X.resize(dpub);
  memcpy(st.folded_X.data(), st.f_X.data(), dpub * sizeof(fe_t));
  auto fill_z = [&](sp_table* z, const sp_table* W, const std::vector<fe_t>& Xv) {
    nn_fill_z(st, z, W, Xv);
    ck(sp_table_zero(ctx, z, nv + 1 + Xv.size(), nv - 1 - Xv.size()), "z: zero high half");  // a working table: the last prove's rounds were bound in place
  };
  fill_z(st.zs, st.fW, st.folded_X);
  fill_z(st.zcc, ps.core.W, ps.core.publics);
  for (sp_table* t : {st.abc_s, st.abc_c, st.zs, st.zcc}) ck(sp_table_set_len(t, 2 * nv, nv, 1 + dpub), "halves");
  st.r_y.resize(pk.ny);
}
static void nn_prove_inner_sumcheck(NNProveState& st) {
  int rc = sp_sumcheck_quad_batched(st.ctx, u64p(st.claims), st.pk.ny, st.abc_s, st.abc_c, st.zs, st.zcc, st.hc.inner_start, nn_batched_hook, &st.hc, u64p(st.r_y.data()),
                                    u64p(st.fin));
  if (st.hc.err) std::rethrow_exception(st.hc.err);
  ck(rc, "inner sum-check (batched)");
}
static void nn_prove_inner_after(NNProveState& st, bool lz_ahead) {
  sp_ctx* ctx = st.ctx;
  const NNZkKey& pk = st.pk;
  NNZkPrep& ps = st.ps;
  vcirc::Circuit& vc = *st.vc;
  const size_t nvr = st.nvr;
  const std::vector<fe_t>& r_y = st.r_y;
  if (st.t_fold) {  // r_y is known: the halves of comm_LZ and beta, under the verifier-circuit phase
    NNOpeningPointsJob& j = st.points_job;
    j.pk = &pk, j.ps = &ps, j.f_comm = &st.f_comm, j.core_comm = &st.core_comm, j.rows = st.rows;
    j.L = eq_evals_host(r_y.data() + 1, nvr);
    j.Rv = eq_evals_host(r_y.data() + 1 + nvr, pk.ny - 1 - nvr);
    st.t_open = st.submit(j);
  }
  if (st.side && lz_ahead) {  // L^T folded_W goes out (NNLzAhead)
    st.lz.cols = (size_t)1 << (pk.ny - 1 - nvr);
    st.lz.begin(ctx, st.fW, r_y.data(), nvr);
  }
  vc.eval_X_step = nn_eval_X(pk.ny, st.folded_X.data(), st.folded_X.size(), r_y.data());
  vc.eval_X_core = nn_eval_X(pk.ny, ps.core.publics.data(), ps.core.publics.size(), r_y.data());
  const fe_t inv = inv_one_minus(r_y[0]);
  vc.eval_W_step = eval_W_from(st.fin[2], r_y[0], vc.eval_X_step, inv);
  vc.eval_W_core = eval_W_from(st.fin[3], r_y[0], vc.eval_X_core, inv);
  st.inner_final = st.hc.inner_start + pk.ny;
  for (size_t k = 0; k < 3; ++k) vcirc::process_round(ctx, *st.vst, pk.vc, pk.vc_ck, vc, st.inner_final + k, *st.tr, st.tape);
  if (st.side) ck(sp_fold_commitments2_begin(ctx, u64p(&st.vst->comm_per_round[st.inner_final + 2][0].x), 1, &st.fold2.eval), "fold eval commitments (ladder)");
  st.t_inner = st.now();
}
static void nn_prove_inner(NNProveState& st) {
  nn_prove_inner_before(st);
  nn_prove_inner_sumcheck(st);
  nn_prove_inner_after(st, true);
}

// finalize_multiround_witness (:1948-1952): U_verifier, its regular form, W_verifier
static void nn_prove_vc_instance(NNProveState& st) {
  const vcirc::Shape& vs = st.pk.vc;
  const vcirc::State& vst = *st.vst;
  st.vpub.assign(vst.cs.inputs.begin() + 1 + vs.total_challenges, vst.cs.inputs.end());
  for (const auto& c : vst.comm_per_round) st.Uv_comm.insert(st.Uv_comm.end(), c.begin(), c.end());
  for (const auto& c : vst.challenges) st.Uv_X.insert(st.Uv_X.end(), c.begin(), c.end());
  st.Uv_X.insert(st.Uv_X.end(), st.vpub.begin(), st.vpub.end());
  for (const auto& b : vst.blind_per_round) st.Wv_r.insert(st.Wv_r.end(), b.begin(), b.end());
  st.laps.lap("(up to the vc instance)");
  if (st.laps.on)
    fprintf(stderr, "nn_prove: process_round totals: synthesis %.3f ms, commitments %.3f ms, transcript %.3f ms over %zu rounds\n", vst.synth_ms, vst.commit_ms, vst.hash_ms, vst.current);
}

// sample_random_instance_witness (src/r1cs/mod.rs:474-531) on the verifier-circuit shape: what the helper's job left, if it is this tape position's; else here
static void nn_prove_random_instance(NNProveState& st) {
  const NNZkKey& pk = st.pk;
  NNZkPrep& ps = st.ps;
  const size_t vnv = pk.vc.total_vars;
  if (st.t_rnd) ps.wk.wait(st.t_rnd);
  const bool ahead_ok = st.side && ps.rnd.valid && ps.rnd.tape_from == st.tape.pos;
  if (ahead_ok) {
    st.tape.skip(ps.rnd.tape_count);
    std::swap(st.rnd, ps.rnd);
  } else {
    if (st.laps.on && st.side)
      fprintf(stderr, "nn_prove: random instance computed inline (job valid %d, tape %zu vs %zu)\n", (int)ps.rnd.valid, ps.rnd.tape_from, st.tape.pos);
    sample_random_instance(pk.vc, st.tape, st.rnd, [&](int, const std::vector<fe_t>& v, const std::vector<fe_t>& bl) { return commit_rows32(st.ctx, ps, pk.vc_ck, v, bl); });
  }
  const std::vector<fe_t>& Z = st.rnd.Z;
  st.rnd_u = Z[vnv];
  st.rnd_W.assign(Z.begin(), Z.begin() + vnv);
  st.rnd_X.assign(Z.begin() + vnv + 1, Z.end());
  st.laps.lap("random instance + 2 commits");
}

// NovaNIFS::prove (src/nifs.rs:34-61) + commit_T (src/r1cs/folds.rs:28-88), then the fold of the two instances and witnesses with the challenge
static void nn_prove_nova_nifs(NNProveState& st) {
  const NNZkKey& pk = st.pk;
  const vcirc::Shape& vs = pk.vc;
  const vcirc::State& vst = *st.vst;
  Tr& tr = *st.tr;
  const size_t vnv = vs.total_vars, vcons = vs.num_cons, vio = vs.num_io();
  const std::vector<fe_t>&rnd_W = st.rnd_W, &rnd_X = st.rnd_X, &rnd_E = st.rnd.E, &rnd_rW = st.rnd.rW, &rnd_rE = st.rnd.rE, &Uv_X = st.Uv_X;
  std::vector<fe_t>&T = st.T, &r_T = st.r_T;
  const fe_t rnd_u = st.rnd_u;
  absorb_U1(tr, st.rnd.comm_W.data(), st.rnd.comm_W.size(), st.rnd.comm_E.data(), st.rnd.comm_E.size(), rnd_u, rnd_X.data(), rnd_X.size());
  absorb_instance(tr, "U2", st.Uv_comm, Uv_X);
  r_T.resize(vcons / 32);
  for (auto& b : r_T) b = st.tape.next();
  std::vector<fe_t> Zs(vnv + 1 + vio), mv[3];
  par_for(vnv, 256, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) Zs[i] = fe_add<S>(rnd_W[i], vst.w[i]);
  });
  const fe_t u1 = fe_add<S>(rnd_u, fe_one<S>());
  Zs[vnv] = u1;
  for (size_t i = 0; i < vio; ++i) Zs[vnv + 1 + i] = fe_add<S>(rnd_X[i], Uv_X[i]);
  vs.multiply_vec(Zs, mv);
  T.resize(vcons);
  par_for(vcons, 48, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) T[i] = fe_sub<S>(fe_sub<S>(fe_mul<S>(mv[0][i], mv[1][i]), fe_mul<S>(u1, mv[2][i])), rnd_E[i]);
  });
  st.laps.lap("NovaNIFS: absorbs, Z, multiply_vec, T");
  st.comm_T = commit_rows32(st.ctx, st.ps, pk.vc_ck, T, r_T, st.side);
  st.laps.lap("NovaNIFS: commit_T");
  absorb_comm_T(tr, st.comm_T.data(), st.comm_T.size());
  st.lz.step(st.ctx, st.ps.core.W, st.r_y.data(), st.nvr);  // L^T folded_W is in; L^T core_W goes out
  st.laps.lap("NovaNIFS: T + commit_T");
  const fe_t rf = tr.squeeze("r");
  std::vector<fe_t>&Wfold = st.Wfold, &Efold = st.Efold, &rWfold = st.rWfold, &rEfold = st.rEfold, &Xfold = st.Xfold;
  Wfold.resize(vnv), Efold.resize(vcons), rWfold.resize(rnd_rW.size()), rEfold.resize(rnd_rE.size()), Xfold.resize(vio);
  par_for(vnv + vcons, 96, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      if (i < vnv) Wfold[i] = fe_add<S>(rnd_W[i], fe_mul<S>(rf, vst.w[i]));
      else Efold[i - vnv] = fe_add<S>(rnd_E[i - vnv], fe_mul<S>(rf, T[i - vnv]));
    }
  });
  for (size_t i = 0; i < rWfold.size(); ++i) rWfold[i] = fe_add<S>(rnd_rW[i], fe_mul<S>(rf, st.Wv_r[i]));
  for (size_t i = 0; i < rEfold.size(); ++i) rEfold[i] = fe_add<S>(rnd_rE[i], fe_mul<S>(rf, r_T[i]));
  for (size_t i = 0; i < vio; ++i) Xfold[i] = fe_add<S>(rnd_X[i], fe_mul<S>(rf, Uv_X[i]));
  st.ufold = fe_add<S>(rnd_u, rf);
}

// RelaxedR1CSSpartanProof::prove (src/spartan_relaxed.rs:98-213) on the folded instance
static void nn_prove_relaxed_spartan(NNProveState& st) {
  sp_ctx* ctx = st.ctx;
  NNZkPrep& ps = st.ps;
  const vcirc::Shape& vs = st.pk.vc;
  Tr& tr = *st.tr;
  const size_t vnv = vs.total_vars, vcons = vs.num_cons;
  const std::vector<fe_t>&Wfold = st.Wfold, &Efold = st.Efold, &Xfold = st.Xfold;
  const fe_t ufold = st.ufold;
  fe_t* v_claims = st.v_claims;
  tr.absorb_scalars("u_relaxed", &ufold, 1);
  tr.absorb_scalars("X_relaxed", Xfold.data(), Xfold.size());
  const size_t vlx = log2_ceil(vcons), vnvp = next_pow2(vnv), vly = log2_ceil(vnvp) + 1, vz_len = 2 * vnvp;
  std::vector<fe_t> zr = Wfold, mv[3];
  zr.push_back(ufold);
  zr.insert(zr.end(), Xfold.begin(), Xfold.end());
  vs.multiply_vec(zr, mv);
  std::vector<fe_t> vtau(vlx);
  for (auto& t : vtau) t = tr.squeeze("t");
  std::vector<fe_t> uczE(vcons);
  par_for(vcons, 96, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) uczE[i] = fe_add<S>(fe_mul<S>(ufold, mv[2][i]), Efold[i]);
  });
  std::vector<fe_t> v_rx(vlx), v_ry(vly);
  st.v_outer.resize(3 * vlx);
  st.v_inner.resize(2 * vly);
  // the two relaxed-Spartan sum-checks run on tables this driver holds on the host (2^9 and 2^12 elements): with polling host threads in the process
  // every round is run there (sp_sumcheck_*_host); staged to the device they are a trip over the bus a round
  static const bool host_sc_off = [] {
    const char* e = getenv("SPARTAN_HOST_SC");  // "0": the device provers on staged tables (A/B runs)
    return e && e[0] == '0';
  }();
  const bool host_sc = st.side && sp_walkers() > 0 && !host_sc_off;
  const fe_t zero = fe_zero();
  if (host_sc) {
    ck(sp_sumcheck_cubic3_host(ctx, u64p(&zero), u64p(vtau.data()), vlx, u64p(mv[0].data()), u64p(mv[1].data()), u64p(uczE.data()), tr.t, u64p(st.v_outer.data()),
                               u64p(v_rx.data()), u64p(v_claims)),
       "relaxed outer sum-check (host tables)");
  } else {
    sp_table *ta = stage(ctx, ps, 0, mv[0].data(), vcons), *tb = stage(ctx, ps, 1, mv[1].data(), vcons), *tc = stage(ctx, ps, 2, uczE.data(), vcons);
    ck(sp_sumcheck_cubic3(ctx, u64p(&zero), u64p(vtau.data()), vlx, ta, tb, tc, tr.t, u64p(st.v_outer.data()), u64p(v_rx.data()), u64p(v_claims)), "relaxed outer sum-check");
  }
  st.laps.lap("folds + relaxed outer sc");
  tr.absorb_scalars("claims_outer", v_claims, 3);
  const fe_t vr = tr.squeeze("r"), vr2 = fe_mul<S>(vr, vr);
  const std::vector<fe_t> v_evals_rx = eq_evals_host(v_rx.data(), vlx);
  fe_t claim_E = fe_zero();
  {
    fe_t partial[32];
    for (auto& x : partial) x = fe_zero();
    std::atomic<unsigned> slot{0};
    par_for(vcons, 64, [&](size_t lo, size_t hi) {
      fe_t acc = fe_zero();
      for (size_t i = lo; i < hi; ++i) acc = fe_add<S>(acc, fe_mul<S>(Efold[i], v_evals_rx[i]));
      partial[slot.fetch_add(1) & 31u] = acc;
    });
    for (const auto& x : partial) claim_E = fe_add<S>(claim_E, x);
  }
  const fe_t minus_E[3] = {v_claims[0], v_claims[1], fe_sub<S>(v_claims[2], claim_E)};
  const fe_t v_claim_inner = joint_inner_claim(minus_E, vr, vr2);
  const size_t vcols = vs.num_cols();
  std::vector<fe_t> vabc(vz_len, fe_zero());
  {
    std::vector<fe_t> ev[3];
    // bind_matrix_row_vars (:22-41): a scatter into the columns of one matrix - the three matrices side by side
    par_for(3, 1, [&](size_t lo, size_t hi) {
      for (size_t m = lo; m < hi; ++m) {
        ev[m].assign(vcols, fe_zero());
        for (size_t row = 0; row < vcons; ++row) {
          if (fe_is_zero(v_evals_rx[row])) continue;
          for (uint64_t k = vs.M[m].ptr[row]; k < vs.M[m].ptr[row + 1]; ++k)
            ev[m][vs.M[m].idx[k]] = fe_add<S>(ev[m][vs.M[m].idx[k]], fe_mul<S>(v_evals_rx[row], vs.M[m].data[k]));
        }
      }
    });
    const fe_t r2u = fe_mul<S>(vr2, ufold);
    par_for(vcols, 128, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) vabc[i] = fe_add<S>(fe_add<S>(ev[0][i], fe_mul<S>(vr, ev[1][i])), fe_mul<S>(r2u, ev[2][i]));
    });
  }
  st.laps.lap("claim_E + bind_matrix_rows");
  zr.resize(vz_len, fe_zero());
  fe_t ci[2];
  if (host_sc) {
    ck(sp_sumcheck_quad_host(ctx, u64p(&v_claim_inner), vly, u64p(vabc.data()), u64p(zr.data()), tr.t, u64p(st.v_inner.data()), u64p(v_ry.data()), u64p(ci)),
       "relaxed inner sum-check (host tables)");
  } else {
    sp_table *ta = stage(ctx, ps, 3, vabc.data(), vz_len), *tb = stage(ctx, ps, 4, zr.data(), vz_len);
    ck(sp_sumcheck_quad(ctx, u64p(&v_claim_inner), vly, ta, tb, tr.t, u64p(st.v_inner.data()), u64p(v_ry.data()), u64p(ci)), "relaxed inner sum-check");
  }
  st.laps.lap("relaxed inner sc");
  prove_direct(32, Wfold, st.rWfold, v_ry.data() + 1, vly - 1, &st.v_W, &st.blind_vW);
  prove_direct(32, Efold, st.rEfold, v_rx.data(), vlx, &st.v_E, &st.blind_vE);
  tr.absorb_scalars("v_W", st.v_W.data(), st.v_W.size());
  tr.absorb_scalars("v_E", st.v_E.data(), st.v_E.size());
  st.laps.lap("prove_direct x2");
  st.t_vc = st.now();
}

// W = folded_W + c_eval * core_W as a table: only where the opening's halves were not computed ahead
static void nn_fold_W(NNProveState& st, const fe_t& c_eval) {
  const sp_table* two[2] = {st.fW, st.ps.core.W};
  const fe_t wts[2] = {fe_one<S>(), c_eval};
  ck(sp_fold_tables(st.ctx, two, 2, u64p(wts), st.nv, st.Wf), "W = folded_W + c_eval * core_W");
}
// PCS::prove(ck, ck_eval = the width-32 key, transcript, comm, W, blind, r_y[1..], comm_eval, blind_eval) (:2067-2080) as one call
static void nn_open_reference_order(NNProveState& st) {
  const NNZkKey& pk = st.pk;
  Tape& tape = st.tape;
  const size_t CW = st.CW;
  nn_fold_W(st, st.c_eval);
  std::vector<uint64_t> arg(16 + 4 * CW + 8);
  ck(sp_hyrax_prove(st.ctx, pk.ck, pk.vc_ck, st.tr->t, u64p(&st.comm[0].x), st.comm.size(), st.Wf, st.nv, u64p(st.blind.data()), u64p(st.r_y.data() + 1), pk.ny - 1,
                    u64p(&st.comm_eval.x), u64p(&st.blind_eval), tape.bytes + 64 * tape.pos, tape.blocks - tape.pos, arg.data()),
     "PCS::prove");
  tape.skip(CW + 2);
  memcpy(&st.delta, arg.data(), 64);
  memcpy(&st.beta, arg.data() + 8, 64);
  memcpy(st.z_vec.data(), arg.data() + 16, 32 * CW);
  memcpy(&st.z_delta, arg.data() + 16 + 4 * CW, 32);
  memcpy(&st.z_beta, arg.data() + 16 + 4 * CW + 4, 32);
}
// HyraxPCS::prove (hyrax_pc.rs:387-478) + InnerProductArgumentLinear::prove (ipa.rs:125-170) statement by statement, taking what the helper's jobs and the
// products ahead have ready
static void nn_open_side(NNProveState& st) {
  sp_ctx* ctx = st.ctx;
  const NNZkKey& pk = st.pk;
  NNZkPrep& ps = st.ps;
  Tape& tape = st.tape;
  Tr& tr = *st.tr;
  const fe_t c_eval = st.c_eval;
  {
    const std::vector<uint8_t> b = commitment_bytes(st.comm.data(), st.comm.size());
    tr.absorb("poly_com", b.data(), b.size());
  }
  st.laps.lap("pcs: absorb poly_com");
  const fe_t* point = st.r_y.data() + 1;
  const size_t npoint = pk.ny - 1, nvr = st.nvr;
  const std::vector<fe_t> L = eq_evals_host(point, nvr);
  const size_t ncols = (size_t)1 << (npoint - nvr);
  if (st.t_open) ps.wk.wait(st.t_open);
  st.laps.lap("pcs: wait for the opening's points");
  const bool open_ahead = st.t_open && ps.open.delta_valid && ps.open.points_valid && ps.open.tape_from == tape.pos && ncols == ps.open.dv.size();
  std::vector<fe_t> LZ(ncols), Rv;
  NNLzAhead& lz = st.lz;
  lz.step(ctx, ps.core.W, st.r_y.data(), nvr);
  if (lz.have == 2 && lz.f.size() == ncols && lz.c.size() == ncols) {
    const fe_t *lf = lz.f.data(), *lc = lz.c.data();
    par_for(ncols, 256, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) LZ[i] = fe_add<S>(lf[i], fe_mul<S>(c_eval, lc[i]));
    });
  } else {
    nn_fold_W(st, c_eval);
    ck(sp_rowmat_vec(ctx, st.Wf, L.size(), ncols, u64p(L.data()), u64p(LZ.data())), "bind_with_delayed");
  }
  st.laps.lap("pcs: L^T W");
  fe_t r_LZ = fe_zero();
  for (size_t i = 0; i < L.size(); ++i) r_LZ = fe_add<S>(r_LZ, fe_mul<S>(L[i], st.blind[i]));
  std::vector<fe_t> dv;
  fe_t r_delta, r_beta;
  aff_t comm_LZ;
  if (open_ahead) {
    // the helper has delta, beta and the two halves of comm_LZ = <L, rows of (folded + c_eval core)> = P_f + c_eval P_c
    dv.swap(ps.open.dv);
    r_delta = ps.open.r_delta;
    r_beta = ps.open.r_beta;
    tape.skip(ps.open.tape_count);
    st.delta = ps.open.delta;
    st.beta = ps.open.beta;
    fold2_finish_or_call(ctx, ps.open.lz_fold, &ps.open.P_f, &ps.open.P_c, 1, c_eval, &comm_LZ, "comm_LZ = P_f + c_eval P_c");
  } else {
    if (st.laps.on && st.side)
      fprintf(stderr, "nn_prove: opening inputs computed inline (delta %d, points %d, tape %zu vs %zu)\n", (int)ps.open.delta_valid, (int)ps.open.points_valid, ps.open.tape_from, tape.pos);
    // the mask d and its blinds do not depend on the transcript (ipa.rs:139-147): delta's MSM runs on the auxiliary stream beside comm_LZ's
    Rv = eq_evals_host(point + nvr, npoint - nvr);
    dv.resize(Rv.size());
    for (auto& x : dv) x = tape.next();
    r_delta = tape.next();
    r_beta = tape.next();
    sp_msm_job* dj = nullptr;
    ck(sp_msm_ck_begin(ctx, pk.ck, u64p(dv.data()), dv.size(), &dj), "delta (begin)");
    int rc_lz = sp_msm_ck(ctx, pk.ck, u64p(LZ.data()), LZ.size(), u64p(&r_LZ), u64p(&comm_LZ.x));
    int rc_d = sp_msm_ck_finish(ctx, pk.ck, dj, u64p(&r_delta), u64p(&st.delta.x));  // always collected: the job owns device work
    ck(rc_lz, "comm_LZ");
    ck(rc_d, "delta (finish)");
    fe_t ip = fe_zero();
    for (size_t i = 0; i < Rv.size(); ++i) ip = fe_add<S>(ip, fe_mul<S>(Rv[i], dv[i]));
    ck(sp_hyrax_commit_small(ctx, pk.vc_ck, u64p(&ip), 1, u64p(&r_beta), u64p(&st.beta.x)), "beta");
  }
  tr.dom_sep("inner product argument (linear)");
  absorb_ipa_instance(tr, comm_LZ, st.comm_eval, st.delta, st.beta);
  const fe_t rr = tr.squeeze("r");
  st.laps.lap("pcs: comm_LZ + transcript");
  par_for(ncols, 256, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) st.z_vec[i] = fe_add<S>(fe_mul<S>(rr, LZ[i]), dv[i]);
  });
  st.z_delta = fe_add<S>(fe_mul<S>(rr, r_LZ), r_delta);
  st.z_beta = fe_add<S>(fe_mul<S>(rr, st.blind_eval), r_beta);
  st.laps.lap("pcs: z_vec");
}
// fold the two evaluation claims (:2019-2051) and open (:2054-2065); ck_eval = the width-32 key (ck_c = its first base, its h)
static void nn_prove_opening(NNProveState& st) {
  sp_ctx* ctx = st.ctx;
  const vcirc::State& vst = *st.vst;
  const size_t rows = st.rows, inner_final = st.inner_final;
  const std::vector<aff_t>& comm_eW_s = vst.comm_per_round[inner_final + 1];
  const std::vector<aff_t>& comm_eW_c = vst.comm_per_round[inner_final + 2];
  const fe_t c_eval = st.c_eval = st.tr->squeeze("c_eval");
  st.comm.resize(rows);
  if (st.t_fold) st.ps.wk.wait(st.t_fold);  // the folded commitment of the step instances: the helper's second job, started behind the NIFS rounds
  st.laps.lap("pcs: wait for the folded commitment");
  fold2_finish_or_call(ctx, st.fold2.rows, st.f_comm.data(), st.core_comm.data(), rows, c_eval, st.comm.data(), "fold_commitments");
  st.laps.lap("pcs: fold_commitments2 (rows)");
  st.blind.resize(rows);
  for (size_t i = 0; i < rows; ++i) {
    fe_t a;
    memcpy(&a, st.f_rW.data() + 4 * i, 32);
    st.blind[i] = fe_add<S>(a, fe_mul<S>(c_eval, st.core_rW[i]));
  }
  fold2_finish_or_call(ctx, st.fold2.eval, comm_eW_s.data(), comm_eW_c.data(), 1, c_eval, &st.comm_eval, "fold eval commitments");
  st.blind_eval = fe_add<S>(vst.blind_per_round[inner_final + 1][0], fe_mul<S>(c_eval, vst.blind_per_round[inner_final + 2][0]));
  st.laps.lap("pcs: W fold + eval commitment fold");
  st.z_vec.resize(st.CW);
  if (st.reference_order) nn_open_reference_order(st);
  else nn_open_side(st);
  st.t_end = st.now();
}

// the rest of the proof in the canonical layout; phase_ms[8]: see nnz_prove_impl
static ProofBuf nn_prove_emit(NNProveState& st, double* phase_ms) {
  ProofBuf& proof = st.proof;
  const vcirc::State& vst = *st.vst;
  proof.pp(st.delta);
  proof.pp(st.beta);
  for (const fe_t& f : st.z_vec) proof.pf(f);
  proof.pf(st.z_delta);
  proof.pf(st.z_beta);
  for (const auto& c : vst.comm_per_round) proof.pc(c);
  for (const fe_t& f : st.vpub) proof.pf(f);
  for (const auto& cr : vst.challenges)
    for (const fe_t& f : cr) proof.pf(f);
  proof.pc(st.comm_T);
  proof.pc(st.rnd.comm_W);
  proof.pc(st.rnd.comm_E);
  proof.pf(st.rnd_u);
  for (const fe_t& f : st.rnd_X) proof.pf(f);
  for (const fe_t& f : st.v_outer) proof.pf(f);
  for (int i = 0; i < 3; ++i) proof.pf(st.v_claims[i]);
  for (const fe_t& f : st.v_inner) proof.pf(f);
  for (const fe_t& f : st.v_W) proof.pf(f);
  proof.pf(st.blind_vW);
  for (const fe_t& f : st.v_E) proof.pf(f);
  proof.pf(st.blind_vE);
  if (phase_ms) {
    phase_ms[0] = st.t_inst - st.t_start;   // rerandomize + instances
    phase_ms[1] = st.t_nifs - st.t_inst;    // NIFS (layers, rounds, folds, process_round per round)
    phase_ms[2] = st.t_outer - st.t_nifs;   // core products + batched outer sum-check
    phase_ms[3] = st.t_inner - st.t_outer;  // poly_ABC x 2 + batched inner sum-check
    phase_ms[4] = st.t_vc - st.t_inner;     // verifier-circuit instance: random instance, NovaNIFS, relaxed Spartan
    phase_ms[5] = st.t_end - st.t_vc;       // folded opening
    phase_ms[6] = st.t_end - st.t_start;
    phase_ms[7] = vst.commit_ms;  // inside the phases above: the per-round verifier-circuit commitments (process_round)
  }
  if (proof.words.size() != st.pk.layout.words()) throw Error(SP_ERR_INTERNAL, "nn_prove: the proof does not fill the key's layout");
  return std::move(proof);
}

static ProofBuf nn_prove(const NNZkKey& pk, NNZkPrep& ps, Tape& tape, double* phase_ms, bool reference_order = false) {
  NNProveState st(pk, ps, tape, reference_order);
  st.t_start = st.now();
  st.laps.start(st.t_start);
  nn_prove_setup(st);
  nn_prove_rerandomize(st);
  nn_prove_rest_commitments(st);
  nn_prove_instances(st);
  nn_prove_nifs(st);
  nn_prove_outer(st);
  nn_prove_inner(st);
  nn_prove_vc_instance(st);
  nn_prove_random_instance(st);
  nn_prove_nova_nifs(st);
  nn_prove_relaxed_spartan(st);
  nn_prove_opening(st);
  return nn_prove_emit(st, phase_ms);
}

// ---- prove for many prepared states of one key: the two batched sum-checks of all proofs in lockstep ---------------------------------------------------
// `count` NNProveStates over `count` distinct prep states, on the calling thread. Per proof, in order: setup .. NIFS (the NIFS stays per proof). Then the
// part of the outer step in front of its sum-check per proof, ONE sp_sumcheck_cubic_outer_pow_batched_lockstep over the (step, core) pairs of all proofs
// with nn_batched_hook on each proof's NNHookCtx, the part behind it per proof; the inner step likewise around ONE sp_sumcheck_quad_batched_lockstep;
// then verifier-circuit instance .. emit per proof. Each proof's transcript, tape and verifier circuit see exactly the calls nn_prove makes, so the proofs
// and the tape use are nn_prove's. Several states alive on ONE context - what a step leaves begun on st.ctx was checked for being per state:
//   the transcript's asynchronous absorb            per sp_transcript (its own pending job)
//   ps.wk, ps.ctx2 and every job on them            per prep state
//   sp_fold_commitments2_begin (rows, eval)         walker-backed, per job; without a free walk slot _finish computes the plain form
//   sp_ctx_round_hooks_host_only                    per CONTEXT: every state sets the same value and every state's destructor resets it - the states of a
//                                                   group die together, and the lockstep calls queue nothing ahead of a hook whatever it says
//   sp_rowmat_vec_eq_begin (NNLzAhead)              per CONTEXT, one job at a time: left out (nn_prove_inner_after(st, false))
// Batches above SP_LOCKSTEP_PAIRS_MAX run in groups of that size. A failure is rethrown naming the proof; every state's destructor runs with all of the
// group's states alive (drain, collect, drop), so every prep state stays usable.
enum : unsigned { NNZ_BATCH_PER_PROOF = 1, NNZ_BATCH_LOCKSTEP = 2 };
// lockstep from this many proofs on (profiles/nn_prove_batch.md: the smallest count whose lockstep median lies below the minimum of sequential proves)
static const size_t NN_PROVE_BATCH_LOCKSTEP_MIN = (size_t)-1;
struct NNBatchPhases {  // milliseconds, summed over the groups
  double head = 0, outer_before = 0, outer_sc = 0, outer_after = 0, inner_before = 0, inner_sc = 0, inner_after = 0, tail = 0, total = 0, lockstep = 0;
};
template <class F>
static void nn_batch_named(size_t k, F&& f) {
  try {
    f();
  } catch (const Error& e) {
    throw Error(e.code, "prove_batch: proof " + std::to_string(k) + ": " + e.what());
  } catch (const std::exception& e) {
    throw Error(SP_ERR_INTERNAL, "prove_batch: proof " + std::to_string(k) + ": " + e.what());
  }
}
// the lockstep call's failure: a hook's exception belongs to its proof; anything else to the call
static void nn_batch_sumcheck_failed(std::vector<std::unique_ptr<NNProveState>>& st, size_t first, int rc, const char* what) {
  for (size_t k = 0; k < st.size(); ++k)
    if (st[k]->hc.err) nn_batch_named(first + k, [&] { std::rethrow_exception(st[k]->hc.err); });
  ck(rc, what);
}
static void nn_prove_group_lockstep(const NNZkKey& pk, NNZkPrep* const* ps, Tape* tapes, size_t first, size_t count, ProofBuf* out, NNBatchPhases& ph) {
  std::vector<std::unique_ptr<NNProveState>> st;
  for (size_t k = 0; k < count; ++k) st.emplace_back(new NNProveState(pk, *ps[k], tapes[k], false));
  auto each = [&](auto&& step) {
    for (size_t k = 0; k < count; ++k) nn_batch_named(first + k, [&] { step(*st[k]); });
  };
  double t0 = NNLaps::now();
  auto lap = [&](double& into) {
    const double t = NNLaps::now();
    into += t - t0;
    t0 = t;
  };
  each([](NNProveState& s) {
    s.t_start = s.now();
    s.laps.start(s.t_start);
    nn_prove_setup(s);
    nn_prove_rerandomize(s);
    nn_prove_rest_commitments(s);
    nn_prove_instances(s);
    nn_prove_nifs(s);
  });
  lap(ph.head);
  std::vector<void*> users(count);
  std::vector<sp_table*> tb[8];
  std::vector<const sp_table*> pr(count);
  for (auto& v : tb) v.resize(count);
  for (size_t k = 0; k < count; ++k) users[k] = &st[k]->hc;
  // outer
  each(nn_prove_outer_before);
  lap(ph.outer_before);
  {
    std::vector<uint64_t> t_out(4 * count), r_x(4 * count * pk.nx);
    for (size_t k = 0; k < count; ++k) {
      NNProveState& s = *st[k];
      sp_table* const six[6] = {s.A, s.B, s.C, s.core_abc[0], s.core_abc[1], s.core_abc[2]};
      for (int q = 0; q < 6; ++q) tb[q][k] = six[q];
      tb[6][k] = s.pl;
      pr[k] = s.pr;
      memcpy(&t_out[4 * k], s.tail.data(), 32);
    }
    const int rc = sp_sumcheck_cubic_outer_pow_batched_lockstep(pk.ctx, count, pk.nx, tb[6].data(), pr.data(), tb[0].data(), tb[1].data(), tb[2].data(), tb[3].data(),
                                                                tb[4].data(), tb[5].data(), t_out.data(), st[0]->hc.outer_start, nn_batched_hook, users.data(), r_x.data());
    if (rc) nn_batch_sumcheck_failed(st, first, rc, "outer sum-check (batched, lockstep)");
    for (size_t k = 0; k < count; ++k) memcpy(st[k]->r_x.data(), &r_x[4 * k * pk.nx], 32 * pk.nx);
  }
  lap(ph.outer_sc);
  each(nn_prove_outer_after);
  lap(ph.outer_after);
  // inner
  each(nn_prove_inner_before);
  lap(ph.inner_before);
  {
    std::vector<uint64_t> claims(8 * count), r_y(4 * count * pk.ny), fin(16 * count);
    for (size_t k = 0; k < count; ++k) {
      NNProveState& s = *st[k];
      tb[0][k] = s.abc_s, tb[1][k] = s.abc_c, tb[2][k] = s.zs, tb[3][k] = s.zcc;
      memcpy(&claims[8 * k], s.claims, 64);
    }
    const int rc = sp_sumcheck_quad_batched_lockstep(pk.ctx, count, claims.data(), pk.ny, tb[0].data(), tb[1].data(), tb[2].data(), tb[3].data(), st[0]->hc.inner_start,
                                                     nn_batched_hook, users.data(), r_y.data(), fin.data());
    if (rc) nn_batch_sumcheck_failed(st, first, rc, "inner sum-check (batched, lockstep)");
    for (size_t k = 0; k < count; ++k) {
      memcpy(st[k]->r_y.data(), &r_y[4 * k * pk.ny], 32 * pk.ny);
      memcpy(st[k]->fin, &fin[16 * k], 128);
    }
  }
  lap(ph.inner_sc);
  each([](NNProveState& s) { nn_prove_inner_after(s, false); });
  lap(ph.inner_after);
  for (size_t k = 0; k < count; ++k)
    nn_batch_named(first + k, [&] {
      NNProveState& s = *st[k];
      nn_prove_vc_instance(s);
      nn_prove_random_instance(s);
      nn_prove_nova_nifs(s);
      nn_prove_relaxed_spartan(s);
      nn_prove_opening(s);
      out[k] = nn_prove_emit(s, nullptr);
    });
  lap(ph.tail);
}
static std::vector<ProofBuf> nn_prove_batch(const NNZkKey& pk, NNZkPrep* const* ps, Tape* tapes, size_t count, unsigned flags, NNBatchPhases* phases) {
  for (size_t k = 0; k < count; ++k) {
    if (!ps[k]) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: proof " + std::to_string(k) + ": null state");
    for (size_t j = 0; j < k; ++j)
      if (ps[j] == ps[k]) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: the same state twice, proofs " + std::to_string(j) + " and " + std::to_string(k));
  }
  if ((flags & NNZ_BATCH_PER_PROOF) && (flags & NNZ_BATCH_LOCKSTEP)) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: both forms forced");
  const bool lockstep = (flags & NNZ_BATCH_LOCKSTEP) || (!(flags & NNZ_BATCH_PER_PROOF) && count >= NN_PROVE_BATCH_LOCKSTEP_MIN);
  std::vector<ProofBuf> out(count);
  std::vector<Tape> work(tapes, tapes + count);  // the callers' tapes move only when every proof is made
  NNBatchPhases ph;
  const double t0 = NNLaps::now();
  if (lockstep) {
    for (size_t at = 0; at < count; at += SP_LOCKSTEP_PAIRS_MAX)
      nn_prove_group_lockstep(pk, ps + at, work.data() + at, at, std::min<size_t>(SP_LOCKSTEP_PAIRS_MAX, count - at), out.data() + at, ph);
  } else {
    for (size_t k = 0; k < count; ++k) nn_batch_named(k, [&] { out[k] = nn_prove(pk, *ps[k], work[k], nullptr); });
  }
  ph.total = NNLaps::now() - t0;
  ph.lockstep = lockstep ? 1 : 0;
  if (phases) *phases = ph;
  std::copy(work.begin(), work.end(), tapes);
  return out;
}



// ---- NeutronNovaZkSNARK::verify (src/neutronnova_zk.rs:2096-2343) — SURVEY 8(f) rank 3 for caller #2 -----------------------------------------------
// What scales with the step circuits runs on the device through the same ABI: the fold of the step instances' commitments (one shared-weights MSM per
// Hyrax row, hyrax_pc.rs:737-793), the six matrix evaluations A, B, C (rx, ry) of the step and core shapes (ONE sp_multiply_vec against T_y = eq(r_y)
// per shape + three dot products with T_x, `evaluate_with_tables_fast` src/r1cs/mod.rs:1216-1226), comm_LZ = <L, comm rows> and the IPA's <z_vec, ck>
// (hyrax_pc.rs:480-531, ipa.rs:173-221). The verifier-circuit instance (replayed transcript of its per-round commitments, NovaNIFS::verify
// src/nifs.rs:65-77, RelaxedR1CSSpartanProof::verify src/spartan_relaxed.rs:216-316 with its two direct openings hyrax_pc.rs:654-711) is host algebra
// over a few hundred constraints plus small MSMs / two-term folds through the ABI. Returns 0 = accept, else the index of the failed check — the
// oracle's codes (oracle/neutronnova_zk.hpp nn_verify): 1 shape / encoding, 2 verifier-circuit instance does not replay, 4 relaxed Spartan proof,
// 5 public values of the verifier circuit, 6 folded opening.
//
// The check is a sequence of named steps over one NNVerifyState; nn_verify runs them for one proof, nn_verify_batch for many proofs of one key:
//   nn_verify_parse              host only: encoding checks, the views, the regular instances, Uv_X, weights_from_r, Xf, the fold's base rows   (1, 2)
//   nn_fold_commitments_one /    the device work that needs r_b, r_x, r_y alone, for ONE proof (side jobs of nn_verify on the second context);
//   nn_matrix_evaluations_one    the batch issues the same work for all proofs at once (nn_batch_fold, nn_batch_matrix_evaluations)
//   nn_verify_transcript         the transcript, the verifier-circuit replay, NovaNIFS::verify, the relaxed Spartan verify                      (2, 4)
//   nn_verify_publics            the six public values against the matrix evaluations                                                           (5)
//   nn_verify_opening_challenge  the folded opening up to the IPA challenge: comm, comm_eval, comm_LZ, r, <z_vec, R>                            (6)
//   nn_verify_opening_check      the two group equations of one proof                                                                           (6)
struct NNVerifyState {
  NNProofView pv;
  size_t np = 0;
  std::vector<std::vector<aff_t>> Ucomm;
  std::vector<aff_t> core_comm, Uv_comm, fold_bases /* [rows][np] */, folded_comm;
  std::vector<fe_t> core_X, Uv_X, wts, Xf, rhos;
  fe_t eabc[2][3];  // A, B, C (r_x, r_y) of the step and of the core shape
  std::unique_ptr<Tr> tr;
  fe_t tau;
  aff_t comm_LZ, comm_eval;
  fe_t rr, ip;  // the IPA challenge; <z_vec, R>
  ZJob zjob;    // <z_vec, ck> of the single form (the batch forms it once for all proofs)
  NNLaps laps{"nn_verify"};
  void lap(const char* what) { laps.lap(what); }
};

static int nn_verify_parse(const NNZkKey& pk, const uint64_t* words, size_t nwords, NNVerifyState& st) {
  const vcirc::Shape& vs = pk.vc;
  const size_t n = pk.num_steps, dpub = pk.dims.num_public, cpub = pk.dims_core.num_public;
  const NNLayout& lay = pk.layout;
  const size_t rows_sh = lay.rows_sh, rows = lay.rows();
  const size_t vnv = vs.total_vars, VW = vs.width;
  if (n == 0 || nwords != lay.words()) return 1;
  // ---- the proof in its canonical layout; every coordinate and scalar of an untrusted proof must be a canonical residue and every point on the curve
  if (!well_formed(lay, words)) return 1;
  st.pv = lay.view(words);
  const NNProofView& pv = st.pv;
  const aff_t* comm_shared = pv.comm_shared;
  // regular instances: comm_W = shared | precommitted | rest rows, X = the public values (src/r1cs/mod.rs:1723-1760)
  auto regular = [&](const NNProofView::Inst& u, size_t my_pre, size_t my_rest) {
    std::vector<aff_t> c(rows);
    std::copy(comm_shared, comm_shared + rows_sh, c.begin());
    std::copy(u.pre, u.pre + my_pre, c.begin() + rows_sh);
    std::copy(u.rest, u.rest + my_rest, c.begin() + rows_sh + my_pre);
    return c;
  };
  size_t np = 2;
  while (np < n) np <<= 1;
  st.np = np;
  const size_t nb = pk.nb, nx = pk.nx, ny = pk.ny;
  if (((size_t)1 << nb) != np) throw Error(SP_ERR_INTERNAL, "nn_verify: a single step instance is not driven by this layer");
  auto inst = [&](size_t i) { return i < n ? i : 0; };  // padding clones instance 0 (:549-552)
  st.Ucomm.resize(n);
  for (size_t i = 0; i < n; ++i) st.Ucomm[i] = regular(pv.steps[i], lay.rows_pre, lay.rows_rest);
  st.core_comm = regular(pv.core, lay.rows_pre_c, lay.rows_rest_c);
  st.core_X.assign(pv.core.pub, pv.core.pub + cpub);
  // the verifier-circuit instance in its regular form: comm_W = the rounds' rows, X = challenges | public values; the challenges are checked against the
  // transcript (nn_verify_transcript), what is computed from them before that is only used after the check
  st.Uv_comm.assign(pv.vcomm[0], pv.vcomm[0] + vnv / VW);  // the rounds are consecutive in the layout
  std::vector<fe_t>& Uv_X = st.Uv_X;
  Uv_X.clear();
  for (size_t r = 0; r < vs.num_rounds; ++r) Uv_X.insert(Uv_X.end(), pv.vchal[r], pv.vchal[r] + vs.chals_per_round[r]);
  Uv_X.insert(Uv_X.end(), pv.vpub, pv.vpub + vs.num_public);
  const size_t num_chal = nb + nx + 1 + ny;
  if (vs.total_challenges != num_chal || vs.num_public != 6) return 2;
  const fe_t* r_b = Uv_X.data();
  // fold_multiple of the step instances (src/r1cs/mod.rs:695-722): X on the host, the commitment rows as shared-weights MSMs
  st.wts.resize(np);
  ck(sp_weights_from_r(u64p(r_b), nb, np, u64p(st.wts.data())), "weights_from_r");
  st.Xf.assign(dpub, fe_zero());
  for (size_t i = 0; i < np; ++i)
    for (size_t j = 0; j < dpub; ++j) st.Xf[j] = fe_add<S>(st.Xf[j], fe_mul<S>(st.wts[i], pv.steps[inst(i)].pub[j]));
  st.folded_comm.resize(rows);
  st.fold_bases.resize(rows * np);
  for (size_t rr = 0; rr < rows; ++rr)
    for (size_t i = 0; i < np; ++i) st.fold_bases[rr * np + i] = st.Ucomm[inst(i)][rr];
  return 0;
}

// fold_commitments of one proof's step instances (hyrax_pc.rs:737-793): one shared-weights MSM over its rows
static void nn_fold_commitments_one(const NNZkKey& pk, sp_ctx* on, NNVerifyState& st) {
  ck(sp_msm_shared_weights(on, u64p(st.wts.data()), st.np, reinterpret_cast<const uint64_t*>(st.fold_bases.data()), pk.layout.rows(),
                           reinterpret_cast<uint64_t*>(st.folded_comm.data())),
     "fold_commitments");
}
// the matrix evaluations A, B, C (r_x, r_y) of the step and core shapes of one proof: T_x^T (M T_y)
static void nn_matrix_evaluations_one(const NNZkKey& pk, sp_ctx* on, NNVerifyState& st) {
  const size_t nb = pk.nb, nx = pk.nx, ny = pk.ny, nv = pk.num_vars, N = pk.dims.num_cons, dpub = pk.dims.num_public, cpub = pk.dims_core.num_public;
  const fe_t *r_x = st.Uv_X.data() + nb, *r_y = r_x + nx + 1;
  if (!pk.v_Tx) {
    ck(sp_table_zeros(on, (size_t)1 << nx, (size_t)-1, (size_t)-1, &pk.v_Tx), "T_x alloc");
    ck(sp_table_zeros(on, (size_t)1 << ny, (size_t)-1, (size_t)-1, &pk.v_Ty), "T_y alloc");
    for (int i = 0; i < 3; ++i) ck(sp_table_zeros(on, N, (size_t)-1, (size_t)-1, &pk.v_mv[i]), "M T_y alloc");
  }
  sp_table *Tx = pk.v_Tx, *Ty = pk.v_Ty, **mv = pk.v_mv;
  ck(sp_table_set_len(Tx, (size_t)1 << nx, (size_t)-1, (size_t)-1), "T_x len");
  ck(sp_table_set_len(Ty, (size_t)1 << ny, (size_t)-1, (size_t)-1), "T_y len");
  ck(sp_eq_table_into(on, u64p(r_x), nx, Tx), "T_x");
  ck(sp_eq_table_into(on, u64p(r_y), ny, Ty), "T_y");
  const sp_shape* shapes[2] = {pk.S_step, pk.S_core};
  const size_t cols[2] = {nv + 1 + dpub, nv + 1 + cpub};
  for (int s2 = 0; s2 < 2; ++s2) {
    ck(sp_table_set_len(Ty, cols[s2], (size_t)-1, (size_t)-1), "T_y as z");
    ck(sp_multiply_vec(on, shapes[s2], Ty, mv[0], mv[1], mv[2]), "M T_y");
    for (int i = 0; i < 3; ++i) ck(sp_table_dot(on, Tx, mv[i], N, u64p(&st.eabc[s2][i])), "T_x . (M T_y)");
  }
}

// the transcript up to the relaxed Spartan proof: 0, or 2 (the verifier-circuit instance does not replay), or 4 (relaxed Spartan)
static int nn_verify_transcript(const NNZkKey& pk, NNVerifyState& st) {
  sp_ctx* ctx = pk.ctx;
  const vcirc::Shape& vs = pk.vc;
  const size_t n = pk.num_steps, np = st.np, nb = pk.nb, dpub = pk.dims.num_public;
  const size_t vnv = vs.total_vars, vcons = vs.num_cons, vio = vs.num_io(), vlx = log2_ceil(vcons), vnvp = next_pow2(vnv), vly = log2_ceil(vnvp) + 1, VW = vs.width;
  const NNProofView& pv = st.pv;
  const aff_t *comm_T = pv.comm_T, *rnd_comm_W = pv.rnd_comm_W, *rnd_comm_E = pv.rnd_comm_E;
  const fe_t *rnd_X = pv.rnd_X, *v_outer = pv.v_outer, *v_claims = pv.v_claims, *v_inner = pv.v_inner, *v_W = pv.v_W, *v_E = pv.v_E;
  const fe_t rnd_u = *pv.rnd_u, blind_vW = *pv.blind_vW, blind_vE = *pv.blind_vE, one = fe_one<S>();
  const std::vector<std::vector<aff_t>>& Ucomm = st.Ucomm;
  const std::vector<aff_t>&core_comm = st.core_comm, &Uv_comm = st.Uv_comm;
  const std::vector<fe_t>&core_X = st.core_X, &Uv_X = st.Uv_X;
  std::vector<fe_t>& rhos = st.rhos;
  auto inst = [&](size_t i) { return i < n ? i : 0; };
  auto lap = [&](const char* what) { st.lap(what); };
  st.tr.reset(new Tr(ctx, "neutronnova_prove"));
  Tr& tr = *st.tr;
  absorb_head(tr, pk, core_comm, core_X);
  for (size_t i = 0; i < np; ++i) absorb_instance(tr, "U", Ucomm[inst(i)], std::vector<fe_t>(pv.steps[inst(i)].pub, pv.steps[inst(i)].pub + dpub));
  {
    uint8_t zero_be[32] = {0};  // T = 0 (:556-557)
    tr.absorb("T", zero_be, 32);
  }
  st.tau = tr.squeeze("tau");
  rhos.assign(nb, fe_zero());
  for (auto& x : rhos) x = tr.squeeze("rho");
  lap("instances absorbed");
  // U_verifier.validate (src/r1cs/mod.rs:1808-1834): the per-round commitments reproduce the challenges the instance carries
  for (size_t round = 0; round < vs.num_rounds; ++round) {
    const std::vector<uint8_t> b = commitment_bytes(pv.vcomm[round], vs.vars_padded[round] / VW);
    tr.absorb("comm_w_round", b.data(), b.size());
    for (size_t i = 0; i < vs.chals_per_round[round]; ++i)
      if (!fe_eq(tr.squeeze("challenge"), pv.vchal[round][i])) return 2;
  }
  lap("vc instance replayed");
  // NovaNIFS::verify (src/nifs.rs:65-77): the random relaxed instance folded with the verifier-circuit instance
  absorb_U1(tr, rnd_comm_W, vnv / VW, rnd_comm_E, vcons / VW, rnd_u, rnd_X, vio);
  absorb_instance(tr, "U2", Uv_comm, Uv_X);
  absorb_comm_T(tr, comm_T, vcons / VW);
  const fe_t rf = tr.squeeze("r");
  std::vector<aff_t> fU_W(vnv / VW), fU_E(vcons / VW);
  ck(sp_fold_commitments2(ctx, u64p(&rnd_comm_W[0].x), u64p(&Uv_comm[0].x), fU_W.size(), u64p(&rf), u64p(&fU_W[0].x)), "fold comm_W");
  ck(sp_fold_commitments2(ctx, u64p(&rnd_comm_E[0].x), u64p(&comm_T[0].x), fU_E.size(), u64p(&rf), u64p(&fU_E[0].x)), "fold comm_E");
  const fe_t fU_u = fe_add<S>(rnd_u, rf);
  std::vector<fe_t> fU_X(vio);
  for (size_t i = 0; i < vio; ++i) fU_X[i] = fe_add<S>(rnd_X[i], fe_mul<S>(rf, Uv_X[i]));
  lap("NovaNIFS::verify");
  // RelaxedR1CSSpartanProof::verify (src/spartan_relaxed.rs:216-316)
  {
    // verify_direct (hyrax_pc.rs:654-711) under the width-32 key: <L, comm rows> must equal <v, ck> + cb * h; returns the evaluation <v, R>
    auto verify_direct = [&](const std::vector<aff_t>& comm, const fe_t* v, const fe_t& cb, const fe_t* point, size_t npoint, fe_t* eval) {
      const size_t nn = (size_t)1 << npoint, drows = (nn + VW - 1) / VW, nvr = log2_ceil(drows);
      aff_t comm_LZ;
      if (nvr == 0) {
        comm_LZ = comm[0];
      } else {
        const std::vector<fe_t> L = eq_evals_host(point, nvr);
        if (comm.size() > L.size()) return false;
        ck(sp_msm(ctx, u64p(L.data()), u64p(&comm[0].x), comm.size(), u64p(&comm_LZ.x)), "direct opening: <L, rows>");
      }
      aff_t expected;
      ck(sp_hyrax_commit_small(ctx, pk.vc_ck, u64p(v), VW, u64p(&cb), u64p(&expected.x)), "direct opening: <v, ck> + cb h");
      if (!fe_eq(comm_LZ.x, expected.x) || !fe_eq(comm_LZ.y, expected.y)) return false;
      const std::vector<fe_t> R = eq_evals_host(point + nvr, npoint - nvr);
      fe_t e = fe_zero();
      for (size_t i = 0; i < VW; ++i) e = fe_add<S>(e, fe_mul<S>(v[i], R[i]));
      *eval = e;
      return true;
    };
    tr.absorb_scalars("u_relaxed", &fU_u, 1);
    tr.absorb_scalars("X_relaxed", fU_X.data(), fU_X.size());
    std::vector<fe_t> vtau(vlx);
    for (auto& t : vtau) t = tr.squeeze("t");
    fe_t claim_outer_final, claim_inner_final;
    std::vector<fe_t> vrx, vry;
    if (!sumcheck_verify(tr, fe_zero(), vlx, 3, v_outer, &claim_outer_final, &vrx)) return 4;
    fe_t eq_tau = one;  // EqPolynomial::evaluate (src/polys/eq.rs:45-57)
    for (size_t i = 0; i < vlx; ++i) eq_tau = fe_mul<S>(eq_tau, fe_add<S>(fe_mul<S>(vtau[i], vrx[i]), fe_mul<S>(fe_sub<S>(one, vtau[i]), fe_sub<S>(one, vrx[i]))));
    if (!fe_eq(claim_outer_final, fe_mul<S>(eq_tau, fe_sub<S>(fe_mul<S>(v_claims[0], v_claims[1]), v_claims[2])))) return 4;
    tr.absorb_scalars("claims_outer", v_claims, 3);
    const fe_t vr = tr.squeeze("r"), vr2 = fe_mul<S>(vr, vr);
    fe_t eval_E, eval_W;
    if (!verify_direct(fU_E, v_E, blind_vE, vrx.data(), vlx, &eval_E)) return 4;
    const fe_t minus_E[3] = {v_claims[0], v_claims[1], fe_sub<S>(v_claims[2], eval_E)};
    const fe_t claim_inner = joint_inner_claim(minus_E, vr, vr2);
    if (!sumcheck_verify(tr, claim_inner, vly, 2, v_inner, &claim_inner_final, &vry)) return 4;
    if (!verify_direct(fU_W, v_W, blind_vW, vry.data() + 1, vly - 1, &eval_W)) return 4;
    const std::vector<fe_t> Tx = eq_evals_host(vrx.data(), vlx), Ty = eq_evals_host(vry.data(), vly);
    fe_t eval_Z = fe_add<S>(fe_mul<S>(fe_sub<S>(one, vry[0]), eval_W), fe_mul<S>(fU_u, Ty[vnv]));
    for (size_t j = 0; j < vio; ++j) eval_Z = fe_add<S>(eval_Z, fe_mul<S>(fU_X[j], Ty[vnv + 1 + j]));
    fe_t em[3];  // evaluate_with_tables on the verifier-circuit matrices (spartan_relaxed.rs:44-67)
    for (int m = 0; m < 3; ++m) {
      fe_t acc = fe_zero();
      for (size_t row = 0; row < vcons; ++row) {
        if (fe_is_zero(Tx[row])) continue;
        fe_t rs = fe_zero();
        for (uint64_t k = vs.M[m].ptr[row]; k < vs.M[m].ptr[row + 1]; ++k) rs = fe_add<S>(rs, fe_mul<S>(Ty[vs.M[m].idx[k]], vs.M[m].data[k]));
        acc = fe_add<S>(acc, fe_mul<S>(Tx[row], rs));
      }
      em[m] = acc;
    }
    const fe_t eval_ABC = fe_add<S>(fe_add<S>(em[0], fe_mul<S>(vr, em[1])), fe_mul<S>(fe_mul<S>(vr2, fU_u), em[2]));
    if (!fe_eq(claim_inner_final, fe_mul<S>(eval_ABC, eval_Z))) return 4;
    tr.absorb_scalars("v_W", v_W, VW);
    tr.absorb_scalars("v_E", v_E, VW);
  }
  lap("relaxed Spartan verify");
  return 0;
}

// the six public values of the verifier circuit (:2280-2330): tau(r_x), the X evaluations, eq(r_b, rho) and the matrix evaluations at (r_x, r_y),
// which st.eabc holds by now. 0 or 5.
static int nn_verify_publics(const NNZkKey& pk, NNVerifyState& st) {
  const size_t nb = pk.nb, nx = pk.nx, ny = pk.ny, dpub = pk.dims.num_public, cpub = pk.dims_core.num_public;
  const NNProofView& pv = st.pv;
  const std::vector<fe_t>&Uv_X = st.Uv_X, &Xf = st.Xf, &rhos = st.rhos;
  const fe_t *r_b = Uv_X.data(), *r_x = r_b + nb, *r_y = r_x + nx + 1, *pub = Uv_X.data() + (nb + nx + 1 + ny);
  const fe_t r = Uv_X[nb + nx], r2 = fe_mul<S>(r, r), one = fe_one<S>(), tau = st.tau;
  const fe_t(*eabc)[3] = st.eabc;
  {
    auto eval_X = [&](const fe_t* Xv, size_t cnt) { return nn_eval_X(ny, Xv, cnt, r_y); };
    const fe_t q_step = joint_inner_claim(eabc[0], r, r2), q_core = joint_inner_claim(eabc[1], r, r2);
    fe_t tau_at_rx = one, p = tau;  // PowPolynomial::evaluate (src/polys/power.rs:33-50): tau^(2^i) pairs with the i-th variable from the end
    for (size_t i = 0; i < nx; ++i) {
      tau_at_rx = fe_mul<S>(tau_at_rx, fe_add<S>(one, fe_mul<S>(fe_sub<S>(p, one), r_x[nx - 1 - i])));
      p = fe_mul<S>(p, p);
    }
    fe_t eq_rho = one;
    for (size_t i = 0; i < nb; ++i) eq_rho = fe_mul<S>(eq_rho, fe_add<S>(fe_mul<S>(rhos[i], r_b[i]), fe_mul<S>(fe_sub<S>(one, rhos[i]), fe_sub<S>(one, r_b[i]))));
    if (!fe_eq(pub[0], tau_at_rx) || !fe_eq(pub[1], eval_X(Xf.data(), dpub)) || !fe_eq(pub[2], eval_X(pv.core.pub, cpub)) || !fe_eq(pub[3], eq_rho) || !fe_eq(pub[4], q_step) ||
        !fe_eq(pub[5], q_core))
      return 5;
  }
  st.lap("matrix evaluations + publics");
  return 0;
}

// the folded opening (:2332-2343) up to the IPA challenge: HyraxPCS::verify (hyrax_pc.rs:480-531) + InnerProductArgumentLinear::verify (ipa.rs:173-194).
// Needs st.folded_comm. Leaves comm_LZ, comm_eval, the challenge rr and ip = <z_vec, R>. 0 or 6.
static int nn_verify_opening_challenge(const NNZkKey& pk, NNVerifyState& st) {
  sp_ctx* ctx = pk.ctx;
  const vcirc::Shape& vs = pk.vc;
  const size_t CW = DEFAULT_COMMITMENT_WIDTH, nb = pk.nb, nx = pk.nx, ny = pk.ny, rows = pk.layout.rows();
  const NNProofView& pv = st.pv;
  const std::vector<aff_t>&folded_comm = st.folded_comm, &core_comm = st.core_comm;
  const fe_t *r_y = st.Uv_X.data() + nb + nx + 1, *z_vec = pv.z_vec;
  const aff_t delta = *pv.delta, beta = *pv.beta;
  Tr& tr = *st.tr;
  aff_t &comm_LZ = st.comm_LZ, &comm_eval = st.comm_eval;
  const fe_t c_eval = tr.squeeze("c_eval");
  const size_t commit_round = nb + 1 + nx + 1 + ny + 1;
  if (commit_round + 1 >= vs.num_rounds) throw Error(SP_ERR_INTERNAL, "nn_verify: verifier-circuit round layout");
  std::vector<aff_t> comm(rows);
  ck(sp_fold_commitments2(ctx, u64p(&folded_comm[0].x), u64p(&core_comm[0].x), rows, u64p(&c_eval), u64p(&comm[0].x)), "fold_commitments");
  ck(sp_fold_commitments2(ctx, u64p(&pv.vcomm[commit_round][0].x), u64p(&pv.vcomm[commit_round + 1][0].x), 1, u64p(&c_eval), u64p(&comm_eval.x)), "fold eval commitments");
  {
    const std::vector<uint8_t> b = commitment_bytes(comm.data(), rows);
    tr.absorb("poly_com", b.data(), b.size());
  }
  const fe_t* point = r_y + 1;
  const size_t npoint = ny - 1, num_rows = (((size_t)1 << npoint) + CW - 1) / CW, nvr = log2_ceil(num_rows);
  std::vector<fe_t> R;
  if (nvr == 0) {
    comm_LZ = comm[0];
    R = eq_evals_host(point, npoint);
  } else {
    const std::vector<fe_t> L = eq_evals_host(point, nvr);
    R = eq_evals_host(point + nvr, npoint - nvr);
    if (rows < L.size()) return 6;
    ck(sp_msm(ctx, u64p(L.data()), u64p(&comm[0].x), L.size(), u64p(&comm_LZ.x)), "comm_LZ");
  }
  if (R.size() != CW) return 6;
  tr.dom_sep("inner product argument (linear)");
  absorb_ipa_instance(tr, comm_LZ, comm_eval, delta, beta);
  st.rr = tr.squeeze("r");
  fe_t ip = fe_zero();
  for (size_t i = 0; i < CW; ++i) ip = fe_add<S>(ip, fe_mul<S>(z_vec[i], R[i]));
  st.ip = ip;
  return 0;
}

// the group equations of one proof (ipa.rs:196-221): r comm_LZ + delta == <z_vec, ck> + z_delta h and r comm_eval + beta == <z_vec, R> ck_c + z_beta h_c. 0 or 6.
static int nn_verify_opening_check(const NNZkKey& pk, NNVerifyState& st) {
  sp_ctx* ctx = pk.ctx;
  const NNProofView& pv = st.pv;
  const aff_t delta = *pv.delta, beta = *pv.beta;
  const fe_t z_delta = *pv.z_delta, z_beta = *pv.z_beta;
  aff_t pr2[2] = {st.comm_LZ, st.comm_eval}, rp[2], hzd, rhs2;
  ck(sp_vartime_scalar_mul(ctx, u64p(&pr2[0].x), 2, u64p(&st.rr), u64p(&rp[0].x)), "r * (comm_LZ, comm_eval)");
  ck(sp_fixed_base_mul_h(ctx, pk.ck, u64p(&z_delta), 1, u64p(&hzd.x)), "h * z_delta");
  ck(sp_hyrax_commit_small(ctx, pk.vc_ck, u64p(&st.ip), 1, u64p(&z_beta), u64p(&rhs2.x)), "<z, R> * ck_c + z_beta * h_c");
  aff_t zc;
  {
    st.zjob.ctx = ctx;
    st.zjob.key = pk.ck;
    if (!st.zjob.job) ck(sp_msm_ck_begin(ctx, pk.ck, u64p(pv.z_vec), DEFAULT_COMMITMENT_WIDTH, &st.zjob.job), "<z, ck> (begin)");  // (a batch's fallback: nn_verify began it)
    sp_msm_job* j = st.zjob.job;
    st.zjob.job = nullptr;
    ck(sp_msm_ck_finish(ctx, pk.ck, j, nullptr, u64p(&zc.x)), "<z, ck> (finish)");
  }
  if (!same_point(jac_add_mixed(jac_from_affine(rp[0]), delta), jac_add_mixed(jac_from_affine(zc), hzd))) return 6;
  if (!same_point(jac_add_mixed(jac_from_affine(rp[1]), beta), jac_from_affine(rhs2))) return 6;
  st.lap("folded opening");
  return 0;
}

static int nn_verify(const NNZkKey& pk, const uint64_t* words, size_t nwords) {
  sp_ctx* ctx = pk.ctx;
  if (pk.num_steps == 0 || nwords != pk.layout.words()) return 1;
  ck(sp_ctx_bind_thread(ctx), "device");
  NNVerifyState st;
  st.laps.start(NNLaps::now());
  int code;
  if ((code = nn_verify_parse(pk, words, nwords, st)) == 1) return 1;
  st.lap("parse + encoding checks");
  // <z_vec, ck> (ipa.rs:196-203) depends on nothing but the proof: its device part runs under everything that follows
  st.zjob.ctx = ctx;
  st.zjob.key = pk.ck;
  ck(sp_msm_ck_begin(ctx, pk.ck, u64p(st.pv.z_vec), DEFAULT_COMMITMENT_WIDTH, &st.zjob.job), "<z, ck> (begin)");
  if (code) return code;
  // r_b, r_x and r_y are words of the proof: the commitment fold and the matrix evaluations run as jobs on the second context beside the transcript work
  struct Drain {  // the jobs read and write `st`
    Worker& w;
    ~Drain() { w.drain(); }
  } drain{pk.v_wk};
  if (!pk.v_ctx2) ck(sp_ctx_create(sp_ctx_device(ctx), &pk.v_ctx2), "second context");
  const size_t t_fold = pk.v_wk.submit([&] {
    ck(sp_ctx_bind_thread(pk.v_ctx2), "device");
    nn_fold_commitments_one(pk, pk.v_ctx2, st);
  });
  const size_t t_mat = pk.v_wk.submit([&] { nn_matrix_evaluations_one(pk, pk.v_ctx2, st); });
  if ((code = nn_verify_transcript(pk, st))) return code;
  pk.v_wk.wait(t_mat);
  if ((code = nn_verify_publics(pk, st))) return code;
  pk.v_wk.wait(t_fold);
  if ((code = nn_verify_opening_challenge(pk, st))) return code;
  return nn_verify_opening_check(pk, st);
}

// ---- verify_batch: `count` proofs under one key in one pass -----------------------------------------------------------------------------------------------
// codes[k] == nn_verify(proof k) for every k; a batch of one IS nn_verify. What the proofs of a batch share is paid once:
//   parse       nn_verify_parse per proof on host threads (it touches no context);
//   shared      on the second context's worker, as nn_verify's side jobs: ONE sp_msm_shared_weights_grouped for the step-instance folds of all proofs that
//               parsed, and the matrix evaluations of S_step and S_core through sp_shape_matrix_evals_batched per chunk of sp_shape_matrix_evals_chunk()
//               proofs (the chunk's eq tables are kept on the key; T_y is cut to each shape's column count) - no product tables, no per-proof launches;
//   per proof   on the calling thread, each proof in nn_verify's order: nn_verify_transcript of every proof (the shared stage runs under all of it), then
//               nn_verify_publics, then nn_verify_opening_challenge. This part stays sequential: sp_fold_commitments2, sp_msm, sp_hyrax_commit_small and
//               the transcript's hash calls drive pk.ctx, and a context is one thread's. Nothing of it was moved to host threads;
//   opening     the group equations of all survivors as one random linear combination (as spartan2::verify_batch):
//                 sum_k rho_k (r_k comm_LZ_k + delta_k)  ==  < sum_k rho_k z_vec_k, ck >  +  (sum_k rho_k z_delta_k) h
//                 sum_k rho'_k (r_k comm_eval_k + beta_k)  ==  (sum_k rho'_k <z_vec_k, R_k>) ck_c  +  (sum_k rho'_k z_beta_k) h_c
//               (comm_eval_k is a fold of two proof points, not a commitment the verifier forms: it stays on the point side.) If either fails,
//               nn_verify_opening_check names the proofs with code 6 one by one.
// rho_k = w[2 k], rho'_k = w[2 k + 1] from the transcript "NeutronNovaZkSNARK::verify_batch": absorb "vk" (digest), "count" (K, 8 bytes LE), per proof in
// batch order "proof_len" (words, 8 bytes LE) and "proof" (the words, LE), then "seed" (32 bytes) if the caller gave one; squeeze "rho" 2 K times.
enum { NNZ_VERIFY_BATCH_PER_PROOF = 1, NNZ_VERIFY_BATCH_SHARED = 2 };  // flags of nnz_verify_batch_opts: force one form (0 = by count, NN_VERIFY_BATCH_MIN)
// the smallest batch the shared form takes by default: the smallest measured K at which its median lay below the minimum of K verify calls
// (profiles/nn_verify_batch.md: not at K = 2, where the combined opening's fixed cost outweighs what two proofs share; at K = 4 in some runs and not in
// the recorded one, 0.98 x either way; at K = 8 and 16 in every run)
static const size_t NN_VERIFY_BATCH_MIN = 8;

static std::vector<fe_t> nn_batch_weights(const NNZkKey& pk, const uint64_t* const* words, const size_t* nwords, size_t count, const uint8_t* seed) {
  Tr tr(pk.ctx, "NeutronNovaZkSNARK::verify_batch");
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

// the step-instance folds of the proofs `live` in one grouped call: group g = proof live[g], its weights and its [rows][np] base rows
static void nn_batch_fold(const NNZkKey& pk, sp_ctx* on, std::vector<NNVerifyState>& st, const std::vector<size_t>& live) {
  const size_t G = live.size(), rows = pk.layout.rows(), np = st[live[0]].np;
  std::vector<fe_t> w(G * np);
  std::vector<aff_t> bases(G * rows * np), out(G * rows);
  for (size_t g = 0; g < G; ++g) {
    const NNVerifyState& s = st[live[g]];
    std::copy(s.wts.begin(), s.wts.end(), w.begin() + g * np);
    std::copy(s.fold_bases.begin(), s.fold_bases.end(), bases.begin() + g * rows * np);
  }
  ck(sp_msm_shared_weights_grouped(on, u64p(w.data()), np, reinterpret_cast<const uint64_t*>(bases.data()), rows, G, reinterpret_cast<uint64_t*>(out.data())),
     "fold_commitments (grouped)");
  for (size_t g = 0; g < G; ++g) std::copy(out.begin() + g * rows, out.begin() + (g + 1) * rows, st[live[g]].folded_comm.begin());
}
// A, B, C (r_x, r_y) of S_step and S_core for the proofs `live`, a chunk of proofs per pair of launches; *chunks counts the sp_shape_matrix_evals_batched calls
static void nn_batch_matrix_evaluations(const NNZkKey& pk, sp_ctx* on, std::vector<NNVerifyState>& st, const std::vector<size_t>& live, uint64_t* chunks) {
  const size_t KC = sp_shape_matrix_evals_chunk(), nb = pk.nb, nx = pk.nx, ny = pk.ny, nv = pk.num_vars;
  if (pk.vb_Tx.empty()) {
    for (size_t j = 0; j < KC; ++j) {
      sp_table *tx = nullptr, *ty = nullptr;
      ck(sp_table_zeros(on, (size_t)1 << nx, (size_t)-1, (size_t)-1, &tx), "T_x alloc");
      pk.vb_Tx.push_back(tx);
      ck(sp_table_zeros(on, (size_t)1 << ny, (size_t)-1, (size_t)-1, &ty), "T_y alloc");
      pk.vb_Ty.push_back(ty);
    }
  }
  const sp_shape* shapes[2] = {pk.S_step, pk.S_core};
  const size_t cols[2] = {nv + 1 + pk.dims.num_public, nv + 1 + pk.dims_core.num_public};
  for (size_t c0 = 0; c0 < live.size(); c0 += KC) {
    const size_t kc = std::min(KC, live.size() - c0);
    for (size_t j = 0; j < kc; ++j) {
      const fe_t *r_x = st[live[c0 + j]].Uv_X.data() + nb, *r_y = r_x + nx + 1;
      ck(sp_table_set_len(pk.vb_Ty[j], (size_t)1 << ny, (size_t)-1, (size_t)-1), "T_y len");
      ck(sp_eq_table_into(on, u64p(r_x), nx, pk.vb_Tx[j]), "T_x");
      ck(sp_eq_table_into(on, u64p(r_y), ny, pk.vb_Ty[j]), "T_y");
    }
    std::vector<fe_t> e(3 * kc);
    for (int s2 = 0; s2 < 2; ++s2) {
      for (size_t j = 0; j < kc; ++j) ck(sp_table_set_len(pk.vb_Ty[j], cols[s2], (size_t)-1, (size_t)-1), "T_y as z");
      ck(sp_shape_matrix_evals_batched(on, shapes[s2], pk.vb_Tx.data(), pk.vb_Ty.data(), kc, u64p(e.data())), "matrix_evals_batched");
      ++*chunks;
      for (size_t j = 0; j < kc; ++j)
        for (int m = 0; m < 3; ++m) st[live[c0 + j]].eabc[s2][m] = e[3 * j + m];
    }
  }
}

static void nn_verify_batch(const NNZkKey& pk, const uint64_t* const* words, const size_t* nwords, size_t count, const uint8_t* seed, int* codes,
                            ss_verify_batch_info* info, unsigned flags) {
  sp_ctx* ctx = pk.ctx;
  ss_verify_batch_info inf{0, 1, 0, 0};
  if (info) *info = inf;
  if (count == 0) return;
  const bool shared = (flags & NNZ_VERIFY_BATCH_SHARED) ? true : (flags & NNZ_VERIFY_BATCH_PER_PROOF) ? false : count >= NN_VERIFY_BATCH_MIN;
  if (count == 1 || !shared) {  // nothing to share, or not enough of it: the single-proof form, proof after proof
    for (size_t k = 0; k < count; ++k) codes[k] = nn_verify(pk, words[k], nwords[k]);
    return;
  }
  ck(sp_ctx_bind_thread(ctx), "device");  // the caller may be a thread other than the one that created the context
  // the weights need the proofs alone: hashed on a thread of their own under everything up to the combined opening
  std::future<std::vector<fe_t>> weights = std::async(std::launch::async, [&] { return nn_batch_weights(pk, words, nwords, count, seed); });
  struct Join {
    std::future<std::vector<fe_t>>& f;
    ~Join() {
      if (f.valid()) f.wait();
    }
  } join{weights};
  std::vector<NNVerifyState> st(count);
  parallel_for(count, (size_t)1 << 20, [&](size_t k) { codes[k] = nn_verify_parse(pk, words[k], nwords[k], st[k]); });
  std::vector<size_t> live;
  for (size_t k = 0; k < count; ++k)
    if (codes[k] == 0) live.push_back(k);
  if (live.empty()) return;
  // the shared device stage, on the second context's worker beside the transcript work below
  const std::vector<size_t> parsed = live;  // (declared before the guard: the jobs read it until they are drained, on every exit)
  struct Drain {  // the jobs read `parsed` and read and write `st` and `inf`: all three outlive this guard
    Worker& w;
    ~Drain() { w.drain(); }
  } drain{pk.v_wk};
  if (!pk.v_ctx2) ck(sp_ctx_create(sp_ctx_device(ctx), &pk.v_ctx2), "second context");
  const size_t t_mat = pk.v_wk.submit([&] {  // (needed first: check 5 comes before the opening)
    ck(sp_ctx_bind_thread(pk.v_ctx2), "device");
    nn_batch_matrix_evaluations(pk, pk.v_ctx2, st, parsed, &inf.matrix_chunks);
  });
  const size_t t_fold = pk.v_wk.submit([&] { nn_batch_fold(pk, pk.v_ctx2, st, parsed); });
  // per proof, every proof in nn_verify's order (each has its own transcript): the transcript step of all proofs first, so that the shared stage has the
  // whole batch's transcript work to run under, then the public values of all, then the opening up to its challenge
  auto step = [&](auto&& f) {
    std::vector<size_t> next;
    for (size_t k : live)
      if ((codes[k] = f(st[k])) == 0) next.push_back(k);
    live.swap(next);
  };
  step([&](NNVerifyState& s) { return nn_verify_transcript(pk, s); });
  pk.v_wk.wait(t_mat);
  step([&](NNVerifyState& s) { return nn_verify_publics(pk, s); });
  pk.v_wk.wait(t_fold);
  step([&](NNVerifyState& s) { return nn_verify_opening_challenge(pk, s); });
  const std::vector<fe_t> w = weights.get();
  if (!live.empty()) {
    const size_t nz = DEFAULT_COMMITMENT_WIDTH, n = live.size();
    inf.opening_proofs = n;
    std::vector<fe_t> zsum(nz, fe_zero()), s1(2 * n), s2(2 * n);
    std::vector<aff_t> p1(2 * n), p2(2 * n);
    fe_t zd = fe_zero(), c2 = fe_zero(), b2 = fe_zero();
    for (size_t i = 0; i < n; ++i) {
      const NNVerifyState& s = st[live[i]];
      const fe_t rho = w[2 * live[i]], rho2 = w[2 * live[i] + 1];
      zd = fe_add<S>(zd, fe_mul<S>(rho, *s.pv.z_delta));
      p1[2 * i] = s.comm_LZ;
      s1[2 * i] = fe_mul<S>(rho, s.rr);
      p1[2 * i + 1] = *s.pv.delta;
      s1[2 * i + 1] = rho;
      p2[2 * i] = s.comm_eval;
      s2[2 * i] = fe_mul<S>(rho2, s.rr);
      p2[2 * i + 1] = *s.pv.beta;
      s2[2 * i + 1] = rho2;
      c2 = fe_add<S>(c2, fe_mul<S>(rho2, s.ip));
      b2 = fe_add<S>(b2, fe_mul<S>(rho2, *s.pv.z_beta));
    }
    parallel_for(8, (size_t)1 << 20, [&](size_t part) {  // sum_k rho_k z_vec_k, a column range per thread
      for (size_t j = part * nz / 8, e = (part + 1) * nz / 8; j < e; ++j)
        for (size_t i = 0; i < n; ++i) zsum[j] = fe_add<S>(zsum[j], fe_mul<S>(w[2 * live[i]], st[live[i]].pv.z_vec[j]));
    });
    ZJob zj;
    zj.ctx = ctx;
    zj.key = pk.ck;
    ck(sp_msm_ck_begin(ctx, pk.ck, u64p(zsum.data()), nz, &zj.job), "<sum rho z, ck> (begin)");
    aff_t lhs1, lhs2, rhs1, rhs2;
    ck(sp_msm(ctx, u64p(s1.data()), u64p(&p1[0].x), 2 * n, u64p(&lhs1.x)), "sum rho (r comm_LZ + delta)");
    ck(sp_msm(ctx, u64p(s2.data()), u64p(&p2[0].x), 2 * n, u64p(&lhs2.x)), "sum rho' (r comm_eval + beta)");
    ck(sp_hyrax_commit_small(ctx, pk.vc_ck, u64p(&c2), 1, u64p(&b2), u64p(&rhs2.x)), "combined right side of the second equation");
    {
      sp_msm_job* j = zj.job;
      zj.job = nullptr;
      ck(sp_msm_ck_finish(ctx, pk.ck, j, u64p(&zd), u64p(&rhs1.x)), "<sum rho z, ck> (finish)");
    }
    const bool ok = same_point(jac_from_affine(lhs1), jac_from_affine(rhs1)) && same_point(jac_from_affine(lhs2), jac_from_affine(rhs2));
    inf.opening_batched_ok = ok ? 1 : 0;
    if (!ok) {
      for (size_t k : live) codes[k] = nn_verify_opening_check(pk, st[k]);
      inf.fallback_proofs = n;
    }
  }
  if (info) *info = inf;
}

// ---- R1CSShape::is_sat (src/r1cs/mod.rs:358-394) on every instance of a prepared state ---------------------------------------------------------------
// Each step instance against S_step - z_i = [W_i | 1 | X_i] (src/neutronnova_zk.rs:1487-1518), the products through sp_multiply_vec_batched and the row
// check of all steps in one launch (sp_r1cs_residual_batched) - and the core instance against S_core; then `res_comm` (:379) per instance: PCS::commit of
// its shared and its precommitted rows with the stored blinds, compared with comm_shared / comm_pre. reports: the steps, then the core. bad: (instance, row)
// pairs, row counted over the instance's [shared | precommitted] rows. The verifier-circuit and folded instances are host-side and tiny: not checked here.
// Works on tables of its own (freed on return): nothing a later prove reads is written.
static bool nn_is_sat(const NNZkKey& pk, NNZkPrep& ps, sp_sat_report* reports, std::vector<uint64_t>* bad, const char** reason) {
  sp_ctx* ctx = pk.ctx;
  const size_t n = ps.steps.size();
  struct Tabs {
    std::vector<sp_table*> v;
    ~Tabs() {
      for (sp_table* t : v) sp_table_free(t);
    }
    sp_table* zeros(sp_ctx* c, size_t len) {
      sp_table* t = nullptr;
      ck(sp_table_zeros(c, len, (size_t)-1, (size_t)-1, &t), "alloc (is_sat)");
      v.push_back(t);
      return t;
    }
  } tabs;
  auto make_z = [&](const sp_dims& dd, const NNPre& p) {
    const size_t M = dd.num_shared + dd.num_precommitted + dd.num_rest;
    sp_table* z = tabs.zeros(ctx, M + 1 + dd.num_public);
    ck(sp_table_copy(ctx, z, 0, p.W, 0, M), "z <- W");
    std::vector<fe_t> tail(1 + dd.num_public);
    tail[0] = fe_one<S>();
    std::copy(p.publics.begin(), p.publics.end(), tail.begin() + 1);
    ck(sp_table_write(ctx, z, M, u64p(tail.data()), tail.size()), "z tail");
    return z;
  };
  const size_t N = pk.dims.num_cons;
  std::vector<const sp_table*> zs(n), azc(n), bzc(n), czc(n);
  std::vector<sp_table*> az(n), bz(n), cz(n);
  for (size_t i = 0; i < n; ++i) {
    zs[i] = make_z(pk.dims, ps.steps[i]);
    azc[i] = az[i] = tabs.zeros(ctx, N);
    bzc[i] = bz[i] = tabs.zeros(ctx, N);
    czc[i] = cz[i] = tabs.zeros(ctx, N);
  }
  ck(sp_multiply_vec_batched(ctx, pk.S_step, zs.data(), n, az.data(), bz.data(), cz.data()), "multiply_vec_batched (is_sat)");
  ck(sp_r1cs_residual_batched(ctx, azc.data(), bzc.data(), czc.data(), nullptr, nullptr, n, N, reports), "r1cs_residual_batched");
  ck(sp_shape_is_sat(ctx, pk.S_core, make_z(pk.dims_core, ps.core), nullptr, nullptr, &reports[n]), "shape_is_sat (core)");
  bad->clear();
  bool rows_ok = true;
  *reason = nullptr;
  for (size_t i = 0; i <= n; ++i) {
    const sp_dims& dd = i < n ? pk.dims : pk.dims_core;
    const NNPre& p = i < n ? ps.steps[i] : ps.core;
    const size_t rows_sh = ps.comm_shared.size(), rows_pre = p.comm_pre.size();
    std::vector<aff_t> again(rows_sh + rows_pre);
    if (rows_sh) ck(sp_hyrax_commit(ctx, pk.ck, p.W, 0, dd.num_shared, u64p(ps.r_shared.data()), ps.is_small ? 1 : 0, u64p(&again[0].x)), "commit shared (is_sat)");
    if (rows_pre)
      ck(sp_hyrax_commit(ctx, pk.ck, p.W, dd.num_shared, dd.num_precommitted, u64p(p.r_pre.data()), ps.is_small ? 1 : 0, u64p(&again[rows_sh].x)), "commit precommitted (is_sat)");
    for (size_t r = 0; r < rows_sh + rows_pre; ++r) {
      const aff_t& want = r < rows_sh ? ps.comm_shared[r] : p.comm_pre[r - rows_sh];
      if (memcmp(&again[r], &want, sizeof(aff_t)) != 0) {
        bad->push_back(i);
        bad->push_back(r);
        rows_ok = false;
      }
    }
    if (reports[i].num_failing) *reason = "R1CS is unsatisfiable";  // takes precedence (:381-391)
  }
  if (!*reason && !rows_ok) *reason = "Invalid commitment";
  return *reason == nullptr;
}

}  // namespace spartan2

using namespace spartan2;
extern "C" void ss_set_error(const char* msg);
static int catch_all_nn() {
  try {
    throw;
  } catch (const Error& e) {
    ss_set_error(e.what());
    return e.code;
  } catch (const std::exception& e) {
    ss_set_error(e.what());
    return SP_ERR_INTERNAL;
  }
}

extern "C" {
// args: the integer R1CS of the step circuit and of the core circuit (same padded dimensions), as for ss_setup
int nnz_setup(sp_ctx* ctx, size_t num_steps, size_t num_cons, size_t num_shared, size_t num_precommitted, size_t num_rest, size_t num_public, size_t num_challenges,
              const int64_t* Ad, const uint32_t* Ai, const uint64_t* Ap, const int64_t* Bd, const uint32_t* Bi, const uint64_t* Bp, const int64_t* Cd, const uint32_t* Ci,
              const uint64_t* Cp, size_t c_num_cons, size_t c_num_shared, size_t c_num_precommitted, size_t c_num_rest, size_t c_num_public, size_t c_num_challenges,
              const int64_t* cAd, const uint32_t* cAi, const uint64_t* cAp, const int64_t* cBd, const uint32_t* cBi, const uint64_t* cBp, const int64_t* cCd,
              const uint32_t* cCi, const uint64_t* cCp, void** out_pk) {
  try {
    *out_pk = nn_setup(ctx, make_view(num_cons, num_shared, num_precommitted, num_rest, num_public, num_challenges, Ad, Ai, Ap, Bd, Bi, Bp, Cd, Ci, Cp),
                       make_view(c_num_cons, c_num_shared, c_num_precommitted, c_num_rest, c_num_public, c_num_challenges, cAd, cAi, cAp, cBd, cBi, cBp, cCd, cCi, cCp),
                       num_steps);
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
void nnz_pk_free(void* pk) { delete (NNZkKey*)pk; }
// The key's NeutronNovaVerifierKey / NeutronNovaProverKey as bincode bytes (see nn_key_to_bytes): the circuit arguments of nnz_setup again, ss_vk_to_bytes's
// protocol. Two passes: out == NULL returns the length, otherwise the bytes are written (cap must hold them) and the length returned; < 0 = error
// (ss_last_error), among them other circuits than the key's and a key that was itself loaded from bytes ("keep those").
static long nnz_key_to_bytes(const char* who, bool prover, void* pk, const R1CSIntView& Rs, const R1CSIntView& Rc, uint8_t* out, size_t cap) {
  try {
    if (!pk) throw Error(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": null key");
    const NNZkKey& key = *(NNZkKey*)pk;
    nn_refuse_loaded(key, who);
    if (!out) return (long)nn_key_bytes_len(key, Rs, Rc, prover);
    const std::vector<uint8_t> b = nn_key_to_bytes(key, Rs, Rc, prover);
    if (cap < b.size()) throw Error(SP_ERR_INVALID_INPUT_LENGTH, std::string(who) + ": buffer too small");
    memcpy(out, b.data(), b.size());
    return (long)b.size();
  } catch (...) {
    return catch_all_nn();
  }
}
long nnz_vk_to_bytes(void* pk, size_t num_cons, size_t num_shared, size_t num_precommitted, size_t num_rest, size_t num_public, size_t num_challenges, const int64_t* Ad,
                     const uint32_t* Ai, const uint64_t* Ap, const int64_t* Bd, const uint32_t* Bi, const uint64_t* Bp, const int64_t* Cd, const uint32_t* Ci,
                     const uint64_t* Cp, size_t c_num_cons, size_t c_num_shared, size_t c_num_precommitted, size_t c_num_rest, size_t c_num_public,
                     size_t c_num_challenges, const int64_t* cAd, const uint32_t* cAi, const uint64_t* cAp, const int64_t* cBd, const uint32_t* cBi, const uint64_t* cBp,
                     const int64_t* cCd, const uint32_t* cCi, const uint64_t* cCp, uint8_t* out, size_t cap) {
  return nnz_key_to_bytes("nnz_vk_to_bytes", false, pk, make_view(num_cons, num_shared, num_precommitted, num_rest, num_public, num_challenges, Ad, Ai, Ap, Bd, Bi, Bp, Cd, Ci, Cp),
                          make_view(c_num_cons, c_num_shared, c_num_precommitted, c_num_rest, c_num_public, c_num_challenges, cAd, cAi, cAp, cBd, cBi, cBp, cCd, cCi, cCp), out,
                          cap);
}
long nnz_pk_to_bytes(void* pk, size_t num_cons, size_t num_shared, size_t num_precommitted, size_t num_rest, size_t num_public, size_t num_challenges, const int64_t* Ad,
                     const uint32_t* Ai, const uint64_t* Ap, const int64_t* Bd, const uint32_t* Bi, const uint64_t* Bp, const int64_t* Cd, const uint32_t* Ci,
                     const uint64_t* Cp, size_t c_num_cons, size_t c_num_shared, size_t c_num_precommitted, size_t c_num_rest, size_t c_num_public,
                     size_t c_num_challenges, const int64_t* cAd, const uint32_t* cAi, const uint64_t* cAp, const int64_t* cBd, const uint32_t* cBi, const uint64_t* cBp,
                     const int64_t* cCd, const uint32_t* cCi, const uint64_t* cCp, uint8_t* out, size_t cap) {
  return nnz_key_to_bytes("nnz_pk_to_bytes", true, pk, make_view(num_cons, num_shared, num_precommitted, num_rest, num_public, num_challenges, Ad, Ai, Ap, Bd, Bi, Bp, Cd, Ci, Cp),
                          make_view(c_num_cons, c_num_shared, c_num_precommitted, c_num_rest, c_num_public, c_num_challenges, cAd, cAi, cAp, cBd, cBi, cBp, cCd, cCi, cCp), out,
                          cap);
}
// A verifier's key from the bytes nnz_vk_to_bytes writes (see nn_key_from_bytes): no circuit, no setup. The key does not hold the step count (the reference
// fixes num_rounds_b alone), so the caller states it. flags: 0, or SP_SHAPE_WIRE_DEVICE / SP_SHAPE_WIRE_HOST to force a decode form, and SP_SHAPE_WIRE_TIMED.
// The verify family, nnz_pk_info, nnz_proof_words and nnz_proof_to_bytes / _from_bytes take the key; every prover entry point refuses it ("verifier-only
// key"); nnz_pk_free ends it.
int nnz_verifier_from_bytes(sp_ctx* ctx, const uint8_t* bytes, size_t n, size_t num_steps, unsigned flags, void** out_vk) {
  try {
    if (!out_vk) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "nnz_verifier_from_bytes: null out");
    *out_vk = nullptr;
    *out_vk = nn_key_from_bytes(ctx, bytes, n, num_steps, flags, false);
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
// A prover's key from the bytes nnz_pk_to_bytes writes. flags: SP_SHAPE_WIRE_FULL_DEVICE / SP_SHAPE_WIRE_FULL force the device / host form of the two full
// shapes (neither: nnz_prover_full_device_default), SP_SHAPE_WIRE_TIMED, SS_PK_TRUST_DIGEST (1 << 16) takes the stored digest unhashed. Every entry point
// takes the key as it takes nnz_setup's, except nnz_vk_to_bytes / nnz_pk_to_bytes.
int nnz_prover_from_bytes(sp_ctx* ctx, const uint8_t* bytes, size_t n, size_t num_steps, unsigned flags, void** out_pk) {
  try {
    if (!out_pk) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "nnz_prover_from_bytes: null out");
    *out_pk = nullptr;
    *out_pk = nn_key_from_bytes(ctx, bytes, n, num_steps, flags, true);
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
// ms of the calling thread's last nnz_verifier_from_bytes / nnz_prover_from_bytes: ck (and vk_ee) read, S_step, S_core, the verifier-circuit shapes compared
// and vc_ck read, the two sp_ck_create, the digest (helper thread; 0 when trusted), the wait for it behind the rest, the whole call
// The verifier key's digest from key bytes alone (nn_vk_digest_from_bytes; host code, no context): prover != 0 = the bytes are a prover's key, whose stored
// digest is stepped over. No element is converted or checked - a key that fails its load never shows its digest.
int nnz_vk_digest_from_bytes(const uint8_t* bytes, size_t n, int prover, uint8_t out[32]) {
  try {
    if (!bytes || !n || !out) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "nnz_vk_digest_from_bytes: null argument");
    nn_vk_digest_from_bytes(bytes, n, prover != 0, out);
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
void nnz_key_stages(double out[8]) { memcpy(out, g_nn_key_stage_ms, sizeof g_nn_key_stage_ms); }
int nnz_verifier_device_default(void) { return NN_VK_DEVICE_DEFAULT ? 1 : 0; }
int nnz_prover_full_device_default(void) { return NN_PK_FULL_DEVICE_DEFAULT ? 1 : 0; }
// the key's shapes, for sp_shape_compare / sp_shape_info (which: 0 = S_step, 1 = S_core); the key keeps owning them
const sp_shape* nnz_pk_shape(void* pk, int which) { return pk ? (which ? ((NNZkKey*)pk)->S_core : ((NNZkKey*)pk)->S_step) : nullptr; }
// out: the ten dimensions of S_step, then of S_core, then num_steps, 1 / 0 = verifier-only, 1 / 0 = loaded from bytes
void nnz_pk_dims(void* pk_, uint64_t out[23]) {
  auto* pk = (NNZkKey*)pk_;
  memcpy(out, &pk->dims, sizeof(sp_dims));
  memcpy(out + 10, &pk->dims_core, sizeof(sp_dims));
  out[20] = pk->num_steps, out[21] = pk->verifier_only, out[22] = pk->from_bytes;
}
// out: nb, nx, ny, vc rounds, vc total vars, vc num_cons, vc num_cons_unpadded, vc num_public; digest = the vk digest (SHA-256 over NeutronNovaVerifierKey::write_bytes)
void nnz_pk_info(void* pk_, uint64_t out[8], uint8_t digest[32]) {
  auto* pk = (NNZkKey*)pk_;
  uint64_t v[8] = {pk->nb, pk->nx, pk->ny, pk->vc.num_rounds, pk->vc.total_vars, pk->vc.num_cons, pk->vc.num_cons_unpadded, pk->vc.num_public};
  memcpy(out, v, sizeof v);
  memcpy(digest, pk->vk_digest, 32);
}
size_t nnz_proof_words(void* pk_) { return ((NNZkKey*)pk_)->layout.words(); }
// prep_prove with the step / core witnesses generated on the device (see nn_prep_prove_sha256): blocks = n x 64 bytes
int nnz_prep_prove_sha256(void* pk, const sp_sha256_plan* plan, const uint8_t* blocks, size_t n, int is_small, const uint8_t* tape, size_t tape_blocks, size_t* tape_used,
                          void** out_ps) {
  try {
    Tape t{tape, tape_blocks};
    *out_ps = nn_prep_prove_sha256(nn_prover_key(pk, "nnz_prep_prove_sha256"), plan, blocks, n, is_small != 0, t);
    if (tape_used) *tape_used = t.pos;
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
int nnz_prep_prove(void* pk, size_t n, const uint64_t* step_wit, size_t wit_len, const uint64_t* step_pub, size_t npub, const uint64_t* core_wit, const uint64_t* core_pub,
                   int is_small, const uint8_t* tape, size_t tape_blocks, size_t* tape_used, void** out_ps) {
  try {
    Tape t{tape, tape_blocks};
    *out_ps = nn_prep_prove(nn_prover_key(pk, "nnz_prep_prove"), n, step_wit, wit_len, step_pub, npub, core_wit, core_pub, is_small != 0, t);
    if (tape_used) *tape_used = t.pos;
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
// prep_prove for `count` states of one key in one pass (nn_prep_prove_batch_from): per state k its step count n[k] (the key's), step_wit[k] = n[k] x wit_len[k]
// words, step_pub[k] = n[k] x npub, core_wit[k], core_pub[k], tapes[k] / tape_blocks[k]; tape_used[k] = the blocks it consumed, out_ps[k] = its state - the
// state nnz_prep_prove makes of the same input and tape, to be proved, checked and freed on its own. phase_ms (8, optional): blinds + allocations, witnesses,
// commitments, layers, mirrors, synchronise, total. flags: NNZ_PREP_PER_STATE_COMMIT (1) = one sp_hyrax_commit per polynomial, NNZ_PREP_PER_STATE_LAYERS (2)
// = nifs_prepare per state, NNZ_PREP_SHARED_COMMIT (4) / NNZ_PREP_SHARED_LAYERS (8) = the shared stage whatever the driver's default. count == 0 and null arguments are refused before a context is touched; a wrong step count or witness length is
// InvalidWitnessLength naming the state ("prep_prove_batch: state 2: ..."), as is a short tape; on any failure every state made so far is freed and out_ps
// is not written.
static std::vector<Tape> nnz_batch_tapes(size_t count, const uint8_t* const* tapes, const size_t* tape_blocks) {
  std::vector<Tape> ts;
  for (size_t k = 0; k < count; ++k) {
    if (!tapes[k]) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: state " + std::to_string(k) + ": null tape");
    ts.push_back(Tape{tapes[k], tape_blocks[k]});
  }
  return ts;
}
static void nnz_batch_out(const std::vector<NNZkPrep*>& st, const std::vector<Tape>& ts, size_t* tape_used, void** out_ps) {
  for (size_t k = 0; k < st.size(); ++k) {
    out_ps[k] = st[k];
    if (tape_used) tape_used[k] = ts[k].pos;
  }
}
int nnz_prep_prove_batch_opts(void* pk, size_t count, const size_t* n, const uint64_t* const* step_wit, const size_t* wit_len, const uint64_t* const* step_pub, size_t npub,
                              const uint64_t* const* core_wit, const uint64_t* const* core_pub, int is_small, const uint8_t* const* tapes, const size_t* tape_blocks,
                              size_t* tape_used, void** out_ps, double* phase_ms, unsigned flags) {
  try {
    if (count == 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: count must be at least 1");
    if (!pk || !n || !step_wit || !wit_len || !step_pub || !core_wit || !core_pub || !tapes || !tape_blocks || !out_ps)
      throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: null argument");
    std::vector<Tape> ts = nnz_batch_tapes(count, tapes, tape_blocks);
    nnz_batch_out(nn_prep_prove_batch(nn_prover_key(pk, "nnz_prep_prove_batch"), count, n, step_wit, wit_len, step_pub, npub, core_wit, core_pub, is_small != 0, ts.data(), flags, phase_ms), ts, tape_used,
                  out_ps);
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
int nnz_prep_prove_batch(void* pk, size_t count, const size_t* n, const uint64_t* const* step_wit, const size_t* wit_len, const uint64_t* const* step_pub, size_t npub,
                         const uint64_t* const* core_wit, const uint64_t* const* core_pub, int is_small, const uint8_t* const* tapes, const size_t* tape_blocks, size_t* tape_used,
                         void** out_ps, double* phase_ms) {
  return nnz_prep_prove_batch_opts(pk, count, n, step_wit, wit_len, step_pub, npub, core_wit, core_pub, is_small, tapes, tape_blocks, tape_used, out_ps, phase_ms, 0);
}
// the same with the witnesses generated on the device in ONE launch (see nn_prep_prove_sha256_batch): blocks[k] = n[k] x 64 bytes
int nnz_prep_prove_sha256_batch_opts(void* pk, const sp_sha256_plan* plan, size_t count, const uint8_t* const* blocks, const size_t* n, int is_small, const uint8_t* const* tapes,
                                     const size_t* tape_blocks, size_t* tape_used, void** out_ps, double* phase_ms, unsigned flags) {
  try {
    if (count == 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: count must be at least 1");
    if (!pk || !plan || !blocks || !n || !tapes || !tape_blocks || !out_ps) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prep_prove_batch: null argument");
    std::vector<Tape> ts = nnz_batch_tapes(count, tapes, tape_blocks);
    nnz_batch_out(nn_prep_prove_sha256_batch(nn_prover_key(pk, "nnz_prep_prove_sha256_batch"), plan, count, blocks, n, is_small != 0, ts.data(), flags, phase_ms), ts, tape_used, out_ps);
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
int nnz_prep_prove_sha256_batch(void* pk, const sp_sha256_plan* plan, size_t count, const uint8_t* const* blocks, const size_t* n, int is_small, const uint8_t* const* tapes,
                                const size_t* tape_blocks, size_t* tape_used, void** out_ps, double* phase_ms) {
  return nnz_prep_prove_sha256_batch_opts(pk, plan, count, blocks, n, is_small, tapes, tape_blocks, tape_used, out_ps, phase_ms, 0);
}
void nnz_prep_free(void* ps) { delete (NNZkPrep*)ps; }
// is_sat of the step instances and the core instance of a prepared state (nn_is_sat): reports = num_steps + 1 entries, the steps, then the core; bad_rows =
// (instance, row) pairs of commitment rows that do not match, at most bad_rows_cap pairs of the *n_bad_rows found. 0 = every instance satisfied and committed
// to; SP_ERR_UNSAT with ss_last_error() = "R1CS is unsatisfiable" (takes precedence) or "Invalid commitment"; another negative value = library error.
int nnz_prep_is_sat(void* pk, void* ps, sp_sat_report* reports, uint64_t* bad_rows, size_t bad_rows_cap, size_t* n_bad_rows) {
  try {
    if (!ps || !reports) throw Error(SP_ERR_INTERNAL, "is_sat before prep_prove");
    std::vector<uint64_t> bad;
    const char* reason = nullptr;
    const bool ok = nn_is_sat(nn_prover_key(pk, "nnz_prep_is_sat"), *(NNZkPrep*)ps, reports, &bad, &reason);
    if (n_bad_rows) *n_bad_rows = bad.size() / 2;
    if (bad_rows) std::copy(bad.begin(), bad.begin() + 2 * std::min(bad.size() / 2, bad_rows_cap), bad_rows);
    if (ok) return 0;
    ss_set_error(reason);
    return SP_ERR_UNSAT;
  } catch (...) {
    return catch_all_nn();
  }
}
// 0 = accept, 1..6 = the failed check (nn_verify above), < 0 = error
int nnz_verify(void* pk, const uint64_t* words, size_t nwords) {
  try {
    return nn_verify(*(NNZkKey*)pk, words, nwords);
  } catch (...) {
    return catch_all_nn();
  }
}
// phase_ms[8]: instances, nifs, outer, inner, verifier-circuit instance, opening, total, (of which) per-round vc commitments
static int nnz_prove_impl(void* pk, void* ps, const uint8_t* tape, size_t tape_blocks, size_t* tape_used, uint64_t* out_words, size_t out_cap, double* phase_ms,
                          bool reference_order) {
  try {
    Tape t{tape, tape_blocks};
    ProofBuf pf = nn_prove(nn_prover_key(pk, reference_order ? "nnz_prove_reference_order" : "nnz_prove"), *(NNZkPrep*)ps, t, phase_ms, reference_order);
    if (pf.words.size() > out_cap) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "proof buffer too small");
    memcpy(out_words, pf.words.data(), pf.words.size() * 8);
    if (tape_used) *tape_used = t.pos;
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
int nnz_prove(void* pk, void* ps, const uint8_t* tape, size_t tape_blocks, size_t* tape_used, uint64_t* out_words, size_t out_cap, double* phase_ms) {
  return nnz_prove_impl(pk, ps, tape, tape_blocks, tape_used, out_words, out_cap, phase_ms, false);
}
// the reference-order driver (see nn_prove): the time of an unchanged neutronnova_zk.rs over the ABI; the proof is the same
int nnz_prove_reference_order(void* pk, void* ps, const uint8_t* tape, size_t tape_blocks, size_t* tape_used, uint64_t* out_words, size_t out_cap, double* phase_ms) {
  return nnz_prove_impl(pk, ps, tape, tape_blocks, tape_used, out_words, out_cap, phase_ms, true);
}
// prove for `count` distinct prepared states of one key (nn_prove_batch): per proof k its state ps[k], tapes[k] / tape_blocks[k], out_words[k] = a buffer of
// out_cap words; tape_used[k] = the blocks it consumed. Proof k and its tape use are those of nnz_prove(pk, ps[k], tapes[k], ..). flags: NNZ_BATCH_PER_PROOF (1)
// = a loop of nn_prove, NNZ_BATCH_LOCKSTEP (2) = the two batched sum-checks of all proofs in lockstep, 0 = the driver's default (NN_PROVE_BATCH_LOCKSTEP_MIN).
// phase_ms (10, optional): setup .. NIFS, outer before / sum-check / after, inner before / sum-check / after, verifier-circuit instance .. emit, total,
// 1.0 when the lockstep form ran (the per-proof form fills the total only). count == 0 and null arguments are refused before a context is touched; the same
// state twice is refused; a failure names the proof ("prove_batch: proof 2: random tape exhausted"), writes no output and leaves every state usable.
int nnz_prove_batch_opts(void* pk, void* const* ps, size_t count, const uint8_t* const* tapes, const size_t* tape_blocks, size_t* tape_used, uint64_t* const* out_words,
                         size_t out_cap, double* phase_ms, unsigned flags) {
  try {
    if (count == 0) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: count must be at least 1");
    if (!pk || !ps || !tapes || !tape_blocks || !out_words) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: null argument");
    std::vector<Tape> ts;
    for (size_t k = 0; k < count; ++k) {
      if (!tapes[k] || !out_words[k]) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "prove_batch: proof " + std::to_string(k) + ": null tape or output");
      ts.push_back(Tape{tapes[k], tape_blocks[k]});
    }
    const NNZkKey& key = nn_prover_key(pk, "nnz_prove_batch");
    if (key.layout.words() > out_cap) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "proof buffer too small");
    NNBatchPhases ph;
    std::vector<ProofBuf> pf = nn_prove_batch(key, (NNZkPrep* const*)ps, ts.data(), count, flags, &ph);
    for (size_t k = 0; k < count; ++k) {
      memcpy(out_words[k], pf[k].words.data(), pf[k].words.size() * 8);
      if (tape_used) tape_used[k] = ts[k].pos;
    }
    if (phase_ms) {
      const double v[10] = {ph.head, ph.outer_before, ph.outer_sc, ph.outer_after, ph.inner_before, ph.inner_sc, ph.inner_after, ph.tail, ph.total, ph.lockstep};
      memcpy(phase_ms, v, sizeof v);
    }
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
int nnz_prove_batch(void* pk, void* const* ps, size_t count, const uint8_t* const* tapes, const size_t* tape_blocks, size_t* tape_used, uint64_t* const* out_words,
                    size_t out_cap, double* phase_ms) {
  return nnz_prove_batch_opts(pk, ps, count, tapes, tape_blocks, tape_used, out_words, out_cap, phase_ms, 0);
}
// NeutronNovaZkSNARK as bincode bytes (the reference's serde framing; include/spartan_hip.h "wire formats"). `_to_bytes`: out may be NULL to learn *len.
int nnz_proof_to_bytes(void* pk, const uint64_t* words, size_t nwords, uint8_t* out, size_t cap, size_t* len) {
  try {
    std::vector<uint8_t> b = ((NNZkKey*)pk)->layout.to_bytes(words, nwords);
    *len = b.size();
    if (out) {
      if (cap < b.size()) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "byte buffer too small");
      memcpy(out, b.data(), b.size());
    }
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
int nnz_proof_from_bytes(void* pk, const uint8_t* bytes, size_t n, uint64_t* out_words, size_t cap_words) {
  try {
    std::vector<uint64_t> w = ((NNZkKey*)pk)->layout.from_bytes(bytes, n);
    if (cap_words < w.size()) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "word buffer too small");
    memcpy(out_words, w.data(), 8 * w.size());
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
// verify on the serialised proof: 0 = accept, 1..6 = the failed check (a proof that does not decode fails check 1), < 0 = error
int nnz_verify_bytes(void* pk, const uint8_t* bytes, size_t n) {
  try {
    std::vector<uint64_t> w;
    try {
      w = ((NNZkKey*)pk)->layout.from_bytes(bytes, n);
    } catch (const Error& e) {
      if (e.code != SP_ERR_INVALID_INPUT_LENGTH) throw;
      ss_set_error(e.what());
      return 1;
    }
    return nn_verify(*(NNZkKey*)pk, w.data(), w.size());
  } catch (...) {
    return catch_all_nn();
  }
}
// verify_batch (see nn_verify_batch): `count` proofs of this key, codes[k] = what nnz_verify returns for proof k (0 accept, 1, 2, 4, 5, 6). seed: 32 bytes mixed
// into the weights of the combined opening check, or NULL. info may be NULL. flags: 0 = the form the batch size calls for, NNZ_VERIFY_BATCH_PER_PROOF (1) =
// one nnz_verify after the other, NNZ_VERIFY_BATCH_SHARED (2) = the shared stage and the combined opening from two proofs on. Returns 0, or < 0 = library
// error (the codes are then meaningless); count != 0 with a null array is refused.
int nnz_verify_batch_opts(void* pk, const uint64_t* const* words, const size_t* nwords, size_t count, const uint8_t* seed, int* codes, ss_verify_batch_info* info,
                          unsigned flags) {
  try {
    if (!pk || (count && (!words || !nwords || !codes))) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "nnz_verify_batch: null argument");
    nn_verify_batch(*(NNZkKey*)pk, words, nwords, count, seed, codes, info, flags);
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
int nnz_verify_batch(void* pk, const uint64_t* const* words, const size_t* nwords, size_t count, const uint8_t* seed, int* codes, ss_verify_batch_info* info) {
  return nnz_verify_batch_opts(pk, words, nwords, count, seed, codes, info, 0);
}
// the same over serialised proofs: bytes that do not decode to a proof of this key get code 1, as in nnz_verify_bytes
int nnz_verify_bytes_batch_opts(void* pk_, const uint8_t* const* bytes, const size_t* nbytes, size_t count, const uint8_t* seed, int* codes, ss_verify_batch_info* info,
                                unsigned flags) {
  try {
    if (!pk_ || (count && (!bytes || !nbytes || !codes))) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "nnz_verify_bytes_batch: null argument");
    auto* pk = (NNZkKey*)pk_;
    std::vector<std::vector<uint64_t>> store(count);
    std::vector<const uint64_t*> words(count);
    std::vector<size_t> nwords(count);
    for (size_t k = 0; k < count; ++k) {
      try {
        store[k] = pk->layout.from_bytes(bytes[k], nbytes[k]);
      } catch (const Error& e) {
        if (e.code != SP_ERR_INVALID_INPUT_LENGTH) throw;
        store[k].clear();  // no words, which fails the length check of the parse with code 1
      }
      words[k] = store[k].data();
      nwords[k] = store[k].size();
    }
    nn_verify_batch(*pk, words.data(), nwords.data(), count, seed, codes, info, flags);
    return 0;
  } catch (...) {
    return catch_all_nn();
  }
}
int nnz_verify_bytes_batch(void* pk, const uint8_t* const* bytes, const size_t* nbytes, size_t count, const uint8_t* seed, int* codes, ss_verify_batch_info* info) {
  return nnz_verify_bytes_batch_opts(pk, bytes, nbytes, count, seed, codes, info, 0);
}
}
