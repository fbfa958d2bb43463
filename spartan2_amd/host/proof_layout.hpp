// The flat word layout of a proof (the parity contract) stated once per proof type: SpartanLayout and NNLayout are plain values
// computed from the padded dimensions, and the word count, the bincode image in both directions, the named view a verifier reads and the encoding checks
// of an untrusted proof all derive from them. Pure host code, no device call.
#pragma once
#include "snark_common.hpp"
#include "verifier_circuit.hpp"

namespace spartan2 {

// what both layouts' visit() feeds with every point and every scalar of a proof: an untrusted proof must hold canonical residues (the reference's
// deserialisation rejects anything >= the modulus) and points on the curve
struct EncodingCheck {
  bool ok = true;
  void points(const aff_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
      if (!limbs_canonical<B>(p[i].x) || !limbs_canonical<B>(p[i].y) || !aff_on_curve(p[i])) ok = false;
  }
  void scalars(const fe_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
      if (!limbs_canonical<S>(p[i])) ok = false;
  }
};
template <class Layout>
inline bool well_formed(const Layout& L, const uint64_t* words) {
  EncodingCheck c;
  L.visit(words, c);
  return c.ok;
}

// ---- SpartanSNARK (src/spartan.rs:125-137) -------------------------------------------------------------------------------------------------------
struct SpartanProofView {
  const aff_t *comm_W, *delta, *beta;
  const fe_t *publics, *challenges, *outer, *claims, *inner, *eval_W, *blind_eval_W, *z_vec, *z_delta, *z_beta;
};
struct SpartanLayout {
  size_t rows_shared = 0, rows_precommitted = 0, rows_rest = 0, rounds_x = 0, rounds_y = 0, z_len = 0, num_public = 0, num_challenges = 0;
  SpartanLayout() = default;
  SpartanLayout(const sp_dims& d, size_t num_vars) {
    const size_t W = DEFAULT_COMMITMENT_WIDTH;
    rows_shared = d.num_shared_unpadded ? (d.num_shared + W - 1) / W : 0;  // a segment without variables has no commitment (Option: None)
    rows_precommitted = d.num_precommitted_unpadded ? (d.num_precommitted + W - 1) / W : 0;
    rows_rest = (d.num_rest + W - 1) / W;
    rounds_x = log2_ceil(d.num_cons);
    rounds_y = log2_ceil(num_vars) + 1;
    z_len = std::min(num_vars, W);
    num_public = d.num_public;
    num_challenges = d.num_challenges;
  }
  size_t rows() const { return rows_shared + rows_precommitted + rows_rest; }
  sp_spartan_layout wire() const { return sp_spartan_layout{rows_shared, rows_precommitted, rows_rest, num_public, num_challenges, rounds_x, rounds_y, z_len}; }
  size_t words() const {
    const sp_spartan_layout L = wire();
    return sp_proof_words(&L);
  }
  SpartanProofView view(const uint64_t* words) const {
    SpartanProofView v;
    v.comm_W = reinterpret_cast<const aff_t*>(words);
    v.publics = reinterpret_cast<const fe_t*>(v.comm_W + rows());
    v.challenges = v.publics + num_public;
    v.outer = v.challenges + num_challenges;
    v.claims = v.outer + 3 * rounds_x;
    v.inner = v.claims + 3;
    v.eval_W = v.inner + 2 * rounds_y;
    v.blind_eval_W = v.eval_W + 1;
    v.delta = reinterpret_cast<const aff_t*>(v.blind_eval_W + 1);
    v.beta = v.delta + 1;
    v.z_vec = reinterpret_cast<const fe_t*>(v.beta + 1);
    v.z_delta = v.z_vec + z_len;
    v.z_beta = v.z_delta + 1;
    return v;
  }
  template <class V>
  void visit(const uint64_t* words, V& on) const {
    const SpartanProofView v = view(words);
    on.points(v.comm_W, rows());
    on.scalars(v.publics, reinterpret_cast<const fe_t*>(v.delta) - v.publics);
    on.points(v.delta, 2);
    on.scalars(v.z_vec, z_len + 2);
  }
};

// ---- NeutronNovaZkSNARK (src/neutronnova_zk.rs:1373-1385; oracle NNProof::serialize) ------------------------------------------------------------------
// { comm_W_shared: Option, step_instances: Vec<SplitR1CSInstance>, core_instance, eval_arg, U_verifier: SplitMultiRoundR1CSInstance, nifs: NovaNIFS
// { comm_T }, random_U: RelaxedR1CSInstance { comm_W, comm_E, X, u }, relaxed_snark }. The instances carry comm_W_shared = None (:2069-2078) and no challenges.
struct NNProofView {
  struct Inst {
    const aff_t *pre, *rest;
    const fe_t* pub;
  };
  const aff_t* comm_shared;
  std::vector<Inst> steps;
  Inst core;
  const aff_t *delta, *beta;
  const fe_t *z_vec, *z_delta, *z_beta;
  std::vector<const aff_t*> vcomm;  // the verifier-circuit instance's rows per round (consecutive in the layout)
  const fe_t* vpub;
  std::vector<const fe_t*> vchal;
  const aff_t *comm_T, *rnd_comm_W, *rnd_comm_E;
  const fe_t *rnd_u, *rnd_X, *v_outer, *v_claims, *v_inner, *v_W, *blind_vW, *v_E, *blind_vE;
};
struct NNLayout {
  // rows of the 2048-wide key: the shared segment is one commitment for every circuit; step and core may split the remaining rows into
  // precommitted | rest differently (SplitR1CSShape::equalize only makes their sums equal)
  size_t rows_sh = 0, rows_pre = 0, rows_rest = 0, rows_pre_c = 0, rows_rest_c = 0, num_steps = 0, step_public = 0, core_public = 0;
  // the verifier circuit: per round the rows of the width-`vw` key and the challenges; public values, constraint rows, all rows, all of X, sum-check rounds
  std::vector<size_t> vrows, vchals;
  size_t vw = 0, vpublic = 0, vcons_rows = 0, vrows_all = 0, vio = 0, vlx = 0, vly = 0;
  NNLayout() = default;
  NNLayout(const sp_dims& step, const sp_dims& core, size_t num_steps_, const vcirc::Shape& vs) {
    const size_t CW = DEFAULT_COMMITMENT_WIDTH;
    rows_sh = step.num_shared_unpadded ? step.num_shared / CW : 0;
    rows_pre = step.num_precommitted_unpadded ? step.num_precommitted / CW : 0;
    rows_rest = step.num_rest / CW;
    rows_pre_c = core.num_precommitted_unpadded ? core.num_precommitted / CW : 0;
    rows_rest_c = core.num_rest / CW;
    if (rows_pre_c + rows_rest_c != rows_pre + rows_rest) throw Error(SP_ERR_INTERNAL, "NeutronNova: step and core rows differ after equalize");
    num_steps = num_steps_;
    step_public = step.num_public;
    core_public = core.num_public;
    vw = vs.width;
    for (size_t r = 0; r < vs.num_rounds; ++r) vrows.push_back(vs.vars_padded[r] / vw), vchals.push_back(vs.chals_per_round[r]);
    vpublic = vs.num_public;
    vcons_rows = vs.num_cons / vw;
    vrows_all = vs.total_vars / vw;
    vio = vs.num_io();
    vlx = log2_ceil(vs.num_cons);
    vly = log2_ceil(next_pow2(vs.total_vars)) + 1;
    Measure m;
    fe_count_ = walk(m);
    wire_len_ = m.bytes;
  }
  size_t rows() const { return rows_sh + rows_pre + rows_rest; }
  size_t words() const { return 4 * fe_count_; }
  size_t wire_len() const { return wire_len_; }

  // THE statement of the layout: the fields in wire order, each with its offset `o` (in field elements) in the flat words. A visitor sees
  //   tag(v)                       an Option tag                                  1 byte
  //   len(v, min_elem_bytes)       a Vec length whose elements follow as fields   8 bytes; min_elem_bytes = the smallest encoding of one element
  //   points(o, n, with_len)       n points (a HyraxCommitment when with_len)     96 bytes each (+ 8)
  //   scalars(o, n, with_len)      n scalars (a Vec<Scalar> when with_len)        32 bytes each (+ 8)
  //   at(&NNProofView::f, o)       the field (or the next entry of the list) `f` of the view starts at o
  //   instance(i, pre, rest, pub)  where step instance i (i == num_steps: the core) has its rows and public values
  // Flat order is wire order except random_U, whose `u` precedes `X` in the flat words and follows it on the wire (src/r1cs/mod.rs:213-218).
  template <class V>
  size_t walk(V& v) const {
    typedef NNProofView P;
    size_t o = 0;
    auto points = [&](size_t n, bool with_len) {
      v.points(o, n, with_len);
      o += 2 * n;
      return o - 2 * n;
    };
    auto scalars = [&](size_t n, bool with_len) {
      v.scalars(o, n, with_len);
      o += n;
      return o - n;
    };
    auto option_commitment = [&](size_t rows) {  // Some exactly when the segment has rows
      v.tag(rows ? 1 : 0);
      return points(rows, rows != 0);
    };
    auto instance = [&](size_t i, size_t npub, size_t my_pre, size_t my_rest) {  // SplitR1CSInstance (src/r1cs/mod.rs:797-806)
      v.tag(0);  // comm_W_shared: None
      const size_t pre = option_commitment(my_pre), rest = points(my_rest, true), pub = scalars(npub, true);
      v.len(0, 32);  // challenges: an empty Vec
      v.instance(i, pre, rest, pub);
    };
    auto sumcheck = [&](size_t rounds, size_t per) {  // Vec<CompressedUniPoly { coeffs_except_linear_term: Vec<Scalar> }>
      const size_t first = o;
      v.len(rounds, 8 + 32 * per);
      for (size_t i = 0; i < rounds; ++i) scalars(per, true);
      return first;
    };
    v.at(&P::comm_shared, option_commitment(rows_sh));
    v.len(num_steps, 1 + 1 + 8 + 8 + 8);  // an instance is at least two Option tags and three Vec lengths
    for (size_t i = 0; i < num_steps; ++i) instance(i, step_public, rows_pre, rows_rest);
    instance(num_steps, core_public, rows_pre_c, rows_rest_c);
    v.at(&P::delta, points(1, false));  // eval_arg: InnerProductArgumentLinear { delta, beta, z_vec, z_delta, z_beta } (src/provider/pcs/ipa.rs:103-114)
    v.at(&P::beta, points(1, false));
    v.at(&P::z_vec, scalars(DEFAULT_COMMITMENT_WIDTH, true));
    v.at(&P::z_delta, scalars(1, false));
    v.at(&P::z_beta, scalars(1, false));
    v.len(vrows.size(), 8);  // U_verifier.comm_w_per_round
    for (size_t r : vrows) v.at(&P::vcomm, points(r, true));
    v.at(&P::vpub, scalars(vpublic, true));
    v.len(vchals.size(), 8);  // challenges_per_round
    for (size_t c : vchals) v.at(&P::vchal, scalars(c, true));
    v.at(&P::comm_T, points(vcons_rows, true));      // nifs.comm_T
    v.at(&P::rnd_comm_W, points(vrows_all, true));   // random_U.comm_W
    v.at(&P::rnd_comm_E, points(vcons_rows, true));  // random_U.comm_E
    v.at(&P::rnd_u, o++);  // random_U.u: before X in the flat words, after it on the wire
    v.at(&P::rnd_X, scalars(vio, true));
    v.scalars(o - vio - 1, 1, false);
    v.at(&P::v_outer, sumcheck(vlx, 3));  // relaxed_snark (src/spartan_relaxed.rs:80-96)
    v.at(&P::v_claims, scalars(3, false));
    v.at(&P::v_inner, sumcheck(vly, 2));
    v.at(&P::v_W, scalars(vw, true));
    v.at(&P::blind_vW, scalars(1, false));
    v.at(&P::v_E, scalars(vw, true));
    v.at(&P::blind_vE, scalars(1, false));
    return o;  // field elements in the flat words
  }

  struct Silent {  // a visitor that ignores what it is shown; the others override what they need
    void tag(uint8_t) {}
    void len(size_t, size_t) {}
    void points(size_t, size_t, bool) {}
    void scalars(size_t, size_t, bool) {}
    template <class F>
    void at(F, size_t) {}
    void instance(size_t, size_t, size_t, size_t) {}
  };
  struct Namer : Silent {  // the visitor behind view(): the offsets of the named fields become pointers into a proof's words
    const fe_t* w;
    size_t num_steps;
    NNProofView p;
    template <class T>
    void at(const T* NNProofView::*f, size_t o) { p.*f = reinterpret_cast<const T*>(w + o); }
    template <class T>
    void at(std::vector<const T*> NNProofView::*f, size_t o) { (p.*f).push_back(reinterpret_cast<const T*>(w + o)); }
    void instance(size_t i, size_t pre, size_t rest, size_t pub) {
      (i < num_steps ? p.steps.emplace_back() : p.core) = {reinterpret_cast<const aff_t*>(w + pre), reinterpret_cast<const aff_t*>(w + rest), w + pub};
    }
  };
  // the named fields of a proof of words() words
  NNProofView view(const uint64_t* words) const {
    Namer namer{{}, reinterpret_cast<const fe_t*>(words), num_steps, {}};
    walk(namer);
    return namer.p;
  }
  template <class V>
  void visit(const uint64_t* words, V& on) const {
    struct Each : Silent {
      const fe_t* w;
      V& on;
      void points(size_t o, size_t n, bool) { on.points(reinterpret_cast<const aff_t*>(w + o), n); }
      void scalars(size_t o, size_t n, bool) { on.scalars(w + o, n); }
    } each{{}, reinterpret_cast<const fe_t*>(words), on};
    walk(each);
  }
  // flat words -> bincode bytes
  std::vector<uint8_t> to_bytes(const uint64_t* words, size_t nwords) const {
    if (nwords != this->words()) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "NNLayout::to_bytes: the word count does not match the key");
    struct Sink : Silent {
      sp_wire* w = nullptr;
      const uint64_t* words;
      ~Sink() { sp_wire_free(w); }
      void tag(uint8_t t) { ck(sp_wire_u8(w, t), "wire"); }
      void len(uint64_t n, size_t) { ck(sp_wire_u64s(w, &n, 1, 0), "wire"); }
      void points(size_t o, size_t n, bool with_len) { ck(sp_wire_points(w, words + 4 * o, n, with_len), "wire"); }
      void scalars(size_t o, size_t n, bool with_len) { ck(sp_wire_scalars(w, words + 4 * o, n, with_len), "wire"); }
    } sink;
    sink.words = words;
    ck(sp_wire_new(0, &sink.w), "wire sink");
    walk(sink);
    std::vector<uint8_t> out(sp_wire_len(sink.w));
    ck(sp_wire_bytes(sink.w, out.data(), out.size()), "wire bytes");
    return out;
  }
  // the inverse; every tag and length prefix must be the one the key's shape dictates (the flat layout has no room for anything else)
  std::vector<uint64_t> from_bytes(const uint8_t* bytes, size_t n) const {
    struct Src : Silent {
      sp_unwire* r = nullptr;
      uint64_t* out;
      ~Src() { sp_unwire_free(r); }
      void tag(uint8_t want) {
        uint8_t t;
        ck(sp_unwire_u8(r, &t), "wire tag");
        if (t != want) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "wire: an Option tag does not match the key's shape");
      }
      void len(size_t want, size_t min_elem_bytes) {  // a prefix larger than the input can hold is refused here, before anything is read
        size_t got;
        ck(sp_unwire_len(r, min_elem_bytes, &got), "wire length");
        if (got != want) throw Error(SP_ERR_INVALID_INPUT_LENGTH, "wire: a length prefix does not match the key's shape");
      }
      void points(size_t o, size_t cnt, bool with_len) {
        if (with_len) len(cnt, 96);
        ck(sp_unwire_points(r, cnt, out + 4 * o), "wire points");
      }
      void scalars(size_t o, size_t cnt, bool with_len) {
        if (with_len) len(cnt, 32);
        ck(sp_unwire_scalars(r, cnt, out + 4 * o), "wire scalars");
      }
    } src;
    ck(sp_unwire_new(bytes, n, &src.r), "wire source");
    std::vector<uint64_t> out(words());
    src.out = out.data();
    walk(src);
    ck(sp_unwire_done(src.r), "wire end");
    return out;
  }

 private:
  struct Measure : Silent {
    size_t bytes = 0;
    void tag(uint8_t) { bytes += 1; }
    void len(size_t, size_t) { bytes += 8; }
    void points(size_t, size_t n, bool with_len) { bytes += 96 * n + (with_len ? 8 : 0); }
    void scalars(size_t, size_t n, bool with_len) { bytes += 32 * n + (with_len ? 8 : 0); }
  };
  size_t fe_count_ = 0, wire_len_ = 0;
};

}  // namespace spartan2
