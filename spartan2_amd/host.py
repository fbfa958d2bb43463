"""ctypes view of libspartan_host.so — the C++ host side above the C ABI (spartan2_amd/host/spartan_snark.cpp), which mirrors
SpartanSNARK::{setup, prep_prove, prove} (src/spartan.rs:146-466) and calls only include/spartan_hip.h."""
import ctypes
import os

import numpy as np

from . import hip

LIB_PATH = os.path.join(hip.LIB_DIR, "libspartan_host.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        hip.lib()  # libspartan_hip.so first (rpath $ORIGIN resolves it too)
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        L.ss_last_error.restype = ctypes.c_char_p
        L.ss_proof_words.restype = ctypes.c_size_t
        L.ssd_proof_words.restype, L.ssd_proof_words.argtypes = ctypes.c_size_t, [ctypes.c_void_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise hip.SpartanHipError(f"rc={rc}: {lib().ss_last_error().decode()}")


def _inst_args(inst):
    args = [ctypes.c_size_t(inst.num_cons), ctypes.c_size_t(inst.num_shared), ctypes.c_size_t(inst.num_precommitted), ctypes.c_size_t(inst.num_rest),
            ctypes.c_size_t(inst.num_public), ctypes.c_size_t(inst.num_challenges)]
    keep = []
    for d, i, p_ in inst.csr:
        d = np.ascontiguousarray(d, dtype=np.int64)
        i = np.ascontiguousarray(i, dtype=np.uint32)
        p_ = np.ascontiguousarray(p_, dtype=np.uint64)
        keep += [d, i, p_]
        args += [d.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), i.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), hip.p64(p_)]
    return args, keep


DIM_NAMES = ("num_cons", "num_cons_unpadded", "num_shared", "num_precommitted", "num_rest", "num_shared_unpadded", "num_precommitted_unpadded",
             "num_rest_unpadded", "num_public", "num_challenges")


def _padded_handle(inst):
    args, keep = _inst_args(inst)
    h = ctypes.c_void_p()
    _check(lib().ss_pad_shape(*args, ctypes.byref(h)))
    return h


def pad_shape(inst):
    """SplitR1CSShape::new (src/r1cs/mod.rs:810-911): padded CSR matrices with field coefficients + dims dict."""
    return _padded_export(_padded_handle(inst))


def pad_shapes_equalized(inst_a, inst_b):
    """SplitR1CSShape::new on both, then SplitR1CSShape::equalize (src/r1cs/mod.rs:913-971): -> ((mats, dims), (mats, dims))"""
    ha, hb = _padded_handle(inst_a), _padded_handle(inst_b)
    lib().ss_padded_equalize(ha, hb)
    return _padded_export(ha), _padded_export(hb)


def _padded_export(h):
    d = (ctypes.c_uint64 * 10)()
    lib().ss_padded_dims(h, d)
    dims = {k: int(v) for k, v in zip(DIM_NAMES, d)}
    mats = []
    for which in range(3):
        data = hip.c_u64p()
        idx = ctypes.POINTER(ctypes.c_uint32)()
        ptr = hip.c_u64p()
        nnz = ctypes.c_uint64()
        lib().ss_padded_csr(h, which, ctypes.byref(data), ctypes.byref(idx), ctypes.byref(ptr), ctypes.byref(nnz))
        n = int(nnz.value)
        mats.append((np.ctypeslib.as_array(data, (max(n, 1) * 4,))[: n * 4].reshape(n, 4).copy(), np.ctypeslib.as_array(idx, (max(n, 1),))[:n].copy(),
                     np.ctypeslib.as_array(ptr, (dims["num_cons"] + 1,)).copy()))
    lib().ss_padded_free(h)
    return mats, dims


def from_label(label: bytes, n: int):
    out = np.zeros((n, 8), dtype=np.uint64)
    _check(lib().ss_from_label(label, ctypes.c_size_t(n), hip.p64(out)))
    return out


REST_HOOK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, hip.c_u64p, ctypes.c_size_t, hip.c_u64p)
SP_ERR_UNSAT = -6  # SpartanError::UnSat: what ss_prep_is_sat / nnz_prep_is_sat return for a finding (the reason is in the report)
SS_BATCH_PER_PROOF_OPENING = 1  # ss_prove_batch_opts flag (host/spartan_snark.cpp)
SS_BATCH_PER_PROOF_POLYABC = 2  # ... one sp_eq_table_into + sp_poly_abc per proof
SS_BATCH_BATCHED_POLYABC = 4  # ... evals_rx + poly_ABC of all proofs through sp_poly_abc_batch
SS_BATCH_PER_PROOF_REST_COMMIT = 8  # ... one rest commitment call per proof
SS_BATCH_BATCHED_REST_COMMIT = 16  # ... the rest commitments of all proofs in one call
SS_BATCH_OPENING_AHEAD = 32  # ... the openings begun ahead of the sum-checks (sp_hyrax_prove_batch_begin / _rows / _finish)
SS_BATCH_OPENING_BEHIND = 64  # ... the openings as one sp_hyrax_prove_batch call behind the inner sum-check
SS_PREP_PER_STATE_COMMIT = 1  # ss_prep_prove_batch_opts / ss_prep_prove_sha256_batch_opts flags: one sp_hyrax_commit per state ...
SS_PREP_PER_STATE_MATVEC = 2  # ... one sp_multiply_vec per state (what the driver takes unless asked otherwise: measured, profiles/prep_prove_batch.md)
SS_PREP_CHUNKED_MATVEC = 4  # ... the cached products through sp_multiply_vec_chunked
NNZ_VERIFY_BATCH_PER_PROOF = 1  # nnz_verify_batch_opts flag (host/neutronnova_zk.cpp): one nnz_verify per proof
NNZ_VERIFY_BATCH_SHARED = 2  # ... the shared device stage and the combined opening from two proofs on
NNZ_PREP_PER_STATE_COMMIT = 1  # nnz_prep_prove_batch_opts / nnz_prep_prove_sha256_batch_opts flags: one sp_hyrax_commit per polynomial ...
NNZ_PREP_PER_STATE_LAYERS = 2  # ... nifs_prepare (a z and one sp_multiply_vec per layer) per state
NNZ_PREP_SHARED_COMMIT = 4  # ... sp_hyrax_commit_batch whatever the driver's default
NNZ_PREP_SHARED_LAYERS = 8  # ... sp_nifs_layers_batch whatever the driver's default
NNZ_BATCH_PER_PROOF = 1  # nnz_prove_batch_opts flags: a loop of nn_prove ...
NNZ_BATCH_LOCKSTEP = 2  # ... the two batched sum-checks of all proofs in lockstep, whatever the driver's default
NN_BATCH_PROVE_PHASES = ("head", "outer_before", "outer_sumcheck", "outer_after", "inner_before", "inner_sumcheck", "inner_after", "tail", "total", "lockstep")
PHASES = ("witness_commit", "matrix_vector_multiply", "outer_sumcheck", "prepare_poly_ABC", "inner_sumcheck", "pcs_prove", "total")


class VerifyBatchInfo(ctypes.Structure):  # ss_verify_batch_info
    _fields_ = [(n, ctypes.c_uint64) for n in ("matrix_chunks", "opening_batched_ok", "fallback_proofs", "opening_proofs")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SpartanSNARK:
    """setup -> prep_prove -> prove, as benches/sha256_spartan.rs:171-243 drives them."""

    def __init__(self, ctx: hip.Context, inst):
        self.ctx = ctx
        self.inst = inst
        args, keep = _inst_args(inst)
        self.pk = ctypes.c_void_p()
        _check(lib().ss_setup(ctx.h, *args, ctypes.byref(self.pk)))
        d = (ctypes.c_uint64 * 10)()
        dig = np.zeros(32, dtype=np.uint8)
        lib().ss_pk_info(self.pk, d, hip.p8(dig))
        self.dims = {k: int(v) for k, v in zip(DIM_NAMES, d)}
        self.vk_digest = dig
        self.ps = None
        self.batch = []  # prep_prove_batch's states: [(prep state, its public values)]
        self.publics = np.ascontiguousarray(inst.publics, dtype=np.uint64)  # the public values prove() states: the instance's, or prep_prove_sha256's
        self._sha_plan = None
        si = (ctypes.c_uint64 * 8)()
        _check(lib().ss_pk_shape_info(self.pk, si))
        self.shape_info = {"nnz": [int(si[i]) for i in range(3)], "nnz_filtered": [int(si[3 + i]) for i in range(3)], "long_columns": int(si[6]),
                           "short_columns": int(si[7])}

    def prep_prove(self, tape: np.ndarray, is_small=True):
        used = ctypes.c_size_t(0)
        w = np.ascontiguousarray(self.inst.witness, dtype=np.uint64)
        ps = ctypes.c_void_p()
        _check(lib().ss_prep_prove(self.pk, hip.p64(w), ctypes.c_size_t(len(w)), int(is_small), hip.p8(tape), ctypes.c_size_t(tape.shape[0]), ctypes.byref(used),
                                   ctypes.byref(ps)))
        self._free_ps()
        self.ps = ps
        self.publics = np.ascontiguousarray(self.inst.publics, dtype=np.uint64)
        return used.value

    def prep_prove_sha256(self, msg: bytes, tape: np.ndarray, is_small=True):
        """prep_prove with the witness generated on the device (ss_prep_prove_sha256) for a key set up from frontend.sha256_circuit(m), len(m) == len(msg):
        callable again and again on one key with different messages; the prove() that follows uses the digest bits of `msg` as public values (self.publics).
        The plan (frontend.sha256_witness_plan(len(msg))) is made on the first call and kept with the key."""
        msg = bytes(msg)
        if self._sha_plan is None or self._sha_plan.msg_len != len(msg):
            from . import frontend

            self._sha_plan = hip.Sha256Plan(self.ctx, frontend.sha256_witness_plan(len(msg)))
        used = ctypes.c_size_t(0)
        ps = ctypes.c_void_p()
        pub = np.zeros(256, dtype=np.uint64)
        buf = np.frombuffer(msg, dtype=np.uint8).copy()
        _check(lib().ss_prep_prove_sha256(self.pk, self._sha_plan.h, hip.p8(buf), ctypes.c_size_t(len(msg)), int(is_small), hip.p8(tape), ctypes.c_size_t(tape.shape[0]),
                                          ctypes.byref(used), ctypes.byref(ps), hip.p64(pub)))
        self._free_ps()
        self.ps = ps
        self.publics = pub
        return used.value

    def _free_ps(self):
        """drops self.ps; a state of self.batch that a caller assigned to self.ps (to prove it alone) stays with the batch"""
        if self.ps and not any(self.ps is b or self.ps.value == b.value for b, _ in self.batch):
            lib().ss_prep_free(self.ps)
        self.ps = None

    def _free_batch(self):
        for ps, _ in self.batch:
            if self.ps is not None and (self.ps is ps or self.ps.value == ps.value):
                self.ps = None
            lib().ss_prep_free(ps)
        self.batch = []

    def prep_prove_batch(self, tapes, witnesses=None, msgs=None, is_small=True, one_pass=True, per_state_commit=False, per_state_matvec=False, chunked_matvec=False):
        """K prep states on this one key for prove_batch, kept in self.batch with their public values (self.ps is left alone): from `msgs` (K messages
        of the key's length, as prep_prove_sha256), from `witnesses` (K instances of this key's circuit - objects with .witness and .publics), or
        K = len(tapes) states of the key's own instance. Returns the blocks used of each tape. State k is the state prep_prove / prep_prove_sha256 makes
        of witness / message k with tape k. By default all K are prepared in one pass (ss_prep_prove_batch_opts / ss_prep_prove_sha256_batch_opts: one
        witness launch, the commitments through sp_hyrax_commit_batch, one synchronise); per_state_commit (SS_PREP_PER_STATE_COMMIT) keeps one
        sp_hyrax_commit per state; the cached products are one sp_multiply_vec per state - per_state_matvec (SS_PREP_PER_STATE_MATVEC) says so
        explicitly - unless chunked_matvec (SS_PREP_CHUNKED_MATVEC) takes sp_multiply_vec_chunked, which was measured and does not win
        (profiles/prep_prove_batch.md); one_pass=False is a loop of single prep_prove calls.
        The phases of the last one-pass batch, ms: self.batch_prep_phases."""
        K = len(tapes)
        if msgs is not None and witnesses is not None:
            raise ValueError("prep_prove_batch: msgs or witnesses, not both")
        for name, v in (("msgs", msgs), ("witnesses", witnesses)):
            if v is not None and len(v) != K:
                raise ValueError(f"prep_prove_batch: {len(v)} {name} for {K} tapes")
        self._free_batch()
        if msgs is not None and K:
            msgs = [bytes(m) for m in msgs]
            if self._sha_plan is None or self._sha_plan.msg_len != len(msgs[0]):
                from . import frontend

                self._sha_plan = hip.Sha256Plan(self.ctx, frontend.sha256_witness_plan(len(msgs[0])))
        if not one_pass or K == 0:
            return self._prep_prove_loop(tapes, witnesses, msgs, is_small)
        flags = (SS_PREP_PER_STATE_COMMIT if per_state_commit else 0) | (SS_PREP_PER_STATE_MATVEC if per_state_matvec else 0) | (SS_PREP_CHUNKED_MATVEC if chunked_matvec else 0)
        tapes = [np.ascontiguousarray(t, dtype=np.uint8) for t in tapes]
        tptr = (hip.c_u8p * K)(*[hip.p8(t) for t in tapes])
        tblk = (ctypes.c_size_t * K)(*[t.shape[0] for t in tapes])
        used = (ctypes.c_size_t * K)()
        pss = (ctypes.c_void_p * K)()
        ms = (ctypes.c_double * 8)()
        if msgs is not None:
            n = len(msgs[0])
            for k, m in enumerate(msgs):
                if len(m) != n:
                    raise hip.SpartanHipError(f"prep_prove_batch: state {k}: a message of {len(m)} bytes in a batch of {n}-byte messages")
            buf = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy() if n else np.zeros(1, dtype=np.uint8)
            pubs = np.zeros((K, 256), dtype=np.uint64)
            _check(lib().ss_prep_prove_sha256_batch_opts(self.pk, self._sha_plan.h, hip.p8(buf), ctypes.c_size_t(n), ctypes.c_size_t(K), int(is_small), tptr, tblk, used,
                                                         pss, hip.p64(pubs), ms, ctypes.c_uint(flags)))
            pub_list = [pubs[k].copy() for k in range(K)]
        else:
            srcs = [self.inst] * K if witnesses is None else list(witnesses)
            ws = [np.ascontiguousarray(src.witness, dtype=np.uint64).reshape(-1) for src in srcs]
            d = self.dims
            want = d["num_shared_unpadded"] + d["num_precommitted_unpadded"] + d["num_rest_unpadded"]
            for k, w in enumerate(ws):  # (the entry point takes one length for all states)
                if len(w) != want:
                    raise hip.SpartanHipError(f"prep_prove_batch: state {k}: InvalidWitnessLength ({len(w)} words, the key takes {want})")
            wptr = (hip.c_u64p * K)(*[hip.p64(w) if len(w) else None for w in ws])
            _check(lib().ss_prep_prove_batch_opts(self.pk, wptr, ctypes.c_size_t(want), ctypes.c_size_t(K), int(is_small), tptr, tblk, used, pss, ms, ctypes.c_uint(flags)))
            pub_list = [np.ascontiguousarray(src.publics, dtype=np.uint64) for src in srcs]
        self.batch = [(ctypes.c_void_p(pss[k]), pub_list[k]) for k in range(K)]
        self.batch_prep_phases = dict(witness=ms[0], commit=ms[1], tables=ms[2], matvec=ms[3], scratch=ms[4], total=ms[6])
        return [int(used[k]) for k in range(K)]

    def _prep_prove_loop(self, tapes, witnesses, msgs, is_small):
        """prep_prove_batch(one_pass=False): one ss_prep_prove / ss_prep_prove_sha256 call per state"""
        used_all = []
        for k in range(len(tapes)):
            tape = tapes[k]
            used = ctypes.c_size_t(0)
            ps = ctypes.c_void_p()
            if msgs is not None:
                msg = msgs[k]
                pub = np.zeros(256, dtype=np.uint64)
                buf = np.frombuffer(msg, dtype=np.uint8).copy()
                _check(lib().ss_prep_prove_sha256(self.pk, self._sha_plan.h, hip.p8(buf), ctypes.c_size_t(len(msg)), int(is_small), hip.p8(tape),
                                                  ctypes.c_size_t(tape.shape[0]), ctypes.byref(used), ctypes.byref(ps), hip.p64(pub)))
            else:
                src = self.inst if witnesses is None else witnesses[k]
                w = np.ascontiguousarray(src.witness, dtype=np.uint64)
                pub = np.ascontiguousarray(src.publics, dtype=np.uint64)
                _check(lib().ss_prep_prove(self.pk, hip.p64(w), ctypes.c_size_t(len(w)), int(is_small), hip.p8(tape), ctypes.c_size_t(tape.shape[0]), ctypes.byref(used),
                                           ctypes.byref(ps)))
            self.batch.append((ps, pub))
            used_all.append(used.value)
        return used_all

    def prove_batch(self, tapes, states=None, per_proof_opening=False, per_proof_polyabc=None, per_proof_rest_commit=None, opening_ahead=None):
        """ss_prove_batch_opts over self.batch (or `states`, a list of (prep state, publics) pairs): one tape per proof -> ([(proof words, blocks used)],
        {phase: ms of the whole batch}). Proof k is word for word what prove() returns on state k with tape k; the outer and the inner sum-check of all
        proofs run in lockstep (sp_sumcheck_cubic3_lockstep / sp_sumcheck_quad_lockstep) and the openings are one sp_hyrax_prove_batch call -
        per_proof_opening=True (SS_BATCH_PER_PROOF_OPENING) keeps them as one sp_hyrax_prove per proof. opening_ahead: True = that opening begun ahead
        (sp_hyrax_prove_batch_begin once comm_W is complete, _rows from the inner sum-check's hook, _finish in its place: SS_BATCH_OPENING_AHEAD), False =
        the one call behind the inner sum-check (SS_BATCH_OPENING_BEHIND), None = what the driver measured to be faster; per_proof_opening wins. per_proof_polyabc: True = one sp_eq_table_into +
        sp_poly_abc per proof, False = one sp_poly_abc_batch call, None = what the driver measured to be faster; per_proof_rest_commit likewise for the
        rest commitments (one call per proof / one sp_fixed_base_mul_h or sp_hyrax_commit_batch call for all). Still per proof: the z assembly,
        sp_multiply_vec_incremental, the eval_W commitment and the lz_tables build."""
        flags = SS_BATCH_PER_PROOF_OPENING if per_proof_opening else 0
        if per_proof_polyabc is not None:
            flags |= SS_BATCH_PER_PROOF_POLYABC if per_proof_polyabc else SS_BATCH_BATCHED_POLYABC
        if per_proof_rest_commit is not None:
            flags |= SS_BATCH_PER_PROOF_REST_COMMIT if per_proof_rest_commit else SS_BATCH_BATCHED_REST_COMMIT
        if opening_ahead is not None:
            flags |= SS_BATCH_OPENING_AHEAD if opening_ahead else SS_BATCH_OPENING_BEHIND
        states = self.batch if states is None else states
        K = len(states)
        if len(tapes) != K:
            raise ValueError(f"prove_batch: {len(tapes)} tapes for {K} states")
        n = lib().ss_proof_words(self.pk)
        npub = self.dims["num_public"]
        words = np.zeros((max(K, 1), n), dtype=np.uint64)
        pubs = np.zeros((max(K, 1), max(npub, 1)), dtype=np.uint64)
        for k, (_, pub) in enumerate(states):
            pubs[k, : len(pub)] = pub
        pubs = np.ascontiguousarray(pubs[:, :npub]) if npub else pubs
        tapes = [np.ascontiguousarray(t, dtype=np.uint8) for t in tapes]
        tptr = (hip.c_u8p * max(K, 1))(*[hip.p8(t) for t in tapes])
        tblk = (ctypes.c_size_t * max(K, 1))(*[t.shape[0] for t in tapes])
        pss = (ctypes.c_void_p * max(K, 1))(*[ps for ps, _ in states])
        used = (ctypes.c_size_t * max(K, 1))()
        ms = (ctypes.c_double * 7)()
        _check(lib().ss_prove_batch_opts(self.pk, pss, ctypes.c_size_t(K), hip.p64(pubs) if npub else None, ctypes.c_size_t(npub), tptr, tblk, used, hip.p64(words),
                                         ctypes.c_size_t(n), ms, ctypes.c_uint(flags)))
        return [(words[k].copy(), int(used[k])) for k in range(K)], dict(zip(PHASES, list(ms)))

    def prep_phases(self):
        """host wall-clock of the last prep_prove's phases, ms (ss_prep_phases)"""
        out = (ctypes.c_double * 8)()
        lib().ss_prep_phases(self.ps, out)
        return dict(witness=out[0], commit=out[1], tables=out[2], matvec=out[3], scratch=out[4], total=out[6])

    def set_flags(self, prefix_cache=None, lz_direct=None, reference_order=None):
        """Driver options of the current prep state (spartan_snark.cpp FLAG_*): prefix_cache = keep the transcript prefix's sponge state across
        proves instead of re-hashing it in every prove (the reference re-hashes); lz_direct = the opening in the reference's own order."""
        lib().ss_prep_get_flags.restype = ctypes.c_uint
        f = lib().ss_prep_get_flags(self.ps)
        if prefix_cache is not None:
            f = (f | 1) if prefix_cache else (f & ~1)
        if lz_direct is not None:
            f = (f | 2) if lz_direct else (f & ~2)
        if reference_order is not None:  # one thread, the reference's statement order, only ABI calls (spartan_snark.cpp prove_reference_order)
            f = (f | 4) if reference_order else (f & ~4)
        lib().ss_prep_set_flags(self.ps, ctypes.c_uint(f))

    def prep_export(self):
        d = self.dims
        rows = ((d["num_shared"] + 2047) // 2048 if d["num_shared_unpadded"] else 0) + ((d["num_precommitted"] + 2047) // 2048 if d["num_precommitted_unpadded"] else 0)
        N = self.dims["num_cons"]
        comm = np.zeros((rows, 8), dtype=np.uint64)
        caz = np.zeros((N, 4), dtype=np.uint64)
        cbz = np.zeros_like(caz)
        ccz = np.zeros_like(caz)
        _check(lib().ss_prep_export(self.pk, self.ps, hip.p64(comm) if rows else None, hip.p64(caz), hip.p64(cbz), hip.p64(ccz)))
        return comm, caz, cbz, ccz

    def _rest_hook(self, synthesize):
        """the circuit's synthesize callback (challenges (k, 4) -> rest witness (num_rest_unpadded, 4)) behind the C hook type prove and is_sat take"""
        if synthesize is None:
            return None
        nrest = self.dims["num_rest_unpadded"]

        def raw(_user, ch_ptr, nch, out_ptr):
            try:
                ch = np.ctypeslib.as_array(ch_ptr, shape=(4 * nch,)).reshape(nch, 4).copy()
                rest = np.ascontiguousarray(synthesize(ch), dtype=np.uint64).reshape(nrest, 4)
                np.ctypeslib.as_array(out_ptr, shape=(4 * max(nrest, 1),))[: 4 * nrest] = rest.reshape(-1)
                return 0
            except Exception:  # noqa: BLE001
                import traceback

                traceback.print_exc()
                return 1

        return REST_HOOK(raw)

    def prove(self, tape: np.ndarray, synthesize=None):
        """Returns (proof words in the canonical layout, tape blocks used, {phase: ms}). Circuits with verifier challenges pass
        synthesize(challenges (k, 4)) -> rest witness (num_rest_unpadded, 4) Montgomery limbs (circuit.synthesize, bellpepper/r1cs.rs:443-461)."""
        n = lib().ss_proof_words(self.pk)
        words = np.zeros(n, dtype=np.uint64)
        used = ctypes.c_size_t(0)
        ms = (ctypes.c_double * 7)()
        pub = self.publics
        cb = self._rest_hook(synthesize)
        _check(lib().ss_prove_hook(self.pk, self.ps, hip.p64(pub) if len(pub) else None, ctypes.c_size_t(len(pub)), hip.p8(tape), ctypes.c_size_t(tape.shape[0]),
                                   ctypes.byref(used), hip.p64(words), ctypes.c_size_t(n), ms, cb, None))
        return words, used.value, dict(zip(PHASES, list(ms)))

    def is_sat(self, publics=None, challenges=None, synthesize=None, commitment=None) -> hip.SatReport:
        """R1CSShape::is_sat (src/r1cs/mod.rs:358-394) on the prepared state, on the device: does the witness the state holds satisfy the circuit for these
        public values (default: self.publics - after prep_prove_sha256 the digest bits of that message), and are the rows committed at prep_prove the
        commitment of that witness? Circuits with verifier challenges pass challenges (k, 4) - a prove's, or any - and the synthesize callback prove takes.
        commitment: (rows, 8) affine rows to compare with instead of the state's own (prep_export()[0] has that layout). A finding is the returned
        SatReport, not an exception; a later prove() on the state is unaffected."""
        if not self.ps:
            raise hip.SpartanHipError("is_sat before prep_prove")
        pub = self.publics if publics is None else np.ascontiguousarray(publics, dtype=np.uint64).reshape(-1)
        cb = self._rest_hook(synthesize)
        ch = None
        if challenges is not None:
            ch = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1, 4)
            if ch.shape[0] != self.dims["num_challenges"]:
                raise hip.SpartanHipError(f"is_sat: {ch.shape[0]} challenges for a circuit with {self.dims['num_challenges']}")
        d = self.dims
        rows = ((d["num_shared"] + 2047) // 2048 if d["num_shared_unpadded"] else 0) + ((d["num_precommitted"] + 2047) // 2048 if d["num_precommitted_unpadded"] else 0)
        comm = None
        if commitment is not None:
            comm = np.ascontiguousarray(commitment, dtype=np.uint64).reshape(-1, 8)
            if comm.shape[0] != rows:
                raise hip.SpartanHipError(f"is_sat: {comm.shape[0]} commitment rows, the state holds {rows}")
        rep = hip._SatReport()
        bad = np.zeros(max(rows, 1), dtype=np.uint64)
        nbad = ctypes.c_size_t(0)
        rc = lib().ss_prep_is_sat(self.pk, self.ps, hip.p64(pub) if len(pub) else None, ctypes.c_size_t(len(pub)), hip.p64(ch) if ch is not None and len(ch) else None, cb,
                                  None, hip.p64(comm) if comm is not None and rows else None, ctypes.byref(rep), hip.p64(bad), ctypes.c_size_t(len(bad)), ctypes.byref(nbad))
        if rc not in (0, SP_ERR_UNSAT):
            _check(rc)
        return hip.SatReport(rep, bad[: nbad.value])

    def verify(self, words: np.ndarray) -> int:
        """SpartanSNARK::verify (src/spartan.rs:469-578) with the matrix evaluations and MSMs on the device: 0 = accept, 1..6 = failed check."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        pub = np.zeros((max(self.dims["num_public"], 1), 4), dtype=np.uint64)
        rc = lib().ss_verify(self.pk, hip.p64(words), ctypes.c_size_t(words.shape[0]), hip.p64(pub))
        if rc < 0:
            _check(rc)
        self.verified_publics = pub[: self.dims["num_public"]] if rc == 0 else None  # what verify() returns in the reference (src/spartan.rs:577)
        return rc

    # ---- wire formats (bincode framing of the reference's serde types; include/spartan_hip.h "wire formats") ----
    def proof_layout(self) -> dict:
        L = hip.SpartanLayout()
        lib().ss_proof_layout(self.pk, ctypes.byref(L))
        return L.as_dict()

    def proof_to_bytes(self, words: np.ndarray) -> bytes:
        words = np.ascontiguousarray(words, dtype=np.uint64)
        n = ctypes.c_size_t(0)
        _check(lib().ss_proof_to_bytes(self.pk, hip.p64(words), ctypes.c_size_t(len(words)), None, ctypes.c_size_t(0), ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        _check(lib().ss_proof_to_bytes(self.pk, hip.p64(words), ctypes.c_size_t(len(words)), hip.p8(out), ctypes.c_size_t(n.value), ctypes.byref(n)))
        return out.tobytes()

    def vk_to_bytes(self) -> bytes:
        """The key's SpartanVerifierKey { vk_ee, ck_s, S } (src/spartan.rs:62-70) as bincode bytes (ss_vk_to_bytes): what SpartanVerifier.from_bytes loads.
        The circuit is handed to the library again (setup keeps no copy of it) and the bytes are returned only if they hash to this key's digest."""
        args, keep = _inst_args(self.inst)
        fn = lib().ss_vk_to_bytes
        fn.restype = ctypes.c_long
        n = fn(self.pk, *args, None, ctypes.c_size_t(0))
        if n < 0:
            _check(n)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        got = fn(self.pk, *args, hip.p8(out), ctypes.c_size_t(n))
        if got < 0:
            _check(got)
        assert got == n, (got, n)
        return out[:n].tobytes()

    def pk_to_bytes(self) -> bytes:
        """The key's SpartanProverKey { ck, ck_s, S, vk_digest } (src/spartan.rs:42-49) as bincode bytes (ss_pk_to_bytes): vk_to_bytes() followed by the 32
        digest bytes - what SpartanProver.from_bytes loads."""
        args, keep = _inst_args(self.inst)
        fn = lib().ss_pk_to_bytes
        fn.restype = ctypes.c_long
        n = fn(self.pk, *args, None, ctypes.c_size_t(0))
        if n < 0:
            _check(n)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        got = fn(self.pk, *args, hip.p8(out), ctypes.c_size_t(n))
        if got < 0:
            _check(got)
        assert got == n, (got, n)
        return out[:n].tobytes()

    def verify_bytes(self, data: bytes) -> int:
        """verify() on a serialised proof: 0 = accept, 1..6 = failed check (1 also for bytes that do not decode to a proof of this key's shape)."""
        arr = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
        pub = np.zeros((max(self.dims["num_public"], 1), 4), dtype=np.uint64)
        rc = lib().ss_verify_bytes(self.pk, hip.p8(arr), ctypes.c_size_t(len(data)), hip.p64(pub))
        if rc < 0:
            _check(rc)
        return rc

    def _verify_batch(self, fn, items, lens, keep, seed, info):
        n = len(lens)  # (items is a ctypes array of at least one slot; keep holds the arrays it points into)
        npub = self.dims["num_public"]
        codes = (ctypes.c_int * max(n, 1))()
        pub = np.zeros((max(n, 1), max(npub, 1), 4), dtype=np.uint64)
        inf = VerifyBatchInfo()
        sd = None
        if seed is not None:
            sd = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
            assert sd.shape[0] == 32, "seed must be 32 bytes"
        _check(fn(self.pk, items, (ctypes.c_size_t * max(n, 1))(*lens), ctypes.c_size_t(n), hip.p8(sd) if sd is not None else None, codes, hip.p64(pub),
                  ctypes.byref(inf)))
        out = [int(codes[k]) for k in range(n)]
        if not info:
            return out
        return out, [pub[k, :npub].copy() if out[k] == 0 else None for k in range(n)], inf.as_dict()

    def verify_batch(self, proofs, seed=None, info=False):
        """verify() for every proof of `proofs` (flat word arrays of this key) in one pass: the matrix evaluations of KC proofs per launch, the openings of
        all proofs as one random linear combination (spartan_snark.cpp verify_batch). -> the list of verify()'s codes; with info=True
        (codes, publics, info): publics[k] = the accepted public values or None, info = {matrix_chunks, opening_batched_ok, fallback_proofs,
        opening_proofs}. seed: 32 bytes mixed into the weights of the combined check, or None. A batch of one is verify() itself."""
        ws = [np.ascontiguousarray(w, dtype=np.uint64).reshape(-1) for w in proofs]
        n = len(ws)
        ptrs = (hip.c_u64p * max(n, 1))(*[hip.p64(w) if w.shape[0] else None for w in ws])
        return self._verify_batch(lib().ss_verify_batch, ptrs, [w.shape[0] for w in ws], ws, seed, info)

    def verify_bytes_batch(self, blobs, seed=None, info=False):
        """verify_batch() over serialised proofs (proof_to_bytes): bytes that do not decode to a proof of this key's shape get code 1."""
        bs = [np.frombuffer(bytes(b), dtype=np.uint8).copy() if len(b) else np.zeros(1, dtype=np.uint8) for b in blobs]
        n = len(bs)
        ptrs = (hip.c_u8p * max(n, 1))(*[hip.p8(b) for b in bs])
        return self._verify_batch(lib().ss_verify_bytes_batch, ptrs, [len(b) for b in blobs], bs, seed, info)

    def close(self):
        if getattr(self, "batch", None):
            self._free_batch()
        if self.ps:
            lib().ss_prep_free(self.ps)
            self.ps = None
        if getattr(self, "_sha_plan", None) is not None:
            self._sha_plan.free()
            self._sha_plan = None
        if self.pk:
            lib().ss_pk_free(self.pk)
            self.pk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpartanVerifier:
    """A verifier's key loaded from the bincode bytes of SpartanVerifierKey (ss_verifier_from_bytes): no circuit, no frontend, no setup. It holds the two
    commitment keys, the row-major matrix structures and the digest - what verify reads - and verifies with the code SpartanSNARK's methods run."""

    def __init__(self):
        raise TypeError("use SpartanVerifier.from_bytes(ctx, data)")

    @classmethod
    def from_bytes(cls, ctx: hip.Context, data, device_decode=None, timed=False):
        """data: SpartanSNARK.vk_to_bytes() (or the oracle's vk_bytes()). device_decode: True / False forces the device / host decode of the matrices,
        None takes the measured default. Raises on bytes that are not a key (short, trailing, inconsistent, off-curve, non-canonical ...)."""
        flags = 0 if device_decode is None else (hip.SHAPE_WIRE_DEVICE if device_decode else hip.SHAPE_WIRE_HOST)
        if timed:
            flags |= hip.SHAPE_WIRE_TIMED
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if data is not None else None
        self = cls.__new__(cls)
        self.ctx = ctx
        self.pk = ctypes.c_void_p()
        _check(lib().ss_verifier_from_bytes(ctx.h if ctx is not None else None, hip.p8(buf) if buf is not None and len(buf) else None,
                                            ctypes.c_size_t(len(buf) if buf is not None else 0), ctypes.c_uint(flags), ctypes.byref(self.pk)))
        self.stages = hip.wire_stages()  # of the shape's decode; .load_stages: of the whole load
        st = (ctypes.c_double * 8)()
        lib().ss_verifier_stages(st)
        self.load_stages = {k: float(v) for k, v in zip(("hyrax_keys", "shape", "ck_create", "digest", "digest_wait", "total"), st)}
        d = (ctypes.c_uint64 * 10)()
        dig = np.zeros(32, dtype=np.uint8)
        lib().ss_pk_info(self.pk, d, hip.p8(dig))
        self.dims = {k: int(v) for k, v in zip(DIM_NAMES, d)}
        self.vk_digest = dig
        si = (ctypes.c_uint64 * 8)()
        _check(lib().ss_pk_shape_info(self.pk, si))
        self.shape_info = {"nnz": [int(si[i]) for i in range(3)], "nnz_filtered": [int(si[3 + i]) for i in range(3)], "long_columns": int(si[6]),
                           "short_columns": int(si[7])}
        return self

    verify = SpartanSNARK.verify
    verify_bytes = SpartanSNARK.verify_bytes
    _verify_batch = SpartanSNARK._verify_batch
    verify_batch = SpartanSNARK.verify_batch
    verify_bytes_batch = SpartanSNARK.verify_bytes_batch
    proof_layout = SpartanSNARK.proof_layout
    proof_to_bytes = SpartanSNARK.proof_to_bytes

    def close(self):
        if getattr(self, "pk", None):
            lib().ss_verifier_free(self.pk)
            self.pk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SS_PK_TRUST_DIGEST = 1 << 16  # ss_prover_from_bytes flag: take the stored digest as it is (outside the SP_SHAPE_WIRE_* range)


class _CallerInstance:
    """what SpartanSNARK's prep methods read of an instance, for a key that has none: the caller's witness words and public values"""

    def __init__(self, witness, publics):
        self.witness = np.ascontiguousarray(witness, dtype=np.uint64).reshape(-1)
        self.publics = np.ascontiguousarray(publics if publics is not None else [], dtype=np.uint64).reshape(-1)


class SpartanProver:
    """A prover's key loaded from the bincode bytes of SpartanProverKey (ss_prover_from_bytes): no circuit, no frontend instance, no setup. The key is
    an ordinary prover key - the full shape, both commitment keys, the digest - and proves and verifies with the code SpartanSNARK's methods run."""

    def __init__(self):
        raise TypeError("use SpartanProver.from_bytes(ctx, data)")

    @classmethod
    def from_bytes(cls, ctx: hip.Context, data, trust_digest=False, full_device=None, timed=False):
        """data: SpartanSNARK.pk_to_bytes(). By default the digest is hashed from the bytes and a key whose stored digest differs is refused;
        trust_digest=True takes the stored one (SS_PK_TRUST_DIGEST). full_device: True / False forces the device / host build of the full shape
        (SP_SHAPE_WIRE_FULL_DEVICE / SP_SHAPE_WIRE_FULL), None takes the measured default."""
        flags = 0 if full_device is None else (hip.SHAPE_WIRE_FULL_DEVICE if full_device else hip.SHAPE_WIRE_FULL)
        if trust_digest:
            flags |= SS_PK_TRUST_DIGEST
        if timed:
            flags |= hip.SHAPE_WIRE_TIMED
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if data is not None else None
        self = cls.__new__(cls)
        self.ctx = ctx
        self.inst = None
        self.pk = ctypes.c_void_p()
        self.ps = None
        self.batch = []
        self.publics = np.zeros(0, dtype=np.uint64)
        self._sha_plan = None
        _check(lib().ss_prover_from_bytes(ctx.h if ctx is not None else None, hip.p8(buf) if buf is not None and len(buf) else None,
                                          ctypes.c_size_t(len(buf) if buf is not None else 0), ctypes.c_uint(flags), ctypes.byref(self.pk)))
        self.stages = hip.wire_stages()  # of the shape's decode; .full_stages: of its full part; .load_stages: of the whole load
        self.full_stages = hip.wire_full_stages()
        st = (ctypes.c_double * 8)()
        lib().ss_prover_stages(st)
        self.load_stages = {k: float(v) for k, v in zip(("hyrax_keys", "shape", "ck_create", "digest", "digest_wait", "total", "full_device", "digest_hashed"), st)}
        d = (ctypes.c_uint64 * 10)()
        dig = np.zeros(32, dtype=np.uint8)
        lib().ss_pk_info(self.pk, d, hip.p8(dig))
        self.dims = {k: int(v) for k, v in zip(DIM_NAMES, d)}
        self.vk_digest = dig
        si = (ctypes.c_uint64 * 8)()
        _check(lib().ss_pk_shape_info(self.pk, si))
        self.shape_info = {"nnz": [int(si[i]) for i in range(3)], "nnz_filtered": [int(si[3 + i]) for i in range(3)], "long_columns": int(si[6]),
                           "short_columns": int(si[7])}
        return self

    def prep_prove(self, tape: np.ndarray, witness, publics, is_small=True):
        """SpartanSNARK.prep_prove on the caller's witness words; the prove() that follows states `publics`"""
        self.inst = _CallerInstance(witness, publics)
        return SpartanSNARK.prep_prove(self, tape, is_small)

    def prep_prove_batch(self, tapes, witnesses=None, msgs=None, publics=None, is_small=True, **opts):
        """SpartanSNARK.prep_prove_batch from `msgs`, or from `witnesses` (K arrays of witness words) with `publics` (K arrays of public values)"""
        if witnesses is not None:
            if publics is None or len(publics) != len(witnesses):
                raise ValueError("prep_prove_batch: one array of public values for every witness")
            witnesses = [_CallerInstance(w, p) for w, p in zip(witnesses, publics)]
        elif msgs is None:
            raise ValueError("prep_prove_batch: a key loaded from its bytes has no instance of its own (pass witnesses= and publics=, or msgs=)")
        return SpartanSNARK.prep_prove_batch(self, tapes, witnesses=witnesses, msgs=msgs, is_small=is_small, **opts)

    prep_prove_sha256 = SpartanSNARK.prep_prove_sha256
    _prep_prove_loop = SpartanSNARK._prep_prove_loop
    _free_ps = SpartanSNARK._free_ps
    _free_batch = SpartanSNARK._free_batch
    _rest_hook = SpartanSNARK._rest_hook
    prep_phases = SpartanSNARK.prep_phases
    set_flags = SpartanSNARK.set_flags
    prep_export = SpartanSNARK.prep_export
    prove = SpartanSNARK.prove
    prove_batch = SpartanSNARK.prove_batch
    is_sat = SpartanSNARK.is_sat
    verify = SpartanSNARK.verify
    verify_bytes = SpartanSNARK.verify_bytes
    _verify_batch = SpartanSNARK._verify_batch
    verify_batch = SpartanSNARK.verify_batch
    verify_bytes_batch = SpartanSNARK.verify_bytes_batch
    proof_layout = SpartanSNARK.proof_layout
    proof_to_bytes = SpartanSNARK.proof_to_bytes
    close = SpartanSNARK.close
    __del__ = SpartanSNARK.__del__


# ---- NeutronNovaNIFS::prove (spartan2_amd/host/neutronnova_nifs.cpp) ----------------------------------------------------------
NIFS_HOOK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_size_t, hip.c_u64p, hip.c_u64p)


def _c_hook(py_hook):
    def raw(_user, t, coeffs_ptr, out_ptr):
        coeffs = np.ctypeslib.as_array(coeffs_ptr, shape=(16,)).reshape(4, 4).copy()
        r = py_hook(int(t), coeffs)
        if r is not None:
            r = np.ascontiguousarray(r, dtype=np.uint64).reshape(4)
            for i in range(4):
                out_ptr[i] = int(r[i])

    return NIFS_HOOK(raw)


def tensor_decomp(n: int):
    """compute_tensor_decomp (src/neutronnova_zk.rs:56-67)."""
    ell = max(n - 1, 0).bit_length()
    return ell, 1 << ((ell + 1) // 2), 1 << (ell // 2)


_P256 = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF  # scalar field of the bench engine (src/provider/pt256.rs:55)


def mont_limbs_from_u64(vals):
    """(n,) uint64 integers -> (n, 4) Montgomery limbs of the engine's scalar field (harness helper: witness vectors of the integer R1CS generators)."""
    vals = np.ascontiguousarray(vals, dtype=np.uint64)
    u, inv = np.unique(vals, return_inverse=True)
    tab = np.array([[((int(v) << 256) % _P256 >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in u], dtype=np.uint64).reshape(-1, 4)
    return tab[inv]


def padded_witness_limbs(dims: dict, witness):
    """[shared | precommitted | rest] with every segment zero-padded to its padded length (SplitR1CSShape layout, src/r1cs/mod.rs:810-911)."""
    w = mont_limbs_from_u64(witness)
    s, p, r = dims["num_shared_unpadded"], dims["num_precommitted_unpadded"], dims["num_rest_unpadded"]
    out = np.zeros((dims["num_shared"] + dims["num_precommitted"] + dims["num_rest"], 4), dtype=np.uint64)
    out[:s] = w[:s]
    out[dims["num_shared"] : dims["num_shared"] + p] = w[s : s + p]
    out[dims["num_shared"] + dims["num_precommitted"] : dims["num_shared"] + dims["num_precommitted"] + r] = w[s + p : s + p + r]
    return out


def nifs_prepare(ctx: hip.Context, shape: hip.Shape, dims: dict, X, W_tables, small_values: bool):
    """The prep_prove part of the NIFS (cached_step_matvec / cached_step_i64, src/neutronnova_zk.rs:1520-1600): layers (+ i64 mirrors) of the
    instances. Returns an opaque handle for nifs_prove(prepared=...); free with nifs_free."""
    n = len(W_tables)
    d = dims["num_public"]
    X = np.ascontiguousarray(X, dtype=np.uint64).reshape(n, d, 4)
    d10 = (ctypes.c_uint64 * 10)(*[dims[k] for k in DIM_NAMES])
    warr = (ctypes.c_void_p * n)(*[t.h for t in W_tables])
    h = ctypes.c_void_p()
    _check(lib().nn_nifs_prepare(ctx.h, shape.h, d10, ctypes.c_size_t(n), hip.p64(X.reshape(-1)) if d else None, warr, 1 if small_values else 0, ctypes.byref(h)))
    return h


def nifs_free(handle):
    hip.lib().sp_nifs_free(handle)


def nifs_prove(ctx: hip.Context, shape: hip.Shape, dims: dict, ck: hip.CommitmentKey, comms, X, W_tables, r_W, small_values: bool, tr: hip.Transcript, py_hook,
               prepared=None):
    """NeutronNovaNIFS::prove (src/neutronnova_zk.rs:511-1273). comms (n, rows, 8), X (n, d, 4), W_tables: n resident witness tables,
    r_W (n, rows, 4); py_hook(t, coeffs (4,4)) -> r_b is the caller's `process_round`. Returns a dict of host arrays and device tables."""
    comms = np.ascontiguousarray(comms, dtype=np.uint64)
    n, rows = comms.shape[0], comms.shape[1]
    d = dims["num_public"]
    X = np.ascontiguousarray(X, dtype=np.uint64).reshape(n, d, 4)
    r_W = np.ascontiguousarray(r_W, dtype=np.uint64).reshape(n, rows, 4)
    n_padded = max(2, 1 << (n - 1).bit_length())
    ell_b = n_padded.bit_length() - 1
    _, left, right = tensor_decomp(dims["num_cons"])
    N, nv = dims["num_cons"], dims["num_shared"] + dims["num_precommitted"] + dims["num_rest"]
    out = dict(polys=np.zeros((ell_b, 4, 4), dtype=np.uint64), r_bs=np.zeros((ell_b, 4), dtype=np.uint64), E_eq=np.zeros((left + right, 4), dtype=np.uint64),
               tail=np.zeros((2, 4), dtype=np.uint64), folded_rW=np.zeros((rows, 4), dtype=np.uint64), folded_X=np.zeros((max(d, 1), 4), dtype=np.uint64),
               folded_comm=np.zeros((rows, 8), dtype=np.uint64))
    tabs = dict(A=hip.Table.zeros(ctx, N), B=hip.Table.zeros(ctx, N), C=hip.Table.zeros(ctx, N), folded_W=hip.Table.zeros(ctx, nv))
    d10 = (ctypes.c_uint64 * 10)(*[dims[k] for k in DIM_NAMES])
    warr = (ctypes.c_void_p * n)(*[t.h for t in W_tables])
    cb = _c_hook(py_hook)
    _check(lib().nn_nifs_prove(ctx.h, shape.h, d10, ck.h, ctypes.c_size_t(n), ctypes.c_size_t(rows), hip.p64(comms.reshape(-1)), hip.p64(X.reshape(-1)) if d else None,
                               warr, hip.p64(r_W.reshape(-1)), 1 if small_values else 0, prepared, tr.h, cb, None, hip.p64(out["polys"]), hip.p64(out["r_bs"]),
                               hip.p64(out["E_eq"]), hip.p64(out["tail"]), hip.p64(out["folded_rW"]), hip.p64(out["folded_X"]), hip.p64(out["folded_comm"]),
                               tabs["A"].h, tabs["B"].h, tabs["C"].h, tabs["folded_W"].h))
    out["folded_X"] = out["folded_X"][:d]
    out.update(tabs)
    return out


def nifs_prove_sharded(ctx: hip.Context, comm, shape: hip.Shape, dims: dict, ck: hip.CommitmentKey, comms_local, X_local, W_tables_local, r_W_local, small_values: bool,
                       tr: hip.Transcript, py_hook, prepared=None, out_tabs=None):
    """NeutronNovaNIFS::prove with the instances sharded over the ranks of `comm` (spartan2_amd/host/neutronnova_nifs.cpp nifs_prove_sharded,
    SURVEY.md 8(e)): this rank passes its n_local consecutive instances; every rank returns the same outputs as `nifs_prove` on the whole batch."""
    comms_local = np.ascontiguousarray(comms_local, dtype=np.uint64)
    n_local, rows = comms_local.shape[0], comms_local.shape[1]
    d = dims["num_public"]
    X_local = np.ascontiguousarray(X_local, dtype=np.uint64).reshape(n_local, d, 4)
    r_W_local = np.ascontiguousarray(r_W_local, dtype=np.uint64).reshape(n_local, rows, 4)
    n = n_local * comm.world
    ell_b = n.bit_length() - 1
    _, left, right = tensor_decomp(dims["num_cons"])
    N, nv = dims["num_cons"], dims["num_shared"] + dims["num_precommitted"] + dims["num_rest"]
    out = dict(polys=np.zeros((ell_b, 4, 4), dtype=np.uint64), r_bs=np.zeros((ell_b, 4), dtype=np.uint64), E_eq=np.zeros((left + right, 4), dtype=np.uint64),
               tail=np.zeros((2, 4), dtype=np.uint64), folded_rW=np.zeros((rows, 4), dtype=np.uint64), folded_X=np.zeros((max(d, 1), 4), dtype=np.uint64),
               folded_comm=np.zeros((rows, 8), dtype=np.uint64))
    tabs = out_tabs if out_tabs is not None else dict(A=hip.Table.zeros(ctx, N), B=hip.Table.zeros(ctx, N), C=hip.Table.zeros(ctx, N), folded_W=hip.Table.zeros(ctx, nv))
    d10 = (ctypes.c_uint64 * 10)(*[dims[k] for k in DIM_NAMES])
    warr = (ctypes.c_void_p * n_local)(*[t.h for t in W_tables_local])
    cb = _c_hook(py_hook)
    _check(lib().nn_nifs_prove_sharded(ctx.h, comm.h, shape.h, d10, ck.h, ctypes.c_size_t(n_local), ctypes.c_size_t(rows), hip.p64(comms_local.reshape(-1)),
                                       hip.p64(X_local.reshape(-1)) if d else None, warr, hip.p64(r_W_local.reshape(-1)), 1 if small_values else 0, prepared, tr.h, cb,
                                       None, hip.p64(out["polys"]), hip.p64(out["r_bs"]), hip.p64(out["E_eq"]), hip.p64(out["tail"]), hip.p64(out["folded_rW"]),
                                       hip.p64(out["folded_X"]), hip.p64(out["folded_comm"]), tabs["A"].h, tabs["B"].h, tabs["C"].h, tabs["folded_W"].h))
    out["folded_X"] = out["folded_X"][:d]
    out.update(tabs)
    return out


# ---- multi-GPU: the exchange layer and the sharded prover (spartan2_amd/host/{comm.hpp, sharded_snark.cpp}) -----------------------------
_ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


class Comm:
    """One all-gather primitive over the ranks of the job. backend "rccl": ncclAllGather from C++ on a communicator of its own
    (the unique id travels through torch.distributed once, at creation); backend "torch": a callback into torch.distributed.all_gather (gloo in
    the tests, where the ranks share one GPU and RCCL cannot be used); world 1 without torch.distributed: "rccl" still creates a one-rank
    communicator so that the production path is the one exercised."""

    def __init__(self, rank: int, world: int, backend: str, device: int = 0):
        import torch

        self.rank, self.world, self.backend = rank, world, backend
        self.h = ctypes.c_void_p()
        self._cb = None
        if backend == "rccl":
            uid = np.zeros(128, dtype=np.uint8)
            if rank == 0:
                _check(lib().ssc_rccl_unique_id(hip.p8(uid)))
            if world > 1:
                import torch.distributed as dist

                t = torch.from_numpy(uid)
                if dist.get_backend() == "nccl":  # (PyTorch's name for its RCCL backend on ROCm)
                    t = t.to("cuda")  # (PyTorch's device-type name for the HIP device)
                dist.broadcast(t, src=0)
                uid = t.cpu().numpy().copy()
            _check(lib().ssc_comm_rccl(int(device), int(rank), int(world), hip.p8(uid), ctypes.byref(self.h)))
        elif backend == "torch":
            import torch.distributed as dist

            def raw(_user, send, nbytes, recv):
                try:
                    src = np.ctypeslib.as_array(ctypes.cast(send, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
                    mine = torch.from_numpy(src.copy())
                    outs = [torch.empty_like(mine) for _ in range(world)]
                    dist.all_gather(outs, mine)
                    dst = np.ctypeslib.as_array(ctypes.cast(recv, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes * world,))
                    for r, o in enumerate(outs):
                        dst[r * nbytes : (r + 1) * nbytes] = o.numpy()
                    return 0
                except Exception:  # noqa: BLE001 — an exception must not unwind through the C frames
                    import traceback

                    traceback.print_exc()
                    return 1

            self._cb = _ALLGATHER_FN(raw)
            _check(lib().ssc_comm_callback(int(rank), int(world), self._cb, None, ctypes.byref(self.h)))
        else:
            raise ValueError(backend)

    def allgather(self, arr: np.ndarray) -> np.ndarray:
        arr = np.ascontiguousarray(arr)
        out = np.zeros((self.world,) + arr.shape, dtype=arr.dtype)
        _check(lib().ssc_comm_allgather(self.h, arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(arr.nbytes), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def stats(self):
        s = (ctypes.c_uint64 * 2)()
        lib().ssc_comm_stats(self.h, s)
        lib().ssc_comm_small_calls.restype = ctypes.c_uint64
        return {"exchanges": int(s[0]), "bytes_gathered": int(s[1]), "copy_free_exchanges": int(lib().ssc_comm_small_calls(self.h))}

    def close(self):
        if self.h:
            lib().ssc_comm_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SHARDED_PHASES = PHASES + ("exchanges",)


class ShardedSpartanSNARK:
    """ONE proof over all ranks of `comm` (row-sharded commitment and Az/Bz/Cz, slice-sharded sum-checks, column-sharded poly_ABC, point-range
    MSMs); every rank calls every method with the same arguments and receives the same proof words."""

    def __init__(self, ctx: hip.Context, comm: Comm, inst):
        self.ctx, self.comm, self.inst = ctx, comm, inst
        args, keep = _inst_args(inst)
        self.pk = ctypes.c_void_p()
        _check(lib().ssd_setup(ctx.h, comm.h, *args, ctypes.byref(self.pk)))
        d = (ctypes.c_uint64 * 10)()
        lib().ssd_pk_info(self.pk, d)
        self.dims = {k: int(v) for k, v in zip(DIM_NAMES, d)}
        self.ps = None

    def prep_prove(self, tape: np.ndarray, is_small=True):
        used = ctypes.c_size_t(0)
        w = np.ascontiguousarray(self.inst.witness, dtype=np.uint64)
        ps = ctypes.c_void_p()
        _check(lib().ssd_prep_prove(self.pk, hip.p64(w), ctypes.c_size_t(len(w)), int(is_small), hip.p8(tape), ctypes.c_size_t(tape.shape[0]), ctypes.byref(used),
                                    ctypes.byref(ps)))
        if self.ps:
            lib().ssd_prep_free(self.ps)
        self.ps = ps
        return used.value

    def proof_words(self):
        return lib().ssd_proof_words(self.pk)

    def prove(self, tape: np.ndarray):
        n = self.proof_words()
        words = np.zeros(n, dtype=np.uint64)
        used = ctypes.c_size_t(0)
        ms = (ctypes.c_double * 8)()
        pub = np.ascontiguousarray(self.inst.publics, dtype=np.uint64)
        _check(lib().ssd_prove(self.pk, self.ps, hip.p64(pub) if len(pub) else None, ctypes.c_size_t(len(pub)), hip.p8(tape), ctypes.c_size_t(tape.shape[0]),
                               ctypes.byref(used), hip.p64(words), ctypes.c_size_t(n), ms))
        return words, used.value, dict(zip(SHARDED_PHASES, list(ms)))

    def close(self):
        if self.ps:
            lib().ssd_prep_free(self.ps)
            self.ps = None
        if self.pk:
            lib().ssd_pk_free(self.pk)
            self.pk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sharded_commit(ctx: hip.Context, comm: Comm, key: hip.CommitmentKey, table: hip.Table, n_local: int, blinds_local, is_small=False):
    """PCS::commit with the rows sharded by row over the ranks (BASELINE config 4's MSM leg): this rank's rows are resident in `table`;
    returns all rows (world * rows_local, 8), rank-major."""
    rows_local = (n_local + 2047) // 2048
    blinds_local = np.ascontiguousarray(blinds_local, dtype=np.uint64).reshape(rows_local, 4)
    out = np.zeros((comm.world * rows_local, 8), dtype=np.uint64)
    _check(lib().ssd_commit(ctx.h, comm.h, key.h, table.h, ctypes.c_size_t(n_local), hip.p64(blinds_local), int(is_small), hip.p64(out)))
    return out


# ---- NeutronNovaZkSNARK (spartan2_amd/host/neutronnova_zk.cpp) ---------------------------------------------------------------------------------
NN_PHASES = ("instances", "nifs", "outer_sumcheck", "inner_sumcheck", "verifier_circuit_instance", "pcs_prove", "total", "of_which_vc_round_commits")


class NeutronNovaZkSNARK:
    """setup -> prep_prove -> prove -> verify (src/neutronnova_zk.rs:1394-2343) for step / core circuits without verifier challenges: shared + precommitted
    variables (the bench circuits, benches/sha256_neutronnova.rs) or rest variables only (the reference's test circuit, src/neutronnova_zk.rs:2357-2418; beside
    shared / precommitted ones the reference's fold drops them, refused). step_insts / core_inst: frontend.R1CSInstanceInt."""

    def __init__(self, ctx: hip.Context, step_insts, core_inst):
        self.ctx, self.steps, self.core = ctx, step_insts, core_inst
        a1, k1 = _inst_args(step_insts[0])
        a2, k2 = _inst_args(core_inst)
        self.pk = ctypes.c_void_p()
        _check(lib().nnz_setup(ctx.h, ctypes.c_size_t(len(step_insts)), *a1, *a2, ctypes.byref(self.pk)))
        info = (ctypes.c_uint64 * 8)()
        dig = np.zeros(32, dtype=np.uint8)
        lib().nnz_pk_info(self.pk, info, hip.p8(dig))
        self.info = dict(zip(("nb", "nx", "ny", "vc_rounds", "vc_vars", "vc_cons", "vc_cons_unpadded", "vc_public"), [int(x) for x in info]))
        self.vk_digest = dig
        self.ps = None
        self.batch = []  # prep_prove_batch's states
        self.batch_prep_phases = None
        self.batch_prove_phases = None
        self._sha_plan = None
        lib().nnz_proof_words.restype = ctypes.c_size_t

    @staticmethod
    def _words(steps, core):
        """(step witnesses (n, len), step publics (n, npub), core witness, core publics) as contiguous machine words"""
        sw = np.ascontiguousarray(np.stack([np.asarray(i.witness, dtype=np.uint64).reshape(-1) for i in steps]))
        sp = np.ascontiguousarray(np.stack([np.asarray(i.publics, dtype=np.uint64).reshape(-1) for i in steps]))
        return sw, sp, np.ascontiguousarray(core.witness, dtype=np.uint64), np.ascontiguousarray(core.publics, dtype=np.uint64)

    def _ensure_sha_plan(self):
        if self._sha_plan is None:
            from . import frontend

            self._sha_plan = hip.Sha256Plan(self.ctx, frontend.sha256_step_witness_plan())

    def prep_prove(self, tape: np.ndarray, is_small=True, _steps=None, _core=None, _keep=True):
        sw, sp, cw, cp = self._words(self.steps if _steps is None else _steps, self.core if _core is None else _core)
        used = ctypes.c_size_t(0)
        ps = ctypes.c_void_p()
        _check(lib().nnz_prep_prove(self.pk, ctypes.c_size_t(sw.shape[0]), hip.p64(sw), ctypes.c_size_t(sw.shape[1]), hip.p64(sp), ctypes.c_size_t(sp.shape[1]), hip.p64(cw),
                                    hip.p64(cp), int(is_small), hip.p8(tape), ctypes.c_size_t(tape.shape[0]), ctypes.byref(used), ctypes.byref(ps)))
        if not _keep:  # prep_prove_batch(one_pass=False): the state is the batch's
            return used.value, ps
        if self.ps:
            lib().nnz_prep_free(self.ps)
        self.ps = ps
        return used.value

    def prep_prove_sha256(self, blocks, tape: np.ndarray, is_small=True, _keep=True):
        """prep_prove with every step's witness and the core circuit's generated on the device in one launch (nnz_prep_prove_sha256) for a key set up from
        frontend.sha256_step_circuit instances: blocks = one 64-byte block per step; the core circuit is the zero block, every public value is x = 0."""
        blocks = [bytes(b) for b in blocks]
        assert all(len(b) == 64 for b in blocks)
        self._ensure_sha_plan()
        buf = np.frombuffer(b"".join(blocks), dtype=np.uint8).copy() if blocks else np.zeros(1, dtype=np.uint8)
        used = ctypes.c_size_t(0)
        ps = ctypes.c_void_p()
        _check(lib().nnz_prep_prove_sha256(self.pk, self._sha_plan.h, hip.p8(buf), ctypes.c_size_t(len(blocks)), int(is_small), hip.p8(tape), ctypes.c_size_t(tape.shape[0]),
                                           ctypes.byref(used), ctypes.byref(ps)))
        if not _keep:
            return used.value, ps
        if self.ps:
            lib().nnz_prep_free(self.ps)
        self.ps = ps
        return used.value

    def _free_batch(self):
        for ps in self.batch:
            lib().nnz_prep_free(ps)
        self.batch = []

    def prep_prove_batch(self, tapes, witnesses=None, blocks=None, is_small=True, one_pass=True, per_state_commit=False, per_state_layers=False, shared_commit=False,
                         shared_layers=False):
        """K = len(tapes) prep states on this one key, kept in self.batch (self.ps is left alone): from `witnesses` (witnesses[k] = (step instances, core
        instance) of this key's shapes), from `blocks` (blocks[k] = one 64-byte block per step, as prep_prove_sha256) or, with neither, the key's own
        instances K times. Returns the blocks used of each tape. State k is the state prep_prove / prep_prove_sha256 makes of input k with tape k; prove and
        check it with prove(tape, state=k) / is_sat(state=k). By default all K are prepared in one pass (nnz_prep_prove_batch_opts /
        nnz_prep_prove_sha256_batch_opts: one witness launch for SHA-256 keys, the commitments through sp_hyrax_commit_batch, every layer of every state from
        one sp_nifs_layers_batch, one synchronise); per_state_commit (NNZ_PREP_PER_STATE_COMMIT) keeps one sp_hyrax_commit per polynomial,
        per_state_layers (NNZ_PREP_PER_STATE_LAYERS) one nifs_prepare per state; shared_commit / shared_layers ask for the shared stage whatever the driver
        takes by default (measured: profiles/nn_prep_prove_batch.md); one_pass=False is a loop of the single calls. The phases of the last one-pass batch, ms: self.batch_prep_phases."""
        K = len(tapes)
        if blocks is not None and witnesses is not None:
            raise ValueError("prep_prove_batch: blocks or witnesses, not both")
        for name, v in (("blocks", blocks), ("witnesses", witnesses)):
            if v is not None and len(v) != K:
                raise ValueError(f"prep_prove_batch: {len(v)} {name} for {K} tapes")
        self._free_batch()
        tapes = [np.ascontiguousarray(t, dtype=np.uint8) for t in tapes]
        if blocks is not None:
            blocks = [[bytes(b) for b in bl] for bl in blocks]
            assert all(len(b) == 64 for bl in blocks for b in bl)
            self._ensure_sha_plan()
        srcs = None if blocks is not None else ([(self.steps, self.core)] * K if witnesses is None else list(witnesses))
        if not one_pass:
            used_all = []
            try:
                for k in range(K):
                    if blocks is not None:
                        used, ps = self.prep_prove_sha256(blocks[k], tapes[k], is_small, _keep=False)
                    else:
                        used, ps = self.prep_prove(tapes[k], is_small, _steps=srcs[k][0], _core=srcs[k][1], _keep=False)
                    self.batch.append(ps)
                    used_all.append(used)
            except Exception:
                self._free_batch()  # a failed batch leaves no state behind
                raise
            return used_all
        flags = ((NNZ_PREP_PER_STATE_COMMIT if per_state_commit else 0) | (NNZ_PREP_PER_STATE_LAYERS if per_state_layers else 0)
                 | (NNZ_PREP_SHARED_COMMIT if shared_commit else 0) | (NNZ_PREP_SHARED_LAYERS if shared_layers else 0))
        sz = ctypes.c_size_t
        A = max(K, 1)  # (ctypes arrays of at least one slot)
        tptr = (hip.c_u8p * A)(*[hip.p8(t) for t in tapes])
        tblk = (sz * A)(*[t.shape[0] for t in tapes])
        used = (sz * A)()
        pss = (ctypes.c_void_p * A)()
        ms = (ctypes.c_double * 8)()
        if blocks is not None:
            bufs = [np.frombuffer(b"".join(bl), dtype=np.uint8).copy() if bl else np.zeros(1, dtype=np.uint8) for bl in blocks]
            _check(lib().nnz_prep_prove_sha256_batch_opts(self.pk, self._sha_plan.h, sz(K), (hip.c_u8p * A)(*[hip.p8(b) for b in bufs]), (sz * A)(*[len(bl) for bl in blocks]),
                                                          int(is_small), tptr, tblk, used, pss, ms, ctypes.c_uint(flags)))
        else:
            ws = [self._words(steps, core) for steps, core in srcs]
            npub = ws[0][1].shape[1] if K else 0
            for k, w in enumerate(ws):  # (the entry point takes one width of public values for all states)
                if w[1].shape[1] != npub:
                    raise hip.SpartanHipError(f"prep_prove_batch: state {k}: InvalidWitnessLength ({w[1].shape[1]} public values a step, state 0 has {npub})")
            arr = lambda i: (hip.c_u64p * A)(*[w[i].ctypes.data_as(hip.c_u64p) for w in ws])
            _check(lib().nnz_prep_prove_batch_opts(self.pk, sz(K), (sz * A)(*[w[0].shape[0] for w in ws]), arr(0), (sz * A)(*[w[0].shape[1] for w in ws]), arr(1), sz(npub), arr(2),
                                                   arr(3), int(is_small), tptr, tblk, used, pss, ms, ctypes.c_uint(flags)))
        self.batch = [ctypes.c_void_p(pss[k]) for k in range(K)]
        self.batch_prep_phases = dict(blinds_alloc=ms[0], witness=ms[1], commit=ms[2], layers=ms[3], mirrors=ms[4], sync=ms[5], total=ms[6])
        return [int(used[k]) for k in range(K)]

    def _state(self, state):
        """the prep state a call works on: self.ps, or self.batch[state]"""
        if state is None:
            return self.ps
        if not 0 <= state < len(self.batch):
            raise hip.SpartanHipError(f"state {state} of a batch of {len(self.batch)}")
        return self.batch[state]

    def prove(self, tape: np.ndarray, reference_order=False, state=None):
        """reference_order: the one-thread driver in the statement order of src/neutronnova_zk.rs:1609-2093 (no side jobs, the opening as one sp_hyrax_prove).
        state=k proves self.batch[k] (prep_prove_batch) instead of self.ps."""
        ps = self._state(state)
        n = lib().nnz_proof_words(self.pk)
        words = np.zeros(n, dtype=np.uint64)
        used = ctypes.c_size_t(0)
        ms = (ctypes.c_double * 8)()
        fn = lib().nnz_prove_reference_order if reference_order else lib().nnz_prove
        _check(fn(self.pk, ps, hip.p8(tape), ctypes.c_size_t(tape.shape[0]), ctypes.byref(used), hip.p64(words), ctypes.c_size_t(n), ms))
        return words, used.value, dict(zip(NN_PHASES, list(ms)))

    def prove_batch(self, tapes, states=None, per_proof=None):
        """prove() for every state of self.batch (or `states`: indices into self.batch or prep-state handles, all distinct) in one call (nnz_prove_batch_opts):
        one tape per proof -> [(proof words, blocks used)], each what prove(tapes[k], state=k) returns. per_proof: True = one prove after the other
        (NNZ_BATCH_PER_PROOF), False = the batched outer and inner sum-checks of all proofs in lockstep, one launch a round for all of them
        (NNZ_BATCH_LOCKSTEP), None = the form the driver measured to be faster at this batch size (profiles/nn_prove_batch.md). A failure names the proof
        and leaves every state usable. The phases of the last batch, ms: self.batch_prove_phases."""
        states = list(range(len(self.batch))) if states is None else list(states)
        pss = [self._state(s) if isinstance(s, int) else s for s in states]
        K = len(pss)
        if len(tapes) != K:
            raise ValueError(f"prove_batch: {len(tapes)} tapes for {K} states")
        tapes = [np.ascontiguousarray(t, dtype=np.uint8) for t in tapes]
        sz = ctypes.c_size_t
        A = max(K, 1)
        n = lib().nnz_proof_words(self.pk)
        words = [np.zeros(n, dtype=np.uint64) for _ in range(K)]
        used = (sz * A)()
        ms = (ctypes.c_double * 10)()
        flags = 0 if per_proof is None else (NNZ_BATCH_PER_PROOF if per_proof else NNZ_BATCH_LOCKSTEP)
        _check(lib().nnz_prove_batch_opts(self.pk, (ctypes.c_void_p * A)(*[p.value if isinstance(p, ctypes.c_void_p) else p for p in pss]), sz(K),
                                          (hip.c_u8p * A)(*[hip.p8(t) for t in tapes]), (sz * A)(*[t.shape[0] for t in tapes]), used,
                                          (hip.c_u64p * A)(*[hip.p64(w) for w in words]), sz(n), ms, ctypes.c_uint(flags)))
        self.batch_prove_phases = dict(zip(NN_BATCH_PROVE_PHASES, list(ms)))
        return [(words[k], int(used[k])) for k in range(K)]

    def is_sat(self, state=None):
        """R1CSShape::is_sat (src/r1cs/mod.rs:358-394) of every instance the prepared state holds, on the device: a list of hip.SatReport, the step instances
        (against S_step, one batched launch), then the core instance (against S_core); bad_commitment_rows counts over an instance's [shared | precommitted]
        rows. A finding is a return value; a later prove() on the state is unaffected. state=k checks self.batch[k] instead of self.ps."""
        ps = self._state(state)
        if not ps:
            raise hip.SpartanHipError("is_sat before prep_prove")
        n = len(self.steps) + 1
        reps = (hip._SatReport * n)()
        cap = 1024
        while True:  # (instance, row) pairs; a list longer than the buffer is asked for again with room for all of it
            bad = np.zeros((cap, 2), dtype=np.uint64)
            nbad = ctypes.c_size_t(0)
            rc = lib().nnz_prep_is_sat(self.pk, ps, reps, hip.p64(bad), ctypes.c_size_t(cap), ctypes.byref(nbad))
            if rc not in (0, SP_ERR_UNSAT):
                _check(rc)
            if nbad.value <= cap:
                break
            cap = nbad.value
        pairs = bad[: nbad.value]
        return [hip.SatReport(reps[i], [int(r) for k, r in pairs if int(k) == i]) for i in range(n)]

    def verify(self, words: np.ndarray) -> int:
        """NeutronNovaZkSNARK::verify (src/neutronnova_zk.rs:2096-2343) with the commitment fold, the six matrix evaluations and the opening's MSMs on the
        device: 0 = accept, else the failed check (1 shape / encoding, 2 verifier-circuit instance, 4 relaxed Spartan proof, 5 public values, 6 opening)."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        rc = lib().nnz_verify(self.pk, hip.p64(words), ctypes.c_size_t(words.shape[0]))
        if rc < 0:
            _check(rc)
        return rc

    def proof_to_bytes(self, words: np.ndarray) -> bytes:
        """NeutronNovaZkSNARK as bincode bytes (src/neutronnova_zk.rs:1373-1385)"""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        n = ctypes.c_size_t(0)
        _check(lib().nnz_proof_to_bytes(self.pk, hip.p64(words), ctypes.c_size_t(len(words)), None, ctypes.c_size_t(0), ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        _check(lib().nnz_proof_to_bytes(self.pk, hip.p64(words), ctypes.c_size_t(len(words)), hip.p8(out), ctypes.c_size_t(n.value), ctypes.byref(n)))
        return out.tobytes()

    def _key_to_bytes(self, fn) -> bytes:
        a1, k1 = _inst_args(self.steps[0])
        a2, k2 = _inst_args(self.core)
        fn.restype = ctypes.c_long
        n = fn(self.pk, *a1, *a2, None, ctypes.c_size_t(0))
        if n < 0:
            _check(n)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        got = fn(self.pk, *a1, *a2, hip.p8(out), ctypes.c_size_t(n))
        if got < 0:
            _check(got)
        assert got == n, (got, n)
        return out[:n].tobytes()

    def vk_to_bytes(self) -> bytes:
        """The key's NeutronNovaVerifierKey { ck, vk_ee, S_step, S_core, vc_shape, vc_shape_regular, vc_ck, vc_vk } (src/neutronnova_zk.rs:1289-1303) as bincode
        bytes (nnz_vk_to_bytes): what NeutronNovaVerifier.from_bytes loads. Both circuits are handed to the library again (setup keeps no copy of them) and
        the bytes are returned only if they hash to this key's digest."""
        return self._key_to_bytes(lib().nnz_vk_to_bytes)

    def pk_to_bytes(self) -> bytes:
        """The key's NeutronNovaProverKey { ck, S_step, S_core, vk_digest, vc_shape, vc_shape_regular, vc_ck } (src/neutronnova_zk.rs:1276-1287) as bincode
        bytes (nnz_pk_to_bytes): what NeutronNovaProver.from_bytes loads."""
        return self._key_to_bytes(lib().nnz_pk_to_bytes)

    def proof_from_bytes(self, data: bytes) -> np.ndarray:
        arr = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
        lib().nnz_proof_words.restype = ctypes.c_size_t
        words = np.zeros(lib().nnz_proof_words(self.pk), dtype=np.uint64)
        _check(lib().nnz_proof_from_bytes(self.pk, hip.p8(arr), ctypes.c_size_t(len(data)), hip.p64(words), ctypes.c_size_t(len(words))))
        return words

    def verify_bytes(self, data: bytes) -> int:
        arr = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
        rc = lib().nnz_verify_bytes(self.pk, hip.p8(arr), ctypes.c_size_t(len(data)))
        if rc < 0:
            _check(rc)
        return rc

    def _verify_batch(self, fn, items, lens, keep, seed, info, per_proof):
        n = len(lens)  # (items is a ctypes array of at least one slot; keep holds the arrays it points into)
        codes = (ctypes.c_int * max(n, 1))()
        inf = VerifyBatchInfo()
        sd = None
        if seed is not None:
            sd = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
            assert sd.shape[0] == 32, "seed must be 32 bytes"
        flags = 0 if per_proof is None else (NNZ_VERIFY_BATCH_PER_PROOF if per_proof else NNZ_VERIFY_BATCH_SHARED)
        _check(fn(self.pk, items, (ctypes.c_size_t * max(n, 1))(*lens), ctypes.c_size_t(n), hip.p8(sd) if sd is not None else None, codes, ctypes.byref(inf),
                  ctypes.c_uint(flags)))
        out = [int(codes[k]) for k in range(n)]
        return (out, inf.as_dict()) if info else out

    def verify_batch(self, proofs, seed=None, info=False, per_proof=None):
        """verify() for every proof of `proofs` (flat word arrays of this key) in one pass (neutronnova_zk.cpp nn_verify_batch): the step-instance folds of
        all proofs as one sp_msm_shared_weights_grouped, the matrix evaluations of a chunk of proofs per launch, the transcript work per proof, the openings
        of all proofs as one random linear combination. -> the list of verify()'s codes; with info=True (codes, info), info = {matrix_chunks,
        opening_batched_ok, fallback_proofs, opening_proofs}. seed: 32 bytes mixed into the weights of the combined check, or None. per_proof: True = one
        verify() after the other (NNZ_VERIFY_BATCH_PER_PROOF), False = the shared form from two proofs on (NNZ_VERIFY_BATCH_SHARED), None = the form the
        driver measured to be faster at this batch size. A batch of one is verify() itself."""
        ws = [np.ascontiguousarray(w, dtype=np.uint64).reshape(-1) for w in proofs]
        n = len(ws)
        ptrs = (hip.c_u64p * max(n, 1))(*[hip.p64(w) if w.shape[0] else None for w in ws])
        return self._verify_batch(lib().nnz_verify_batch_opts, ptrs, [w.shape[0] for w in ws], ws, seed, info, per_proof)

    def verify_bytes_batch(self, blobs, seed=None, info=False, per_proof=None):
        """verify_batch() over serialised proofs (proof_to_bytes): bytes that do not decode to a proof of this key get code 1."""
        bs = [np.frombuffer(bytes(b), dtype=np.uint8).copy() if len(b) else np.zeros(1, dtype=np.uint8) for b in blobs]
        n = len(bs)
        ptrs = (hip.c_u8p * max(n, 1))(*[hip.p8(b) for b in bs])
        return self._verify_batch(lib().nnz_verify_bytes_batch_opts, ptrs, [len(b) for b in blobs], bs, seed, info, per_proof)

    def close(self):
        if self.ps:
            lib().nnz_prep_free(self.ps)
            self.ps = None
        if getattr(self, "batch", None):
            self._free_batch()
        if getattr(self, "_sha_plan", None) is not None:
            self._sha_plan.free()
            self._sha_plan = None
        if self.pk:
            lib().nnz_pk_free(self.pk)
            self.pk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- NeutronNova keys from their bytes (neutronnova_zk.cpp nn_key_from_bytes) --------------------------------------------------------------------------
NN_KEY_STAGES = ("hyrax_key", "S_step", "S_core", "vc_shapes", "ck_create", "digest", "digest_wait", "total")


class _KeyShape(hip.Shape):
    """S_step / S_core of a NeutronNova key seen through hip.Shape (compare, info, dims): the key owns the handle"""

    def __init__(self, ctx, h, dims):
        self.ctx, self.h, self.dims, self._keep = ctx, h, dims, []

    def __del__(self):
        pass


def nn_key_shapes(obj):
    """(S_step, S_core) of a NeutronNovaZkSNARK, NeutronNovaVerifier or NeutronNovaProver as hip.Shape views; they live as long as the key does"""
    L = lib()
    L.nnz_pk_shape.restype = ctypes.c_void_p
    d = (ctypes.c_uint64 * 23)()
    L.nnz_pk_dims(obj.pk, d)
    dims = [{k: int(v) for k, v in zip(DIM_NAMES, d[10 * i : 10 * i + 10])} for i in range(2)]
    return tuple(_KeyShape(obj.ctx, ctypes.c_void_p(L.nnz_pk_shape(obj.pk, i)), dims[i]) for i in range(2))


def nn_vk_digest_from_bytes(data, prover=False) -> bytes:
    """nnz_vk_digest_from_bytes: DigestHelperTrait::digest of a NeutronNovaVerifierKey from its own bincode bytes, or (prover=True) from the bytes of the
    NeutronNovaProverKey beside it (host code; no context)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    _check(lib().nnz_vk_digest_from_bytes(hip.p8(buf) if len(buf) else None, ctypes.c_size_t(len(buf)), int(bool(prover)), hip.p8(out)))
    return out.tobytes()


def _nn_key_load(self, fn, ctx, data, num_steps, flags):
    """what both loaded keys are made of: the handle, info and digest as NeutronNovaZkSNARK has them, the shapes' dimensions, the load's stages"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if data is not None else None
    self.ctx = ctx
    self.num_steps = int(num_steps)
    self.pk = ctypes.c_void_p()
    self.ps = None
    self.batch = []
    self.batch_prep_phases = None
    self.batch_prove_phases = None
    self._sha_plan = None
    _check(fn(ctx.h if ctx is not None else None, hip.p8(buf) if buf is not None and len(buf) else None, ctypes.c_size_t(len(buf) if buf is not None else 0),
              ctypes.c_size_t(self.num_steps), ctypes.c_uint(flags), ctypes.byref(self.pk)))
    st = (ctypes.c_double * 8)()
    lib().nnz_key_stages(st)
    self.load_stages = {k: float(v) for k, v in zip(NN_KEY_STAGES, st)}
    self.wire_stages = hip.wire_stages()  # of S_core's decode, the later of the two
    self.wire_full_stages = hip.wire_full_stages()
    info = (ctypes.c_uint64 * 8)()
    dig = np.zeros(32, dtype=np.uint8)
    lib().nnz_pk_info(self.pk, info, hip.p8(dig))
    self.info = dict(zip(("nb", "nx", "ny", "vc_rounds", "vc_vars", "vc_cons", "vc_cons_unpadded", "vc_public"), [int(x) for x in info]))
    self.vk_digest = dig
    d = (ctypes.c_uint64 * 23)()
    lib().nnz_pk_dims(self.pk, d)
    self.dims = {k: int(v) for k, v in zip(DIM_NAMES, d[:10])}
    self.dims_core = {k: int(v) for k, v in zip(DIM_NAMES, d[10:20])}
    lib().nnz_proof_words.restype = ctypes.c_size_t
    return self


class NeutronNovaVerifier:
    """A verifier's key loaded from the bincode bytes of NeutronNovaVerifierKey (nnz_verifier_from_bytes): no circuits, no frontend, no setup. It holds
    the two commitment keys, the row-major structures of S_step and S_core, the verifier circuit's shape and the digest - what verify reads - and verifies
    with the code NeutronNovaZkSNARK's methods run."""

    def __init__(self):
        raise TypeError("use NeutronNovaVerifier.from_bytes(ctx, data, num_steps)")

    @classmethod
    def from_bytes(cls, ctx: hip.Context, data, num_steps, device_decode=None, timed=False):
        """data: NeutronNovaZkSNARK.vk_to_bytes(). num_steps: the step count of the proofs to verify - the key fixes only ceil(log2) of it, so one key
        serves e.g. 3 and 4 steps. device_decode: True / False forces the device / host decode of the matrices, None takes the measured default. Raises on
        bytes that are not a key of that step count (short, trailing, inconsistent, not equalized, another verifier circuit ...)."""
        flags = 0 if device_decode is None else (hip.SHAPE_WIRE_DEVICE if device_decode else hip.SHAPE_WIRE_HOST)
        if timed:
            flags |= hip.SHAPE_WIRE_TIMED
        return _nn_key_load(cls.__new__(cls), lib().nnz_verifier_from_bytes, ctx, data, num_steps, flags)

    def stages(self) -> dict:
        """ms of the load by stage (NN_KEY_STAGES; host clock), and of S_core's sp_shape_from_wire under "wire" (device events when timed)"""
        return dict(self.load_stages, wire=dict(self.wire_stages))

    verify = NeutronNovaZkSNARK.verify
    verify_bytes = NeutronNovaZkSNARK.verify_bytes
    _verify_batch = NeutronNovaZkSNARK._verify_batch
    verify_batch = NeutronNovaZkSNARK.verify_batch
    verify_bytes_batch = NeutronNovaZkSNARK.verify_bytes_batch
    proof_to_bytes = NeutronNovaZkSNARK.proof_to_bytes
    proof_from_bytes = NeutronNovaZkSNARK.proof_from_bytes

    def close(self):
        if getattr(self, "pk", None):
            lib().nnz_pk_free(self.pk)
            self.pk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NeutronNovaProver:
    """A prover's key loaded from the bincode bytes of NeutronNovaProverKey (nnz_prover_from_bytes): no circuits, no frontend instances, no setup. The key
    is an ordinary prover key - both full shapes, both commitment keys, the verifier circuit's shape, the digest - and proves and verifies with the code
    NeutronNovaZkSNARK's methods run."""

    def __init__(self):
        raise TypeError("use NeutronNovaProver.from_bytes(ctx, data, num_steps)")

    @classmethod
    def from_bytes(cls, ctx: hip.Context, data, num_steps, trust_digest=False, full_device=None, timed=False):
        """data: NeutronNovaZkSNARK.pk_to_bytes(). num_steps: the step count to prove (see NeutronNovaVerifier.from_bytes). By default the digest is hashed
        from the bytes and a key whose stored digest differs is refused; trust_digest=True takes the stored one (SS_PK_TRUST_DIGEST). full_device: True /
        False forces the device / host build of the full shapes (SP_SHAPE_WIRE_FULL_DEVICE / SP_SHAPE_WIRE_FULL), None takes the measured default."""
        flags = 0 if full_device is None else (hip.SHAPE_WIRE_FULL_DEVICE if full_device else hip.SHAPE_WIRE_FULL)
        if trust_digest:
            flags |= SS_PK_TRUST_DIGEST
        if timed:
            flags |= hip.SHAPE_WIRE_TIMED
        self = _nn_key_load(cls.__new__(cls), lib().nnz_prover_from_bytes, ctx, data, num_steps, flags)
        self.steps = [None] * self.num_steps  # (is_sat counts them; the key has no instances: every prep method takes the caller's words)
        self.core = None
        return self

    stages = NeutronNovaVerifier.stages

    @staticmethod
    def _instances(step_witnesses, step_publics, core_witness, core_publics):
        if len(step_witnesses) != len(step_publics):
            raise ValueError("prep_prove: one array of public values for every step witness")
        return [_CallerInstance(w, p) for w, p in zip(step_witnesses, step_publics)], _CallerInstance(core_witness, core_publics)

    def prep_prove(self, tape: np.ndarray, step_witnesses, step_publics, core_witness, core_publics, is_small=True):
        """NeutronNovaZkSNARK.prep_prove on the caller's witness words: one array of witness words and one of public values per step, and the core's"""
        steps, core = self._instances(step_witnesses, step_publics, core_witness, core_publics)
        return NeutronNovaZkSNARK.prep_prove(self, tape, is_small, _steps=steps, _core=core)

    def prep_prove_batch(self, tapes, witnesses=None, blocks=None, is_small=True, **opts):
        """NeutronNovaZkSNARK.prep_prove_batch from `blocks`, or from `witnesses`: witnesses[k] = (step_witnesses, step_publics, core_witness, core_publics)"""
        if witnesses is not None:
            witnesses = [self._instances(*w) for w in witnesses]
        elif blocks is None:
            raise ValueError("prep_prove_batch: a key loaded from its bytes has no instances of its own (pass witnesses= or blocks=)")
        return NeutronNovaZkSNARK.prep_prove_batch(self, tapes, witnesses=witnesses, blocks=blocks, is_small=is_small, **opts)

    _words = staticmethod(NeutronNovaZkSNARK._words)
    _ensure_sha_plan = NeutronNovaZkSNARK._ensure_sha_plan
    prep_prove_sha256 = NeutronNovaZkSNARK.prep_prove_sha256
    _free_batch = NeutronNovaZkSNARK._free_batch
    _state = NeutronNovaZkSNARK._state
    prove = NeutronNovaZkSNARK.prove
    prove_batch = NeutronNovaZkSNARK.prove_batch
    is_sat = NeutronNovaZkSNARK.is_sat
    verify = NeutronNovaZkSNARK.verify
    verify_bytes = NeutronNovaZkSNARK.verify_bytes
    _verify_batch = NeutronNovaZkSNARK._verify_batch
    verify_batch = NeutronNovaZkSNARK.verify_batch
    verify_bytes_batch = NeutronNovaZkSNARK.verify_bytes_batch
    proof_to_bytes = NeutronNovaZkSNARK.proof_to_bytes
    proof_from_bytes = NeutronNovaZkSNARK.proof_from_bytes
    close = NeutronNovaZkSNARK.close
    __del__ = NeutronNovaZkSNARK.__del__
