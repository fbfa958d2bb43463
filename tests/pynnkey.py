"""NeutronNovaVerifierKey / NeutronNovaProverKey (src/neutronnova_zk.rs:1276-1303) as bincode bytes, written in Python from the integer circuits, and the
key's digest recomputed from those bytes. No product code and no oracle: pywire (Writer, pad_shape, equalize) for the framing and the equalized shapes,
pyvcircuit (its synthesis of the verifier circuit, multiround_shape, multiround_shape_bytes, regular_shape_bytes) for the two verifier-circuit shapes.

Derived field order, little-endian, fixint:
  verifier: ck, vk_ee, S_step, S_core, vc_shape, vc_shape_regular, vc_ck, vc_vk      (`digest` is #[serde(skip)])
  prover:   ck, S_step, S_core, vk_digest ([u8; 32]: no length), vc_shape, vc_shape_regular, vc_ck
For Hyrax a verifier key serialises as its commitment key does. gens: the (>= 2049, 8) generator limbs of label "ck" - PCS::setup(b"ck", ., 2048) for ck /
vk_ee, PCS::setup(b"ck", ., 32) for vc_ck / vc_vk: the same label, a shorter prefix, h right after it (src/r1cs/mod.rs:1690-1693)."""
import hashlib
import struct

import numpy as np

import pyvcircuit
import pywire

DIM_ORDER = ("num_cons", "num_cons_unpadded", "num_shared_unpadded", "num_precommitted_unpadded", "num_rest_unpadded", "num_shared", "num_precommitted",
             "num_rest", "num_public", "num_challenges")  # field order of SplitR1CSShape (src/r1cs/mod.rs:743-755)


def shape_bytes(shape):
    """the derived Serialize of SplitR1CSShape (src/r1cs/mod.rs:742-773) for a (dims, mats, num_cols) of pywire.pad_shape / equalize; SparseMatrix
    { data, indices, indptr, cols } (src/r1cs/sparse.rs:383-394)"""
    dims, mats, num_cols = shape
    w = pywire.Writer()
    for k in DIM_ORDER:
        w.u64(dims[k])
    lut = {}
    for data, cols, ptr in mats:
        w.u64(len(data))
        for v in data:
            v = int(v)
            if v not in lut:
                lut[v] = (v % pywire.P_SCALAR).to_bytes(32, "little")
            w.parts.append(lut[v])
        w.u64(len(cols))
        w.parts.append(np.asarray(cols, dtype="<u8").tobytes())
        w.u64(len(ptr))
        w.parts.append(np.asarray(ptr, dtype="<u8").tobytes())
        w.u64(num_cols)
    return w.bytes()


def hyrax_key_bytes(gens, width):
    w = pywire.Writer()
    w.hyrax_key(gens[:width], gens[width])
    return w.bytes()


def fields(step_inst, core_inst, num_steps, gens):
    """the fields both keys are made of, by name, as bytes"""
    S_step, S_core = pywire.equalize(pywire.pad_shape(step_inst), pywire.pad_shape(core_inst))
    d = S_step[0]
    nv = d["num_shared"] + d["num_precommitted"] + d["num_rest"]
    nb = max(0, (num_steps - 1).bit_length())
    sh = pyvcircuit.multiround_shape(pyvcircuit.VerifierCircuit(nb, d["num_cons"].bit_length() - 1, nv.bit_length(), 32))
    return dict(ck=hyrax_key_bytes(gens, pywire.WIDTH), S_step=shape_bytes(S_step), S_core=shape_bytes(S_core), vc_shape=pyvcircuit.multiround_shape_bytes(sh),
                vc_shape_regular=pyvcircuit.regular_shape_bytes(sh), vc_ck=hyrax_key_bytes(gens, 32))


VK_FIELDS = ("ck", "vk_ee", "S_step", "S_core", "vc_shape", "vc_shape_regular", "vc_ck", "vc_vk")
PK_FIELDS = ("ck", "S_step", "S_core", "vk_digest", "vc_shape", "vc_shape_regular", "vc_ck")


def vk_fields(step_inst, core_inst, num_steps, gens):
    f = fields(step_inst, core_inst, num_steps, gens)
    f["vk_ee"], f["vc_vk"] = f["ck"], f["vc_ck"]
    return [(k, f[k]) for k in VK_FIELDS]


def vk_bytes(step_inst, core_inst, num_steps, gens):
    return b"".join(b for _, b in vk_fields(step_inst, core_inst, num_steps, gens))


def pk_fields(step_inst, core_inst, num_steps, gens, digest=None):
    f = fields(step_inst, core_inst, num_steps, gens)
    f["vk_digest"] = bytes(digest) if digest is not None else digest_from_bytes(vk_bytes(step_inst, core_inst, num_steps, gens))
    assert len(f["vk_digest"]) == 32
    return [(k, f[k]) for k in PK_FIELDS]


def pk_bytes(step_inst, core_inst, num_steps, gens, digest=None):
    return b"".join(b for _, b in pk_fields(step_inst, core_inst, num_steps, gens, digest))


def offsets(named_fields):
    """{name: offset of its first byte}, plus "end" """
    out, at = {}, 0
    for k, b in named_fields:
        out[k] = at
        at += len(b)
    out["end"] = at
    return out


class _Walk:
    def __init__(self, data):
        self.b, self.o = memoryview(bytes(data)), 0

    def u64(self):
        assert self.o + 8 <= len(self.b), "unexpected end of input"
        v = struct.unpack_from("<Q", self.b, self.o)[0]
        self.o += 8
        return v

    def take(self, n):
        assert self.o + n <= len(self.b), "unexpected end of input"
        out = self.b[self.o:self.o + n]
        self.o += n
        return out


def digest_from_bytes(vk):
    """SHA-256 over NeutronNovaVerifierKey::write_bytes (src/neutronnova_zk.rs:1305-1333) from the key's serde bytes, as the loader walks them: bincode(ck)
    and bincode(vk_ee) as they stand; each shape in digest form - SplitR1CSShape::write_bytes (src/r1cs/mod.rs:775-794) is the ten dimensions, then per matrix
    write_digest_bytes (src/r1cs/sparse.rs:398-417): the three lengths and cols, then the data, indices and indptr bytes of the serde form unchanged; the
    last four fields as they stand."""
    r = _Walk(vk)
    h = hashlib.sha256()
    for _ in range(2):  # ck, vk_ee: num_cols, Vec<Affine>, GE
        r.u64()
        r.take(64 * r.u64() + 96)
    h.update(r.b[:r.o])
    for _ in range(2):  # S_step, S_core
        h.update(r.take(80))
        for _m in range(3):
            nd = r.u64()
            data = r.take(32 * nd)
            ni = r.u64()
            idx = r.take(8 * ni)
            nptr = r.u64()
            ptr = r.take(8 * nptr)
            h.update(struct.pack("<QQQQ", nd, ni, nptr, r.u64()))
            h.update(data)
            h.update(idx)
            h.update(ptr)
    h.update(r.b[r.o:])
    return h.digest()
