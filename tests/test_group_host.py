"""The point-addition routines of spartan2_amd/csrc/curve.hpp (xyzz_add, xyzz_add_mixed, xyzz_dbl, jac_add, jac_add_mixed, jac_dbl) and the
block-cooperative xyzz_add_block4 of coop_add.hpp at their exceptional exits - an identity operand, P = Q, P = -Q - evaluated by
tests/native/group_check.hip (host build: no GPU; device build: one gpu test) and judged here: every result is normalised in Python integers and
compared with (a + b) H, the oracle's fixed-base multiple of the integer sum of the operands' discrete logs.

Operands come normalised (ZZ = ZZZ = 1) and RESCALED by lambda (X lambda^2, Y lambda^3, ZZ lambda^2, ZZZ lambda^3; Jacobian Z = lambda): the equality test
pd == 0 && rd == 0 then runs on unequal representatives of equal points, and a doubling that mixes up ZZ and ZZZ shows. lambda is drawn from the
edge-value pool of tests/edge_values.py (raw limb patterns of the base field), so the products inside the tests land in the reduction's rare windows."""
import collections
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import edge_values as ev
import oracle_lib as ol
from oracle_lib import lib as olib, p64

HERE = os.path.dirname(os.path.abspath(__file__))
N, Q = ol.MODULI[0], ol.MODULI[1]  # group order, base field
R = 1 << 256
RINV_Q = pow(R, -1, Q)
OPS = {name: i + 1 for i, name in enumerate(["XYZZ_ADD", "XYZZ_ADD_MIXED", "XYZZ_DBL", "JAC_ADD", "JAC_ADD_MIXED", "JAC_DBL", "BLOCK4"])}
OP_NAMES = {v: k for k, v in OPS.items()}
INACTIVE = 0x80000000
REC = np.dtype([("op", "<u4"), ("p", "<u4", 32), ("q", "<u4", 32)])


class Points:
    """affine coordinates (Python integers, standard form; None = identity) of a H for the dlogs asked for, from ONE oracle call per batch"""

    def __init__(self):
        self.H = np.zeros((1, 8), dtype=np.uint64)
        olib().orc_from_label(b"group_check", ctypes.c_size_t(1), p64(self.H))
        self.known = {0: None}

    def need(self, dlogs):
        new = sorted({d % N for d in dlogs} - set(self.known))
        if not new:
            return
        out = np.zeros((len(new), 8), dtype=np.uint64)
        olib().orc_fixed_base_mul(p64(np.ascontiguousarray(self.H[0])), p64(ol.mont_array(new)), ctypes.c_size_t(len(new)), p64(out))
        for d, row in zip(new, out):
            self.known[d] = (ol.from_mont(row[:4], 1), ol.from_mont(row[4:], 1))

    def __getitem__(self, d):
        return self.known[d % N]


def _words(vals):
    """standard-form base-field values -> their Montgomery limbs, 8 u32 words each, concatenated"""
    return b"".join((v % Q * R % Q).to_bytes(32, "little") for v in vals)


def xyzz_of(pt, lam=1, garbage=0):
    if pt is None:
        return (garbage, garbage, 0, 0)
    l2, l3 = lam * lam % Q, lam * lam * lam % Q
    return (pt[0] * l2, pt[1] * l3, l2, l3)


def jac_of(pt, lam=1, garbage=1):
    if pt is None:
        return (garbage, garbage, 0, 0)  # jac_identity() is (1, 1, 0); only z is tested
    return (pt[0] * lam * lam, pt[1] * lam * lam * lam, lam, 0)


def aff_of(pt):
    return (0, 0, 0, 0) if pt is None else (pt[0], pt[1], 0, 0)


def build_records(pts, specs):
    """specs: (op name, a, b, lam, mu, active) -> (records array, expected list). The second operand of a mixed op is affine (mu ignored), a doubling
    has none. expected: ("point", affine or None) or ("raw", words) for an item of xyzz_add_block4 that does not take part."""
    arr = np.zeros(len(specs), dtype=REC)
    pw, qw, want = [], [], []
    for name, a, b, lam, mu, active in specs:
        jac = name.startswith("JAC")
        rep = jac_of if jac else xyzz_of
        p = rep(pts[a], lam)
        if name.endswith("DBL"):
            q, total = (0, 0, 0, 0), 2 * a
        else:
            q, total = (aff_of(pts[b]) if name.endswith("MIXED") else rep(pts[b], mu)), a + b
        pw.append(_words(p))
        qw.append(_words(q))
        want.append(("point", pts[total]) if active else ("raw", pw[-1]))
    arr["op"] = [OPS[sp[0]] | (0 if sp[5] else INACTIVE) for sp in specs]
    arr["p"] = np.frombuffer(b"".join(pw), dtype="<u4").reshape(-1, 32)
    arr["q"] = np.frombuffer(b"".join(qw), dtype="<u4").reshape(-1, 32)
    return arr, want


def run_group_check(exe, mode, arr, tmp_path):
    fin, fout = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    arr.tofile(fin)
    out = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and f"{mode}: {len(arr)} records" in out.stdout, out.stdout + out.stderr
    with open(fout, "rb") as f:
        raw = f.read()
    os.remove(fin)
    os.remove(fout)
    assert len(raw) == 128 * len(arr)
    return raw


def normalise(name, raw):
    """(affine point or None, well-formed) of one 128-byte result: x = X / ZZ, y = Y / ZZZ with ZZ^3 = ZZZ^2 for the xyzz ops, x = X / Z^2, y = Y / Z^3 for
    the Jacobian ones; all in standard form"""
    c = [int.from_bytes(raw[32 * i : 32 * i + 32], "little") for i in range(4)]
    if any(v >= Q for v in c):
        return None, False
    x, y, z, w = [v * RINV_Q % Q for v in c]
    if name.startswith("JAC"):
        if z == 0:
            return None, True
        zi = pow(z, -1, Q)
        return (x * zi * zi % Q, y * zi * zi * zi % Q), True
    if z == 0:
        return None, w == 0
    if w == 0:
        return None, False
    return (x * pow(z, -1, Q) % Q, y * pow(w, -1, Q) % Q), pow(z, 3, Q) == w * w % Q


def mismatches(specs, want, raw):
    """indices of the records whose result is not the expected point (or, for an idle item, not its untouched first operand)"""
    bad = []
    for i, (sp, (kind, exp)) in enumerate(zip(specs, want)):
        res = raw[128 * i : 128 * i + 128]
        if kind == "raw":
            ok = res == exp
        else:
            got, well = normalise(sp[0], res)
            ok = well and got == exp
        if not ok:
            bad.append(i)
    return bad


def judge(specs, want, raw, what):
    bad = mismatches(specs, want, raw)
    if bad:
        import group_edges as ge
        name, a, b, lam, mu, active = specs[bad[0]]
        kinds = collections.Counter((specs[i][0], "dbl" if specs[i][0].endswith("DBL") else ge.classify(specs[i][1], specs[i][2])) for i in bad)
        pytest.fail(f"{what}: {len(bad)} of {len(specs)} results differ {dict(kinds)}; first at record {bad[0]}: {name} a={a:#x} b={b:#x} lambda={lam:#x} mu={mu:#x} "
                    f"active={active}")


# ---- the pairs -----------------------------------------------------------------------------------------------------------------------------------
def crafted_pairs():
    """(a, b) dlog pairs of all five classes: identities on either side and on both, P + P, P - P, neighbours of both, small and large multiples"""
    rng = np.random.default_rng(0x6E0)
    u = [int.from_bytes(rng.bytes(40), "little") % (N - 1) + 1 for _ in range(6)]
    base = u + [1, 2, 3, N - 1, N - 2, (N - 1) // 2, (N + 1) // 2]
    pairs = [(0, 0)]
    for a in base:
        pairs += [(0, a), (a, 0), (a, a), (a, N - a), (a, a + 1), (a, N - a + 1), (a, 2 * a % N)]
    pairs += [(u[0], u[1]), (u[2], u[3]), (u[4], u[5]), (1, N - 2), ((N - 1) // 2, (N - 1) // 2), ((N - 1) // 2, (N + 1) // 2)]
    return pairs


def uniform_pairs(n, seed=0x6E1):
    rng = np.random.default_rng(seed)
    v = [int.from_bytes(rng.bytes(40), "little") % N for _ in range(2 * n)]
    return list(zip(v[0::2], v[1::2]))


def lambdas(n, seed):
    """n scaling factors in standard form whose MONTGOMERY limbs are values of the edge pool (a Jacobian Z is then exactly the pool's limb pattern)"""
    pool = [v for v in ev.operand_pool(ev.P_BASE) if v]
    idx = np.random.default_rng(seed).integers(0, len(pool), size=n)
    return [pool[int(i)] * RINV_Q % Q for i in idx]


LANE_OPS = ["XYZZ_ADD", "XYZZ_ADD_MIXED", "XYZZ_DBL", "JAC_ADD", "JAC_ADD_MIXED", "JAC_DBL"]


def specs_for(pairs, ops, per_pair=3, seed=1):
    """every pair through every op: once normalised, once with only one side rescaled, and `per_pair` times with both sides rescaled by pool values"""
    lam = lambdas(2 * per_pair * len(pairs) * len(ops) + 2, seed)
    out, it = [], iter(lam)
    for op in ops:
        for a, b in pairs:
            out.append((op, a, b, 1, 1, True))
            out.append((op, a, b, next(it), 1, True))
            out.append((op, a, b, 1, next(it), True))
            for _ in range(per_pair - 1):
                out.append((op, a, b, next(it), next(it), True))
    return out


def pool_sweep(ops, seed=3):
    """P + P, P - P and P + Q with lambda = EVERY non-zero value of the edge pool on the first operand and a pool value on the second"""
    pool = [v * RINV_Q % Q for v in ev.operand_pool(ev.P_BASE) if v]
    rng = np.random.default_rng(seed)
    u = [int.from_bytes(rng.bytes(40), "little") % (N - 1) + 1 for _ in range(2)]
    out = []
    for i, lam in enumerate(pool):
        mu = pool[int(rng.integers(0, len(pool)))]
        b = (u[0], N - u[0], u[1])[i % 3]
        out += [(op, u[0], b, lam, mu, True) for op in ops]
    return out


def points_for(specs):
    pts = Points()
    need = set()
    for name, a, b, *_ in specs:
        need |= {a, b, a + b, 2 * a}
    pts.need(need)
    return pts


@pytest.fixture(scope="module")
def group_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("group_check") / "group_check")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-w", "-o", exe, os.path.join(HERE, "native", "group_check.hip")], check=True, capture_output=True, timeout=900)
    return exe


def lane_specs():
    return specs_for(crafted_pairs(), LANE_OPS) + pool_sweep(["XYZZ_ADD", "XYZZ_ADD_MIXED", "JAC_ADD", "JAC_ADD_MIXED"]) + specs_for(uniform_pairs(200), LANE_OPS, per_pair=1, seed=2)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_addition_routines_at_their_exceptional_exits_on_the_host(group_check_exe, tmp_path):
    """xyzz_add, xyzz_add_mixed, xyzz_dbl, jac_add, jac_add_mixed, jac_dbl as the host compiles them: all five classes of operand pairs, normalised and
    rescaled representatives, the whole edge pool as scaling factors, and uniform pairs; every result normalised and compared with (a + b) H."""
    specs = lane_specs()
    arr, want = build_records(points_for(specs), specs)
    judge(specs, want, run_group_check(group_check_exe, "host", arr, tmp_path), "group_check host")


def block4_specs():
    """blocks of 64 items for xyzz_add_block4<64>: exceptional items between generic ones, whole blocks of one class, and items that do not take part
    (their slots hold operands of every class: the full-EXEC products run on them, the result must stay the first operand)"""
    rng = np.random.default_rng(0x6E2)
    pairs = crafted_pairs()
    generic = uniform_pairs(64, 0x6E3)
    lam = iter(lambdas(40000, 5))
    specs = []

    def block(items):
        assert len(items) == 64
        for (a, b), active in items:
            norm = rng.integers(0, 4) == 0
            specs.append(("BLOCK4", a, b, 1 if norm else next(lam), 1 if norm else next(lam), active))

    for lo in range(0, len(pairs), 16):  # 16 crafted pairs spread over a block of generic ones, taking part and idle
        chunk = pairs[lo : lo + 16]
        for idle in (False, True):
            items = [(g, True) for g in generic]
            for j, pr in enumerate(chunk):
                items[(5 * j + 3) % 64] = (pr, not (idle and j % 2))
            block(items)
    for cls_pairs in ([(a, a) for a, _ in generic], [(a, N - a) for a, _ in generic], [(0, b) for _, b in generic], [(a, 0) for a, _ in generic], [(0, 0)] * 64):
        block([(pr, True) for pr in cls_pairs])
        block([(pr, j % 3 != 0) for j, pr in enumerate(cls_pairs)])
    block([(pr, False) for pr in generic])  # a block none of whose items takes part: the products are skipped
    sweep = pool_sweep(["BLOCK4"])
    sweep = sweep[: len(sweep) // 64 * 64]
    return specs + sweep


@pytest.mark.gpu
def test_addition_routines_and_the_cooperative_addition_on_the_device(group_check_exe, tmp_path):
    """The same records on the device in 256-thread blocks, and xyzz_add_block4<64> as one block per 64 items: the flag / fix pair written in stages 1
    and 3 and consumed after the last barrier, with exceptional, generic and idle items side by side in one wave."""
    specs = lane_specs() + block4_specs()
    arr, want = build_records(points_for(specs), specs)
    judge(specs, want, run_group_check(group_check_exe, "device", arr, tmp_path), "group_check device")
