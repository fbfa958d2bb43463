"""Host side of the library's field arithmetic, without a GPU: the binary extended-GCD inversion (spartan2_amd/csrc/field.hpp fe_inv_host_xgcd, raw for public values and behind a multiplicative mask in fe_inv — every
normalisation of a point on the host and the prover's division by 1 - r_y[0] go through it) against Fermat's little theorem and x * inv(x) == 1, on
edge values and seeded random residues of both fields (tests/native/inv_check.hip, compiled here with hipcc: host code only, nothing is launched).
Further down: the 32-bit-limb arithmetic of both fields and the device's reductions on the edge-value pool of tests/edge_values.py, evaluated by
tests/native/fq_check.hip and judged here against Python integers."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

import edge_values as ev

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_host_inversion_matches_fermat(tmp_path):
    exe = str(tmp_path / "inv_check")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-o", exe, os.path.join(HERE, "native", "inv_check.hip")], check=True, capture_output=True, timeout=600)
    out = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scalar field: 20000 samples, 0 mismatches" in out.stdout and "base field: 20000 samples, 0 mismatches" in out.stdout


def _build_mul_check(tmp_path):
    exe = str(tmp_path / "mul_check")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-w", "-o", exe, os.path.join(HERE, "native", "mul_check.hip")], check=True, capture_output=True, timeout=600)
    return exe


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_product_scanning_base_field_product_on_the_host(tmp_path):
    """The base-field product the kernels use (column-wise 96-bit accumulation, field.hpp / field_fips_device.hpp) in its plain-C form and the 32-bit
    row-wise form against the 64-bit CIOS product: edge values and seeded random residues."""
    out = subprocess.run([_build_mul_check(tmp_path), "host", "50000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "host: 0 mismatches in 50000 products" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_product_scanning_base_field_product_on_the_device(tmp_path):
    """The generated asm column blocks on the device (a lone wave, then full blocks; single products and 64-deep dependent chains) against the host."""
    out = subprocess.run([_build_mul_check(tmp_path), "device", "100000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "device: 0 mismatches in 100064 lanes" in out.stdout, out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_host_keccak_permutation_forms_agree(tmp_path):
    """The unrolled host permutation (generic and BMI builds) against the loop form the device compiles, plus the Keccak-256 digests of "" and "abc"."""
    exe = str(tmp_path / "keccak_check")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-w", "-o", exe, os.path.join(HERE, "native", "keccak_check.hip")], check=True, capture_output=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "keccak: 0 mismatches" in out.stdout, out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_limb_sum_reduction_matches_modular_additions(tmp_path):
    """fe_from_limb_sums (the one reduction behind the host's limb-wise gathering of up to 64 result slots per round) against a chain of modular additions:
    1..64 random, all-ones, zero and near-p summands, both fields."""
    exe = str(tmp_path / "limb_sum_check")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-w", "-o", exe, os.path.join(HERE, "native", "limb_sum_check.hip")], check=True, capture_output=True, timeout=600)
    out = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scalar field: 20000 sums, 0 mismatches" in out.stdout and "base field: 20000 sums, 0 mismatches" in out.stdout


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_opening_host_arithmetic_matches_its_definitions(tmp_path):
    """csrc/opening_host.hpp, the host arithmetic of an announced opening, against the definitions it shortens (seeded, scalar field): folding by the
    top variable r_0 .. r_(k-1) leaves <eq(r), v> for k = 1..6; the level-by-level eq expansion, its last level formed as (P[i] - P[i] r, P[i] r), gives
    the eq table; the tensor partial sums closed by <right, T> equal <eq(point), d> for 0, 1 and 5 column variables (hb = 0 included)."""
    exe = str(tmp_path / "opening_fold_check")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-w", "-o", exe, os.path.join(HERE, "native", "opening_fold_check.hip")], check=True, capture_output=True, timeout=600)
    out = subprocess.run([exe, "20"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    for what in ("fold_top", "eq_expand", "tensor"):
        assert f"{what}: 20 trials, 0 mismatches" in out.stdout


# ---- the scalar field's 32-bit-limb arithmetic and the device reductions on edge values (tests/native/fq_check.hip) ---------------------------------
# fq_check only evaluates: it reads records (op, a[8], b[8]) and writes one result per record. Every result is judged here against Python integers.
OPS ={name: i + 1 for i, name in enumerate(
    ["MUL_FQ", "MUL_FP", "CHAIN_FQ", "ADD_FQ", "SUB_FQ", "NEG_FQ", "DBL_FQ", "ADD_FP", "SUB_FP", "NEG_FP", "DBL_FP", "UNIFORM_FQ", "LAZY_REDUCE",
     "LAZY_WAVE", "WAVE_SUM_64", "WAVE_SUM_128", "WAVE_SUM_256", "BLOCK_SUM_64", "BLOCK_SUM_128", "BLOCK_SUM_256"])}
OP_NAMES = {v: k for k, v in OPS.items()}
REC = np.dtype([("op", "<u4"), ("a", "<u4", 8), ("b", "<u4", 8)])
LONE = 4096  # records the lone wave of `fq_check device` walks
RINV_BASE = pow(ev.R, -1, ev.P_BASE)


def _chain(a, b):
    c = a
    for k in range(64):
        c = c * (b if k & 1 else c) * ev.RINV % ev.P
    return c


def _elementwise_reference(op, a, b):
    """the result of one element-wise record, in Python integers on the raw values"""
    name = OP_NAMES[op]
    p = ev.P_BASE if name.endswith("_FP") else ev.P
    if name == "MUL_FQ":
        return a * b * ev.RINV % p
    if name == "MUL_FP":
        return a * b * RINV_BASE % p
    if name == "CHAIN_FQ":
        return _chain(a, b)
    if name == "UNIFORM_FQ":  # the 64 bytes a || b, little-endian, as a field element in Montgomery form
        return (a + (b << 256)) % p * ev.R % p
    if name == "LAZY_REDUCE":  # the 9-word value a + b[0] 2^256
        return (a + ((b & ev.M32) << 256)) % p
    return {"ADD": (a + b) % p, "SUB": (a - b) % p, "NEG": (-a) % p, "DBL": 2 * a % p}[name[:3]]


def _reference(recs):
    """expected results of a whole record list [(op, a, b)]: element-wise records one by one, per-wave and per-block records by their groups"""
    want = [0] * len(recs)
    i = 0
    while i < len(recs):
        op = recs[i][0]
        name = OP_NAMES[op]
        if name == "LAZY_WAVE" or name.startswith("WAVE_SUM"):
            s = sum(a for _, a, _ in recs[i : i + 64]) % ev.P
            assert all(o == op for o, _, _ in recs[i : i + 64])
            want[i : i + 64] = [s] * 64
            i += 64
        elif name.startswith("BLOCK_SUM"):
            T = int(name.rsplit("_", 1)[1])
            grp = recs[i : i + T]
            assert len(grp) == T and all(o == op for o, _, _ in grp)
            want[i : i + 3] = [sum(a for _, a, _ in grp) % ev.P, sum(b for _, _, b in grp) % ev.P, sum((a - b) % ev.P for _, a, b in grp) % ev.P]
            i += T
        else:
            want[i] = _elementwise_reference(*recs[i])
            i += 1
    return want


def _run_fq_check(exe, mode, recs, tmp_path):
    arr = np.zeros(len(recs), dtype=REC)
    arr["op"] = [r[0] for r in recs]
    arr["a"] = np.frombuffer(b"".join(r[1].to_bytes(32, "little") for r in recs), dtype="<u4").reshape(-1, 8)
    arr["b"] = np.frombuffer(b"".join(r[2].to_bytes(32, "little") for r in recs), dtype="<u4").reshape(-1, 8)
    fin, fout = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    arr.tofile(fin)
    out = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and f"{mode}: {len(recs)} records" in out.stdout, out.stdout + out.stderr
    with open(fout, "rb") as f:
        raw = f.read()
    os.remove(fin)
    os.remove(fout)
    n_extra = min(len(recs), LONE) if mode == "device" else 0
    assert len(raw) == 32 * (len(recs) + n_extra)
    vals = [int.from_bytes(raw[i : i + 32], "little") for i in range(0, len(raw), 32)]
    return vals[: len(recs)], vals[len(recs) :]


def _judge(recs, got, want, what):
    """bit-exact, and the first difference named with its operands and, for a scalar-field product, the branch of the reduction it takes"""
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    if bad:
        op, a, b = recs[bad[0]]
        cls = f", redc_class {ev.redc_class(a * b)}" if OP_NAMES[op] == "MUL_FQ" else ""
        kinds = collections.Counter(OP_NAMES[recs[i][0]] for i in bad)
        pytest.fail(f"{what}: {len(bad)} of {len(got)} results differ {dict(kinds)}; first at record {bad[0]}: {OP_NAMES[op]} a={a:#066x} b={b:#066x}{cls}: "
                    f"got {got[bad[0]]:#066x}, want {want[bad[0]]:#066x}")


def _complements(pool, p):
    """pairs around a + b = p and a - b = 0: where fe_add's conditional subtraction and fe_sub's add-back change sides"""
    out = []
    for v in pool:
        out += [(v, (p - v) % p), (v, v), (v, (p - v + 1) % p), (v, (p - v - 1) % p), (v, (v + 1) % p), (v, 0), (0, v)]
    return out


@pytest.fixture(scope="module")
def fq_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fq_check") / "fq_check")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-w", "-o", exe, os.path.join(HERE, "native", "fq_check.hip")], check=True, capture_output=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def shared_records():
    return _shared_records()


def _shared_records():
    """(head, rest): the records both modes evaluate. Scalar-field products: the N_PAIRS pool pairs of the coverage conditions (test_edge_values_cpu.py) and, behind
    each pair that takes a non-identity transform, the transformed pair - a product known to land in p <= r < 2^256, where the conditional subtraction
    must subtract although nothing carried. Base-field products, and add / sub / neg / dbl of both fields, on pool pairs and on the pairs around
    a + b = p and a = b. `head` is the part the device's lone wave walks too: it starts with the window products."""
    pool, base = ev.operand_pool(), ev.operand_pool(ev.P_BASE)
    pairs = ev.pool_pairs(ev.N_PAIRS, pool=pool)
    window, products = [], []
    for a, b in pairs:
        products.append((OPS["MUL_FQ"], a, b))
        i = ev.pick_transform(a, b)
        if i:
            x, y = ev.transforms[i][1](a, b)
            products.append((OPS["MUL_FQ"], x, y))
            if len(window) < 1500:
                window.append((OPS["MUL_FQ"], x, y))
    assert len(window) == 1500
    head = list(window)
    for a, b in ev.carry_chain_pairs():  # the signed carry k added across seven words of zeros or ones
        products.append((OPS["MUL_FQ"], a, b))
        k, r = ev.redc_parts(a * b)
        if k and (r - k + (k > 0)) % (1 << 224) == 0 and len(head) < 1800:  # the sum before k ends in zeros (k < 0) or ones (k > 0)
            head.append((OPS["MUL_FQ"], a, b))
    rest = []
    for fld, pl, p in (("FQ", pool, ev.P), ("FP", base, ev.P_BASE)):
        pp = ev.pool_pairs(20000, seed=11, pool=pl)
        comp = _complements(pl, p)
        near = _complements([d for d in range(10)] + [p - d for d in range(1, 11)], p)
        for name in ("ADD", "SUB", "NEG", "DBL"):
            op = OPS[f"{name}_{fld}"]
            head += [(op, a, b) for a, b in near]
            rest +=[(op, a, b) for a, b in comp] + [(op, a, b) for a, b in pp]
    bp = ev.pool_pairs(20000, seed=12, pool=base)
    head += [(OPS["MUL_FP"], a, b) for a, b in bp[:500]]
    rest += [(OPS["MUL_FP"], a, b) for a, b in bp[500:]] + [(OPS["MUL_FP"], a, b) for a, b in _complements(base[2560:3206], ev.P_BASE)]
    return head, products + rest


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_limb32_field_arithmetic_on_edge_values_on_the_host(fq_check_exe, shared_records, tmp_path):
    """fe_mul_limb32 (fe_mul_wide + fe_redc_p256 for the scalar field, the word-serial reduction for the base field), fe_add, fe_sub, fe_neg and fe_dbl as
    the host compiles them, against Python integers (a b 2^-256 mod p for products) on the edge-value pool: all twelve branches of the reduction."""
    head, rest = shared_records
    recs = head + rest
    got, _ = _run_fq_check(fq_check_exe, "host", recs, tmp_path)
    _judge(recs, got, _reference(recs), "fq_check host")


def _device_only_records():
    """(head, rest) of the ops only the device mode has"""
    rng = np.random.default_rng(0xF9)
    pool = ev.operand_pool()
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % ev.P  # noqa: E731
    chain = [(OPS["CHAIN_FQ"], a, b) for a, b in ev.pool_pairs(2048, seed=13, pool=pool)]
    full = ev.R - 1
    uni = [(full, full), (0, 0), (1, 0), (0, 1)]
    for v in (ev.P - 1, ev.P, ev.R - 1):
        uni += [(v, 0), (0, v), (v, v)]
    uni += [(v, w) for v in (ev.P - 1, ev.P, ev.P + 1, ev.R - 1) for w in (ev.P - 1, ev.P, ev.P + 1, ev.R - 1)]
    uni += [(int.from_bytes(rng.bytes(32), "little"), int.from_bytes(rng.bytes(32), "little")) for _ in range(2000)]
    uniform = [(OPS["UNIFORM_FQ"], lo, hi) for lo, hi in uni]
    lazy = []
    for x in (ev.P - 1, rnd(), rnd(), 1, (ev.P - 1) // 2):
        for n in (0, 1, 2, 1 << 16, 1 << 31, (1 << 32) - 1, 1 << 32):  # at most 2^32 canonical summands: the stated contract of lazy9_t
            v = n * x
            assert v < 1 << 288
            lazy.append((OPS["LAZY_REDUCE"], v & (ev.R - 1), v >> 256))
    head = chain[:256] + uniform[:64] + lazy
    # lists for the wave and block sums: all p - 1 (the largest sum), all zero, one non-zero lane at either end, pool values, uniform values
    def lists(T, k):
        out = [[ev.P - 1] * T, [0] * T, [ev.P - 1] + [0] * (T - 1), [0] * (T - 1) + [ev.P - 1], [(ev.P - 1) // 2 + (i & 1) for i in range(T)]]
        out += [[pool[int(j)] for j in rng.integers(0, len(pool), size=T)] for _ in range(k)]
        out += [[rnd() for _ in range(T)] for _ in range(k)]
        return out
    grouped = []
    for name, T in (("LAZY_WAVE", 64), ("WAVE_SUM_64", 64), ("WAVE_SUM_128", 128), ("WAVE_SUM_256", 256), ("BLOCK_SUM_64", 64), ("BLOCK_SUM_128", 128), ("BLOCK_SUM_256", 256)):
        for la, lb in zip(lists(T, 8), reversed(lists(T, 8))):
            grouped += [(OPS[name], a, b) for a, b in zip(la, lb)]
    return head, chain[256:] + uniform[64:] + grouped


@pytest.mark.gpu
def test_field_arithmetic_and_reductions_on_edge_values_on_the_device(fq_check_exe, shared_records, tmp_path):
    """On the device, a lone wave first and full 256-thread blocks after it: fe_mul<FqP> (single products and 64-deep dependent chains),
    fe_mul_rowwise<FpP>, add / sub / neg / dbl of both fields, fe_from_uniform<FqP> on 64-byte inputs up to all-ones, and the reductions of
    device_utils.hpp - lazy_from / lazy_wave_sum / lazy_reduce on lists of 64 values, lazy_reduce on crafted 9-word values n (p - 1) and n x up to
    n = 2^32, wave_sum and block_sum<3> at 64, 128 and 256 threads. References: Python integers (int.from_bytes(...) % p, the integer sum mod p)."""
    head, rest = shared_records
    dhead, drest = _device_only_records()
    recs = head + dhead + rest + drest
    assert len(head) + len(dhead) <= LONE
    want = _reference(recs)
    got, lone = _run_fq_check(fq_check_exe, "device", recs, tmp_path)
    _judge(recs, got, want, "fq_check device, full blocks")
    grouped = [OP_NAMES[op].startswith(("LAZY_WAVE", "WAVE_SUM", "BLOCK_SUM")) for op, _, _ in recs[:LONE]]
    _judge(recs[:LONE], lone, [0 if g else w for g, w in zip(grouped, want[:LONE])], "fq_check device, lone wave")
