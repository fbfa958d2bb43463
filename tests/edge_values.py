"""Edge-valued operands for the scalar-field arithmetic (spartan2_amd/csrc/field.hpp) and the tables built from them. A plain module, shared by
test_edge_values_cpu.py, test_field_host.py and test_gpu_edge_values.py; everything in it is Python integers and numpy, nothing calls the library.

Why a pool: the device product is fe_mul_wide + fe_redc_p256, whose result before the conditional subtraction is r = (T + M p) / 2^256 < 2^257. r lands
in p <= r < 2^256 - where fe_cond_sub_p_top has to subtract although nothing carried - for 2^-32 of uniform products, so uniform tables never see that
branch. redc_class() names the branch a product takes; operand_pool() is a set of structured canonical values whose pairs reach every one of them."""
import numpy as np

P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF  # T256 scalar field (FqP): the NIST P-256 prime
P_BASE = 0xFFFFFFFF0000000100000000000000017E72B42B30E7317793135661B1C4B117  # T256 base field (FpP)
R = 1 << 256
M32 = 0xFFFFFFFF
RINV = pow(R, -1, P)
NINV = (-pow(P, -1, R)) % R  # -p^-1 mod 2^256: the Montgomery quotient of T is T NINV mod 2^256

EDGE_WORDS = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
N_PAIRS = 400_000  # pairs drawn by the coverage conditions
MIN_HITS = 50


# ---- raw limbs -----------------------------------------------------------------------------------------------------------------------------------
def to_limbs32(v):
    """8 x u32 little-endian words of 0 <= v < 2^256"""
    assert 0 <= v < R
    return np.frombuffer(v.to_bytes(32, "little"), dtype="<u4").astype(np.uint32)


def from_limbs32(w):
    return int.from_bytes(np.asarray(w, dtype="<u4").tobytes(), "little")


def to_limbs64(v):
    """4 x u64 little-endian words: the layout of a table row at the C ABI"""
    assert 0 <= v < R
    return np.frombuffer(v.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def rows_to_ints(arr):
    """the raw 256-bit value of every row of an (n, 4) u64 or (n, 8) u32 array"""
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[i : i + 32], "little") for i in range(0, len(raw), 32)]


def ints_to_rows(vals):
    """(n, 4) u64 rows of raw values below 2^256"""
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def mont_mul(a, b, p=P):
    """the Montgomery product of two raw values: a b 2^-256 mod p"""
    return a * b * (RINV if p == P else pow(R, -1, p)) % p


# ---- the operand pool ----------------------------------------------------------------------------------------------------------------------------
def operand_pool(p=P, seed=1, n_words=2560, n_uniform=400):
    """Canonical raw values (Python integers below p), seeded: per-limb edge words, the neighbourhoods of 0 and p, powers of two and their negations,
    the Montgomery constants, and a few hundred uniform values."""
    rng = np.random.default_rng(seed)
    pool = []
    while len(pool) < n_words:
        pick = rng.integers(0, len(EDGE_WORDS) + 1, size=8)
        rnd = rng.integers(0, 1 << 32, size=8)
        words = [EDGE_WORDS[k] if k < len(EDGE_WORDS) else int(w) for k, w in zip(pick, rnd)]
        v = sum(w << (32 * i) for i, w in enumerate(words))
        if v < p:
            pool.append(v)
    for d in range(65):
        pool += [d, (p - d) % p]
    for k in range(256):
        pool += [1 << k, p - (1 << k)]  # 2^255 < p
    r1, r2 = R % p, R * R % p
    pool += [r1, r2, p - r1, p - r2]
    for _ in range(n_uniform):
        pool.append(int.from_bytes(rng.bytes(40), "little") % p)
    assert all(0 <= v < p for v in pool)
    return pool


def pool_pairs(n, seed=1, pool=None):
    """n seeded pairs (a, b) of pool values"""
    pool = operand_pool() if pool is None else pool
    idx = np.random.default_rng(seed + 1000).integers(0, len(pool), size=(n, 2))
    return [(pool[i], pool[j]) for i, j in idx]


def uniform_pairs(n, seed=1, p=P):
    """n seeded pairs of uniform canonical values: what ol.random_field_array gives the other tests"""
    rng = np.random.default_rng(seed + 2000)
    raw = rng.bytes(80 * n)
    vals = [int.from_bytes(raw[i : i + 40], "little") % p for i in range(0, len(raw), 40)]
    return list(zip(vals[0::2], vals[1::2]))


# ---- fe_redc_p256, restated --------------------------------------------------------------------------------------------------------------------------
def _addc(a, b, c):
    s = a + b + c
    return s & M32, s >> 32


def _subb(a, b, bw):
    d = a - b - bw
    return d & M32, 1 if d < 0 else 0


def redc_class(T):
    """The branch fe_redc_p256 takes on the 512-bit value T = a b: (k, r >= p, r >= 2^256). The quotient words m[0..7] are read from t[0..7] word by
    word as the header does, k is the signed carry of that recurrence (-1 .. 2) and r = (T + M p) / 2^256 is the value before the conditional
    subtraction. 4 carries x 3 ranges of r = 12 classes."""
    k, r = redc_parts(T)
    return k, r >= P, r >= R


def redc_parts(T):
    """(k, r) of redc_class"""
    assert 0 <= T < R * R
    t = [(T >> (32 * i)) & M32 for i in range(16)]
    m = [t[0], t[1], t[2], 0, 0, 0, 0, 0]
    c = 0
    m[3], c = _addc(t[3], m[0], c)
    m[4], c = _addc(t[4], m[1], c)
    m[5], c = _addc(t[5], m[2], c)
    x6, c = _addc(t[6], m[3], c)
    x7, c = _addc(t[7], m[4], c)
    k = c
    c = 0
    x6, c = _addc(x6, m[0], c)
    x7, c = _addc(x7, m[1], c)
    k += c
    x7, bw = _subb(x7, m[0], 0)
    k -= bw
    m[6], m[7] = x6, x7
    M = sum(w << (32 * i) for i, w in enumerate(m))
    assert (T + M * P) % R == 0, "the recurrence did not give the Montgomery quotient"
    r = (T + M * P) // R
    assert r == (T >> 256) + M - (M >> 32) + (M >> 64) + (M >> 160) + k, "the header's closed form of (T + M p) / 2^256"
    assert -1 <= k <= 2 and r < 2 * R
    return k, r


def carry_chain_pairs(seed=1, n_b=48, n_x=24):
    """Pairs (a, b) whose product REDUCES to a value next to a multiple of 2^224: X 2^224 - 1, X 2^224, X 2^224 + 1. fe_redc_p256 adds the signed carry k
    last, across all eight words; with these results the sum before it ends in seven words of zeros or ones, so k = -1 borrows, and k = 1, 2 carry, all
    the way into the top word. Pool pairs do not get there (2^-224); a is solved from the wanted result, a = v 2^256 / b mod p."""
    rng = np.random.default_rng(seed + 3000)
    pool = operand_pool()
    bs = [1, 2, R % P, P - 1] + [pool[int(i)] for i in rng.integers(0, len(pool), size=n_b)]
    bs = [b for b in bs if b]
    inv = [pow(b, -1, P) for b in bs]
    xs = [1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE] + [int(x) for x in rng.integers(1, M32, size=n_x)]
    out = []
    for x in xs:
        for d in (-1, 0, 1):
            v = (x << 224) + d
            out += [(v * R * ib % P, b) for b, ib in zip(bs, inv)]
    return out


ALL_CLASSES = [(k, ge_p, ge_r) for k in (-1, 0, 1, 2) for ge_p, ge_r in ((False, False), (True, False), (True, True))]


def in_window(a, b):
    """whether the product a b lands in p <= r < 2^256: the quotient taken as T (-p^-1) mod 2^256, no word recurrence"""
    T = a * b
    return P <= (T + (T * NINV % R) * P) >> 256 < R


# ---- the self-check transforms -------------------------------------------------------------------------------------------------------------------------
# The device evaluator cannot be mutated, and its operands and references both come from Python; so every FqP product record is evaluated a second
# time on a pair derived from it whose product is known to take the rare branch. In this order; p - 0 = p is not canonical, such pairs stay as they are.
transforms = [
    ("identity", lambda a, b: (a, b)),
    ("(p - a, b)", lambda a, b: (P - a, b)),
    ("(a, p - b)", lambda a, b: (a, P - b)),
    ("(p - a, p - b)", lambda a, b: (P - a, P - b)),
]


def pick_transform(a, b):
    """index into `transforms`: the first whose product lands in p <= r < 2^256, the identity when none does"""
    if in_window(a, b):
        return 0
    for i in range(1, len(transforms)):
        x, y = transforms[i][1](a, b)
        if x < P and y < P and in_window(x, y):
            return i
    return 0


# ---- tables --------------------------------------------------------------------------------------------------------------------------------------
def raw_max():
    """the raw limb pattern p - 1: the largest canonical representative (the Montgomery form of -2^-256)"""
    return to_limbs64(P - 1)


def mont(v):
    """Montgomery limbs (4 x u64) of the field element v"""
    return to_limbs64(v % P * R % P)


def palette(rng, n_random=10):
    """About 16 raw Montgomery elements, (n, 4) u64: 0, 1, -1, the raw patterns p - 1, (p - 1) / 2 and 2^255, and seeded uniform elements."""
    fixed = [0, R % P, (P - 1) * R % P, P - 1, (P - 1) // 2, 1 << 255]
    rnd = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(n_random)]
    return ints_to_rows(fixed + rnd)


def palette_table(rng, n, pal, weights=None):
    """an (n, 4) table whose rows are drawn from the palette (np.take: no per-element Python)"""
    w = None if weights is None else np.asarray(weights, dtype=np.float64) / np.sum(weights)
    return np.ascontiguousarray(np.take(pal, rng.choice(len(pal), size=n, p=w), axis=0))


def constant_table(n, row):
    return np.ascontiguousarray(np.tile(np.asarray(row, dtype=np.uint64).reshape(1, 4), (n, 1)))


def random_rows(rng, n):
    """n uniform canonical raw rows without per-element Python: 256 random bits, the 2^-32 of them that are >= p set to zero"""
    t = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    t[(t[:, 3] >> np.uint64(32)) == np.uint64(M32)] = 0  # top word all ones: the only rows that can reach p
    return t
