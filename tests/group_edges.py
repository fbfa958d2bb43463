"""Point additions with KNOWN discrete logs: every base is k_i H, so every intermediate point of every kernel is a H with a an integer mod the group
order N, and an addition a H + b H can be classified on integers - identity operand, P + P, P - P, generic - and steered into a chosen tree level.
A plain module shared by test_group_edges_cpu.py and test_gpu_group_edges.py; everything in it is Python integers, nothing calls the library or the
oracle.

  classify(a, b)            the exit an addition routine takes on a H + b H
  byte digits / signed digits   the window digits the kernels read (kernels_msm.hpp signed_digit, k_fold_sign)
  replay_*                  one kernel's addition order re-run on integers: Counter[(stage, class)] and the final dlog
  families and CASES        crafted (k, s) inputs; the CPU test demands that they reach every cell of every replay, the GPU test runs the same list

Replayed: k_multi_mul_coop with its join (both forms: groups joined on the host, one join on the device), k_multi_mul_wide, the per-scalar trees of
the fixed-base walks, K11 (k_msm_bucket_sum, k_msm_window_reduce[_coop], the host Horner) and the batched-row path (the sequential bucket chains,
k_msm_window_reduce_seg, k_msm_horner_rows). NOT replayed: the general Pippenger of kernels_pippenger.hpp - the order of additions inside one of its
buckets depends on block scheduling."""
import collections

import numpy as np

from edge_values import P as N  # the group order is the scalar field's modulus

CLASSES = ("left_id", "right_id", "equal", "opposite", "generic")


def classify(a, b):
    """the exit xyzz_add / xyzz_add_mixed / jac_add / jac_add_mixed / xyzz_add_block4 takes on a H + b H (curve.hpp:69-78, :88-98, :208-213, :223-228;
    coop_add.hpp:78-87, :114-117): the first operand's identity test comes first, as in xyzz_add and the block-cooperative stage 1"""
    a, b = a % N, b % N
    if a == 0:
        return "left_id"
    if b == 0:
        return "right_id"
    if a == b:
        return "equal"
    if (a + b) % N == 0:
        return "opposite"
    return "generic"


class Tally:
    def __init__(self):
        self.cells = collections.Counter()

    def add(self, stage, a, b):
        self.cells[(stage, classify(a, b))] += 1
        return (a + b) % N


# ---- digits --------------------------------------------------------------------------------------------------------------------------------------
def byte_digits(s):
    """the 32 unsigned byte digits of a canonical scalar: what the table walks index with (kernels_msm.hpp:640, :780)"""
    assert 0 <= s < N
    return list(s.to_bytes(32, "little"))


def fold_sign(s):
    """k_fold_sign (kernels_msm.hpp:54-69): (min(s, N - s), negated); 0 stays 0"""
    assert 0 <= s < N
    return (N - s, True) if s and N - s < s else (s, False)


def signed_digits(s, windows=33):
    """signed_digit (kernels_msm.hpp:129-145) of every window of an already folded scalar (bit 255 is the fold sign and masked off): digits in -128 .. 127"""
    out, carry = [], 0
    for w in range(windows):
        raw = ((s >> (8 * w)) & (0x7F if w == 31 else 0xFF)) if w < 32 else 0
        raw += carry
        carry = 1 if raw >= 128 else 0
        out.append(raw - 256 if raw >= 128 else raw)
    return out


def dot(k, s):
    return sum(a * b for a, b in zip(k, s)) % N


# ---- replay: k_multi_mul_coop ----------------------------------------------------------------------------------------------------------------------
MM_GROUPS, MM_GROUP_MIN_BLOCKS, MM_WIDE_MIN = 8, 32, 1024  # capi_group.hip:2102, :2126


def replay_multi_mul_coop(k, s, walk_groups=True):
    """kernels_msm.hpp:753-855 as launched by capi_group.hip:2152-2165. Block b owns scalars 4b .. 4b + 3; item 32 (i mod 4) + j holds
    digit_j(s_i) 2^(8j) k_i (:761-783). Tree levels off = 64 .. 1 add item kk + off into item kk for kk < off (:786-789): stages tree64 .. tree1.
    The join (:798-838): the last block loads block sums 0 .. min(nbg, 128) - 1, takes in sums kk + 128, kk + 256, ... (:819-831, stage join_takein)
    and runs a tree from top = the largest power of two below the live count (:832-838, stages join_tree<off>). With >= 32 blocks and
    SPARTAN_WALK_GROUPS unset, every ceil(nblk / 8) blocks join on their own and multi_mul_collect adds the groups' sums on the host, jac_add from
    the identity (capi_group.hip:2172-2195, stage host_groups; the order in which the slots arrive is free, taken here as 0, 1, ...)."""
    n = len(k)
    assert 0 < n < MM_WIDE_MIN and len(s) == n
    t = Tally()
    nblk = (n + 3) // 4
    sums = []
    for b in range(nblk):
        items = [0] * 128
        for q in range(4):
            i = 4 * b + q
            if i < n:
                for j, d in enumerate(byte_digits(s[i])):
                    items[32 * q + j] = (d << (8 * j)) * k[i] % N
        off = 64
        while off >= 1:
            for kk in range(off):
                items[kk] = t.add(f"tree{off}", items[kk], items[kk + off])
            off >>= 1
        sums.append(items[0])
    gblocks = (nblk + MM_GROUPS - 1) // MM_GROUPS if (walk_groups and nblk >= MM_GROUP_MIN_BLOCKS) else 0
    group_sums = []
    for g0 in range(0, nblk, gblocks or nblk):
        part = sums[g0 : g0 + (gblocks or nblk)]
        nbg = len(part)
        if nbg > 1:
            live = min(nbg, 128)
            sl = part[:live] + [0] * (128 - live)
            for base in range(128, nbg, 128):
                for kk in range(128):
                    if base + kk < nbg:
                        sl[kk] = t.add("join_takein", sl[kk], part[base + kk])
            top = 1
            while 2 * top < live:
                top <<= 1
            off = top
            while off >= 1:
                for kk in range(off):
                    sl[kk] = t.add(f"join_tree{off}", sl[kk], sl[kk + off])
                off >>= 1
            group_sums.append(sl[0])
        else:
            group_sums.append(part[0])
    if gblocks:
        acc = 0
        for v in group_sums:
            acc = t.add("host_groups", acc, v)
        return t.cells, acc
    return t.cells, group_sums[0]


COOP_STAGES = [f"tree{o}" for o in (64, 32, 16, 8, 4, 2, 1)] + ["join_takein"] + [f"join_tree{o}" for o in (64, 32, 16, 8, 4, 2, 1)] + ["host_groups"]
# nothing is unreachable in the cooperative walk: its in-scalar levels run AFTER levels 64 and 32 have mixed the block's four scalars
COOP_UNREACHABLE = {}


# ---- replay: the per-scalar trees of the fixed-base walks ----------------------------------------------------------------------------------------
def replay_fixed_base(kappa, s, wbits=8):
    """k_fixed_base_rows_coop (kernels_msm.hpp:628-651, off = 16 .. 1 at :646-649) and k_fixed_base_rows_coop_mapped<64, 8, *> (:665-703: PER = 32, the
    same levels) for wbits = 8; k_fixed_base_rows_coop_mapped<*, 16, *> (PER = 16, off = 8 .. 1) for wbits = 16. Every scalar has a tree of its own over
    the entries digit_j(s) 2^(wbits j) kappa of ONE base: item j + off is added into item j for j < off. Returns the cells of all scalars and the list
    of final dlogs. sp_fixed_base_mul_h reaches the mapped form up to 128 scalars, k_fixed_base_rows_coop up to 2048 (capi_group.hip:727-733, :742)."""
    t = Tally()
    per = 256 // wbits
    outs = []
    for sc in s:
        assert 0 <= sc < N
        items = [((sc >> (wbits * j)) & ((1 << wbits) - 1)) * kappa % N * pow(2, wbits * j, N) % N for j in range(per)]
        off = per // 2
        while off >= 1:
            for j in range(off):
                items[j] = t.add(f"fb{wbits}_tree{off}", items[j], items[j + off])
            off >>= 1
        outs.append(items[0])
    return t.cells, outs


FB_STAGES = {8: [f"fb8_tree{o}" for o in (16, 8, 4, 2, 1)], 16: [f"fb16_tree{o}" for o in (8, 4, 2, 1)]}
# One base: both operands of a tree node are A kappa and B kappa with A, B sums of DISJOINT digit sets of one canonical scalar s = A + B + (rest) < N,
# as integers 0 <= A, B and A + B <= s < N.
#   equal:    A = B mod N with A, B < N means A = B as integers; their digit sets are disjoint, so both are 0 - and that is left_id.
#   opposite: A + B = 0 mod N with 0 < A + B < N is impossible.
FB_UNREACHABLE = {(st, c): "disjoint digit sets of one canonical scalar: A = B forces A = B = 0, and 0 < A + B <= s < N is never 0 mod N"
                  for w in (8, 16) for st in FB_STAGES[w] for c in ("equal", "opposite")}


# ---- structured bases for the cooperative walk ------------------------------------------------------------------------------------------------------
def S(m):
    return pow(256, m, N)


def coop_bases(n, seed=7):
    """dlogs of n bases whose blocks of four carry, by block index mod 8, the relations the tree levels need (a, b, c, d fresh uniform values per block):
       0  a  b  a  b              scalars q and q + 2 alike: tree64 equal      4  a  256^16 a   256^8 a   256^4 a      shifted(16), (8), (4)
       1  a  b -a -b              tree64 opposite                              5  a -256^16 a  -256^8 a  -256^4 a
       2  a  a  c  d              scalars 0 and 1 alike: tree32 equal          6  a  256^2 a    256 a    -256 a        shifted(2), (1), -(1)
       3  a -a  c  d              tree32 opposite                              7  a -256^2 a    0         d            an identity base
    The scalars of a case decide which relation is used; with uniform scalars none of them shows."""
    rng = np.random.default_rng(seed)
    u = lambda: int.from_bytes(rng.bytes(40), "little") % (N - 1) + 1  # noqa: E731
    out = []
    for b in range((n + 3) // 4):
        a, bb, c, d = u(), u(), u(), u()
        out += [[a, bb, a, bb], [a, bb, -a, -bb], [a, a, c, d], [a, -a, c, d], [a, S(16) * a, S(8) * a, S(4) * a], [a, -S(16) * a, -S(8) * a, -S(4) * a],
                [a, S(2) * a, S(1) * a, -S(1) * a], [a, -S(2) * a, 0, d]][b % 8]
    return [v % N for v in out[:n]]


def uniform_values(n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.bytes(40 * n)
    return [int.from_bytes(raw[i : i + 40], "little") % N for i in range(0, len(raw), 40)]


def _low(rng, nbytes):
    """a value with every one of its low `nbytes` bytes non-zero and nothing above them"""
    return int.from_bytes(bytes(int(x) for x in rng.integers(1, 256, size=nbytes)), "little")


def coop_scalar_cases(n, seed=11):
    """[(name, s)] for coop_bases(n): scalar vectors, zero except where a case says otherwise. Block types refer to coop_bases."""
    rng = np.random.default_rng(seed + n)
    k = coop_bases(n)
    nblk = (n + 3) // 4
    r = lambda: int.from_bytes(rng.bytes(40), "little") % (N - 1) + 1  # noqa: E731
    cases = []

    def case(name, assign):
        s = [0] * n
        for i, v in assign.items():
            if i < n:
                s[i] = v % N
        cases.append((name, s))

    def block_of(t):  # first scalar of the first block of type t, or None
        return 4 * t if 4 * t + 3 < n else None

    case("zero", {})
    case("uniform", {i: r() for i in range(n)})
    case("single", {n // 2: r()})
    case("order_minus_1", {i: N - 1 for i in range(0, n, 3)})
    x = r()
    # twin / anti-twin two apart and one apart, one side only (left_id / right_id at the level where the pair would meet)
    for t, d, lvl in ((0, 2, 64), (1, 2, 64), (2, 1, 32), (3, 1, 32)):
        b0 = block_of(t)
        if b0 is None:
            continue
        case(f"pair{lvl}_type{t}", {b0: x, b0 + d: x})
        case(f"pair{lvl}_type{t}_second_only", {b0 + d: x})
        case(f"pair{lvl}_type{t}_first_only", {b0: x})
    # shifted(m): s_0 = a 256^m on base a, s_q = a on base +-256^m a, a confined to bytes [0, m): items j + m and j meet at level off = m
    for t, q, m in ((4, 1, 16), (4, 2, 8), (4, 3, 4), (5, 1, 16), (5, 2, 8), (5, 3, 4), (6, 1, 2), (6, 2, 1), (6, 3, 1), (7, 1, 2)):
        b0 = block_of(t)
        if b0 is None:
            continue
        a = _low(rng, m if m < 16 else 15)  # a 256^16 < N
        assert k[b0 + q] in (S(m) * k[b0] % N, -S(m) * k[b0] % N) and (a << (8 * m)) < N
        case(f"shifted{m}_type{t}_q{q}", {b0: a << (8 * m), b0 + q: a})
    # one non-zero byte, in each of the 32 positions: the identity on either side of every in-scalar level
    for j in range(32):
        case(f"byte{j}", {(4 * j) % n: 1 << (8 * j) if j < 31 else 0x7F << 248})
    b0 = block_of(7)
    if b0 is not None:
        case("identity_base", {b0 + 2: x, b0 + 3: r()})

    # block sums chosen at will: scalar 4b = v_b / k_4b, the block's other scalars zero
    def blocks(name, vals):
        case(name, {4 * b: v * pow(k[4 * b], -1, N) for b, v in vals.items()})

    y = r()
    gb = (nblk + MM_GROUPS - 1) // MM_GROUPS if nblk >= MM_GROUP_MIN_BLOCKS else nblk  # blocks per join with the groups on
    offs = [o for o in (1, 2, 4, 8, 16, 32, 64, 128) if o < nblk]
    for o in offs:
        blocks(f"blocks_equal_{o}", {0: x, o: x})
        blocks(f"blocks_opposite_{o}", {0: x, o: -x})
        blocks(f"blocks_second_only_{o}", {o: x})
        blocks(f"blocks_generic_{o}", {0: x, o: y})
    if nblk > 1:
        blocks("blocks_first_only", {0: x})
        blocks("blocks_all_equal", {b: x for b in range(nblk)})
        blocks("blocks_alternating", {b: x if b % 2 == 0 else -x for b in range(nblk)})
    if gb < nblk:  # the groups' sums on the host: groups 0 and 1 alike, opposite, the second empty, different
        blocks("groups_equal", {0: x, gb: x})
        blocks("groups_opposite", {0: x, gb: -x})
        blocks("groups_first_only", {0: x, 2 * gb: y})
        blocks("groups_generic", {0: x, gb: y, 2 * gb: x})
    return cases


# sizes of the cooperative walk: (n, walk_groups). 4: one block; 8: the smallest join; 130: 33 blocks, the smallest size with groups (of 5);
# 516: 129 blocks - groups of 17, and with SPARTAN_WALK_GROUPS=0 the only join with more than 128 sums (the take-in); 1022: the largest size below
# k_multi_mul_wide, 256 blocks in groups of 32
COOP_SIZES = [(4, True), (8, True), (130, True), (516, True), (516, False), (1022, True)]


def coop_cases():
    """[(n, walk_groups, name, k, s)]: every case of the cooperative walk, for the CPU coverage test and the GPU test alike"""
    out = []
    for n, groups in COOP_SIZES:
        k = coop_bases(n)
        for name, s in coop_scalar_cases(n):
            if n == 1022 and not (name.startswith(("blocks_", "groups_")) or name in ("zero", "uniform", "single")):
                continue  # the block-level cases are those of n = 130; this size is about its join
            out.append((n, groups, name, k, s))
    return out


# ---- replay: k_multi_mul_wide ------------------------------------------------------------------------------------------------------------------------
WIDE_BLOCK = 32  # scalars per block: 1024 (scalar, digit) items


def replay_multi_mul_wide(k, s):
    """kernels_msm.hpp:863-939. Block b owns scalars 32b .. 32b + 31; thread t takes bytes 2 (t mod 16) and 2 (t mod 16) + 1 of scalar t / 16
    (:872-873): entry 0 by conversion, entry 1 by xyzz_add_mixed when its digit is non-zero (:883-884, stage pair). Lanes 32 .. 63 of a wave hand their
    sum to lanes 0 .. 31 (:886-887, stage shfl32: scalar u meets u + 2); the 256 sums go through the cooperative level + 128 (:891, stage coop128: u meets
    u + 16) and levels 64 .. 1 (:892-895, stages tree64 .. tree1: u meets u + 8, u + 4, u + 1, then byte pairs 16, 8, 4, 2 bytes apart). The join
    (:896-924) is k_multi_mul_coop's without groups and without a take-in: the launcher keeps the grid within 128 blocks."""
    n = len(k)
    assert MM_WIDE_MIN <= n <= 4096 and len(s) == n
    t = Tally()
    nblk = (32 * n + 1023) // 1024
    sums = []
    for b in range(nblk):
        acc = [0] * 512
        digits = [byte_digits(s[i]) for i in range(WIDE_BLOCK * b, min(n, WIDE_BLOCK * (b + 1)))]
        for th in range(512):
            i = WIDE_BLOCK * b + th // 16
            if i < n:
                dg = digits[th // 16]
                j = 2 * (th % 16)
                e0 = (dg[j] << (8 * j)) * k[i] % N
                if dg[j + 1]:
                    e0 = t.add("pair", e0, (dg[j + 1] << (8 * (j + 1))) * k[i] % N)
                acc[th] = e0
        sl = [0] * 256
        for wv in range(8):
            for ln in range(32):
                sl[32 * wv + ln] = t.add("shfl32", acc[64 * wv + ln], acc[64 * wv + ln + 32])
        for kk in range(128):
            sl[kk] = t.add("coop128", sl[kk], sl[kk + 128])
        off = 64
        while off >= 1:
            for kk in range(off):
                sl[kk] = t.add(f"tree{off}", sl[kk], sl[kk + off])
            off >>= 1
        sums.append(sl[0])
    if nblk > 1:
        live = min(nblk, 128)
        sl = sums[:live] + [0] * (128 - live)
        top = 1
        while 2 * top < live:
            top <<= 1
        off = top
        while off >= 1:
            for kk in range(off):
                sl[kk] = t.add(f"join_tree{off}", sl[kk], sl[kk + off])
            off >>= 1
        return t.cells, sl[0]
    return t.cells, sums[0]


WIDE_N = 1030  # 33 blocks (the last one partial): just above the launcher's switch at 1024; its join runs levels 32 .. 1
WIDE_STAGES = ["pair", "shfl32", "coop128"] + [f"tree{o}" for o in (64, 32, 16, 8, 4, 2, 1)] + [f"join_tree{o}" for o in (32, 16, 8, 4, 2, 1)]
# pair adds entries d0 256^j k and d1 256^(j+1) k of ONE base, d1 != 0 (the addition is skipped otherwise), 0 <= d0 <= 255, 1 <= d1 <= 255:
_PAIR = "two byte entries of one base: A = d0 256^j, B = d1 256^(j+1) with B != 0 and 0 < A + B < N as integers"
WIDE_UNREACHABLE = {("pair", "right_id"): _PAIR + "; B k = 0 needs k = 0, and then A k = 0 as well: that is left_id",
                    ("pair", "equal"): _PAIR + "; A = B would need d0 = 256 d1 > 255",
                    ("pair", "opposite"): _PAIR + "; A + B is never 0 mod N"}


def wide_bases(n, seed=8):
    """dlogs of n bases in blocks of 32, by block index mod 5 (a fresh uniform a per block; u = the scalar's place in the block):
       0  every base a                              scalars any distance apart alike: equal at the level where they meet
       1  (-1)^popcount(u) a                         u and u + 2^t opposite for a u with bit t clear
       2  a, 256^16 a, 256^8 a, 256^4 a, ., 256^2 a at u = 0, 1, 2, 3, 5; uniform elsewhere: byte pairs 16, 8, 4, 2 bytes apart carry one point
       3  the negated multiples of block 2 at u = 1, 2, 3, 5; the identity at u = 6
       4  uniform"""
    rng = np.random.default_rng(seed)
    u = lambda: int.from_bytes(rng.bytes(40), "little") % (N - 1) + 1  # noqa: E731
    out = []
    for b in range((n + WIDE_BLOCK - 1) // WIDE_BLOCK):
        a = u()
        blk = [u() for _ in range(WIDE_BLOCK)]
        blk[0] = a
        t = b % 5
        if t == 0:
            blk = [a] * WIDE_BLOCK
        elif t == 1:
            blk = [a if bin(i).count("1") % 2 == 0 else -a for i in range(WIDE_BLOCK)]
        elif t in (2, 3):
            sg = 1 if t == 2 else -1
            for i, m in ((1, 16), (2, 8), (3, 4), (5, 2)):
                blk[i] = sg * S(m) * a
            if t == 3:
                blk[6] = 0
        out += blk
    return [v % N for v in out[:n]]


def wide_scalar_cases(n=WIDE_N, seed=12):
    """[(name, s)] for wide_bases(n)"""
    rng = np.random.default_rng(seed + n)
    k = wide_bases(n)
    nblk = (n + WIDE_BLOCK - 1) // WIDE_BLOCK
    r = lambda: int.from_bytes(rng.bytes(40), "little") % (N - 1) + 1  # noqa: E731
    cases = []

    def case(name, assign):
        s = [0] * n
        for i, v in assign.items():
            if i < n:
                s[i] = v % N
        cases.append((name, s))

    case("zero", {})
    case("uniform", {i: r() for i in range(n)})
    case("single", {n // 2: r()})
    case("order_minus_1", {i: N - 1 for i in range(0, n, 3)})
    x, y = r(), r()
    for t in (0, 1):  # equal / opposite bases at every distance at which two scalars of a block meet
        b0 = WIDE_BLOCK * t
        for d in (2, 16, 8, 4, 1):
            case(f"pair_d{d}_type{t}", {b0: x, b0 + d: x})
            case(f"pair_d{d}_type{t}_second_only", {b0 + d: x})
            case(f"pair_d{d}_type{t}_first_only", {b0: x})
    for t in (2, 3):
        b0 = WIDE_BLOCK * t
        for q, m in ((1, 16), (2, 8), (3, 4), (5, 2)):
            a = _low(rng, min(m, 15))
            assert k[b0 + q] in (S(m) * k[b0] % N, -S(m) * k[b0] % N)
            case(f"shifted{m}_type{t}", {b0: a << (8 * m), b0 + q: a})
    case("identity_base", {3 * WIDE_BLOCK + 6: x, 3 * WIDE_BLOCK + 7: y})
    for j in range(32):
        case(f"byte{j}", {(WIDE_BLOCK * j + j) % n: 1 << (8 * j) if j < 31 else 0x7F << 248})
    case("odd_bytes_only", {4 * WIDE_BLOCK + 1: int.from_bytes(bytes([0, 9] * 15 + [0, 0]), "little")})

    def blocks(name, vals):
        case(name, {WIDE_BLOCK * b: v * pow(k[WIDE_BLOCK * b], -1, N) for b, v in vals.items()})

    for o in [o for o in (1, 2, 4, 8, 16, 32, 64) if o < nblk]:
        blocks(f"blocks_equal_{o}", {0: x, o: x})
        blocks(f"blocks_opposite_{o}", {0: x, o: -x})
        blocks(f"blocks_second_only_{o}", {o: x})
        blocks(f"blocks_generic_{o}", {0: x, o: y})
    blocks("blocks_first_only", {0: x})
    blocks("blocks_all_equal", {b: x for b in range(nblk)})
    blocks("blocks_alternating", {b: x if b % 2 == 0 else -x for b in range(nblk)})
    return cases


# ---- replays: the signed-digit bucket method -------------------------------------------------------------------------------------------------------
# The counting sorts (k_msm_sort, k_msm_sort_digits, k_msm_sort_rows) place a bucket's entries with an atomic cursor: the order INSIDE a bucket is the
# order in which the atomics land. `order` names the one a replay assumes: "index" (thread order), "reverse", or a seed for a permutation. The final
# dlog does not depend on it; the cells may, so the coverage conditions are demanded under "index" and under "reverse".
MSM_WINDOWS, MSM_BUCKETS = 33, 128


def _bucket_lists(k, s, order="index"):
    """k_fold_sign + signed_digit + the counting sort: buckets[w][b] = the dlogs (negated where the entry's bit 31 is set) of bucket b of window w"""
    buckets = [[[] for _ in range(MSM_BUCKETS)] for _ in range(MSM_WINDOWS)]
    for kj, sj in zip(k, s):
        f, neg = fold_sign(sj)
        for w, d in enumerate(signed_digits(f)):
            if d:
                buckets[w][abs(d) - 1].append((-kj if (d < 0) != neg else kj) % N)
    if order != "index":
        rng = None if order == "reverse" else np.random.default_rng(order)
        for win in buckets:
            for lst in win:
                if order == "reverse":
                    lst.reverse()
                elif len(lst) > 1:
                    lst[:] = [lst[int(i)] for i in rng.permutation(len(lst))]
    return buckets


def _horner(t, stage, wsums):
    """acc = 2^8 acc + W_w from the top window down (msm_finish capi_group.hip:113-117, horner_rows_host, k_msm_horner_rows kernels_msm.hpp:507-516)"""
    acc = 0
    for w in range(len(wsums) - 1, -1, -1):
        acc = t.add(stage, acc * 256 % N, wsums[w])
    return acc


def _k11_window(t, win):
    sk = []
    for lst in win:
        lanes = [0] * 8
        for p, v in enumerate(lst):
            lanes[p % 8] = t.add("bucket_chain", lanes[p % 8], v)
        for d in (4, 2, 1):
            for sub in range(d):
                lanes[sub] = t.add(f"bucket_shfl{d}", lanes[sub], lanes[sub + d])
        sk.append(lanes[0])
    off = 1
    while off < MSM_BUCKETS:
        sk = [t.add(f"scan{off}", sk[i], sk[i + off]) if i + off < MSM_BUCKETS else sk[i] for i in range(MSM_BUCKETS)]
        off <<= 1
    off = MSM_BUCKETS // 2
    while off >= 1:
        for i in range(off):
            sk[i] = t.add(f"wtree{off}", sk[i], sk[i + off])
        off >>= 1
    return sk[0]


def _row_window(t, win):
    bsum = []
    for lst in win:
        acc = 0
        for v in lst:
            acc = t.add("seq_chain", acc, v)
        bsum.append(acc)
    runs, accs = [], []
    for seg in range(8):
        run = acc = 0
        for i in range(15, -1, -1):
            run = t.add("seg_run", run, bsum[16 * seg + i])
            acc = t.add("seg_acc", acc, run)
        runs.append(run)
        accs.append(acc)
    for d in (4, 2, 1):
        for seg in range(d):
            accs[seg] = t.add(f"seg_x{d}", accs[seg], accs[seg + d])
    rr = y = 0
    for sg in range(7, 0, -1):
        rr = t.add("seg_rr", rr, runs[sg])
        y = t.add("seg_y", y, rr)
    return t.add("seg_final", accs[0], 16 * y % N)


_EMPTY_WINDOW = {}


def _windows(t, per_window, k, s, order):
    """the window sums of one input; an empty window (every addition identity + identity) is replayed once and its cells reused"""
    if per_window not in _EMPTY_WINDOW:
        e = Tally()
        assert per_window(e, [[] for _ in range(MSM_BUCKETS)]) == 0
        _EMPTY_WINDOW[per_window] = e.cells
    wsums = []
    for win in _bucket_lists(k, s, order):
        if any(win):
            wsums.append(per_window(t, win))
        else:
            t.cells.update(_EMPTY_WINDOW[per_window])
            wsums.append(0)
    return wsums


def replay_msm_k11(k, s, order="index"):
    """sp_msm below 4096 points (msm_launch capi_group.hip:62-105). k_msm_bucket_sum (kernels_msm.hpp:258-283): lane `sub` of a bucket's 8 adds entries
    sub, sub + 8, ... with xyzz_add_mixed from the identity (:270-275, stage bucket_chain), then shuffle levels 4, 2, 1 (:278-281, stages bucket_shfl4 ..).
    k_msm_window_reduce_coop (:286-305; k_msm_window_reduce :308-324 has the same order): the suffix scan s_k += s_(k + off), off = 1 .. 64, every
    level reading the values of the level before (:296-299, stages scan1 .. scan64), then the tree off = 64 .. 1 (:300-303, stages wtree64 .. wtree1).
    The Horner on the host (stage horner)."""
    t = Tally()
    return t.cells, _horner(t, "horner", _windows(t, _k11_window, k, s, order))


K11_STAGES = (["bucket_chain"] + [f"bucket_shfl{d}" for d in (4, 2, 1)] + [f"scan{o}" for o in (1, 2, 4, 8, 16, 32, 64)]
              + [f"wtree{o}" for o in (64, 32, 16, 8, 4, 2, 1)] + ["horner"])
K11_UNREACHABLE = {}


def replay_batched_row(k, s, order="index"):
    """One row of the batched-row path (msm_shared_weights_on from 64 rows, msm_shared_weights_grouped_on, msm_rows_batched). The bucket chain of
    k_msm_bucket_sum_shared / _grouped / _rows (kernels_msm.hpp:427-433, :458-464, :400-406): one lane adds a bucket's entries in turn from the identity
    (stage seq_chain). k_msm_window_reduce_seg (:471-503): lane seg runs run += B_(16 seg + i), acc += run for i = 15 .. 0 (:478-481, stages seg_run,
    seg_acc); x = sum of the acc by shuffle levels 4, 2, 1 (:486-489, stages seg_x4 ..); rr += run_s, y += rr for s = 7 .. 1 (:491-497, stages seg_rr,
    seg_y); four doublings of y and the final jac_add(x, 16 y) (:499-501, stage seg_final). The Horner, on the device or on host threads
    (stage horner_rows)."""
    t = Tally()
    return t.cells, _horner(t, "horner_rows", _windows(t, _row_window, k, s, order))


ROW_STAGES = ["seq_chain", "seg_run", "seg_acc", "seg_x4", "seg_x2", "seg_x1", "seg_rr", "seg_y", "seg_final", "horner_rows"]
ROW_UNREACHABLE = {}

# Inputs given as bucket contents: {(window, bucket): [dlogs]} - base d H gets the scalar (bucket + 1) 256^window: one positive digit, no carry, no fold
_X, _Y, _Z = (v or 1 for v in uniform_values(3, 59))
_W = 2  # the window the bucket-level cases live in


def spec_input(spec, n=None):
    k, s = [], []
    for (w, b), ds in spec.items():
        assert 0 <= b < 127 and 0 <= w < 31
        for d in ds:
            k.append(d % N)
            s.append((b + 1) << (8 * w))
    pad = (n or len(k)) - len(k)
    assert pad >= 0
    return k + [1] * pad, s + [0] * pad


def k11_specs():
    """[(name, spec)] reaching every cell of replay_msm_k11. S_k = the suffix sum of the buckets from k up: with bucket `off` = x and bucket 0 = c x,
    node 0 of tree level `off` adds S_0 = (1 + c) x and S_off = x."""
    x, y = _X, _Y
    u16 = [v or 1 for v in uniform_values(16, 67)]
    out = [("chain_equal", {(_W, 5): [x] * 16}), ("chain_opposite", {(_W, 5): [x] * 8 + [-x] * 8}), ("chain_identity_bases", {(_W, 5): [x] * 8 + [0] * 8 + [x] * 8}),
           ("chain_generic", {(_W, 5): u16}), ("shfl_equal", {(_W, 5): [x] * 8}), ("shfl4_opposite", {(_W, 5): [x] * 4 + [-x] * 4}),
           ("shfl2_opposite", {(_W, 5): [x, y, -x, -y]}), ("shfl1_opposite", {(_W, 5): [x, -x]}), ("shfl_generic", {(_W, 5): u16[:8]}),
           ("shfl2_equal", {(_W, 5): [x] * 4}), ("shfl1_equal", {(_W, 5): [x] * 2}), ("one_entry", {(_W, 0): [x]}),
           ("horner_equal", {(6, 4): [x], (5, 4): [256 * x]}), ("horner_opposite", {(6, 4): [x], (5, 4): [-256 * x]}), ("horner_generic", {(6, 4): [x], (5, 4): [y]}),
           ("top_bucket_only", {(_W, 126): [x]})]
    for off in (1, 2, 4, 8, 16, 32, 64):
        out += [(f"scan{off}_equal", {(_W, 0): [x], (_W, off): [x]}), (f"scan{off}_opposite", {(_W, 0): [x], (_W, off): [-x]}),
                (f"scan{off}_generic", {(_W, 0): [x], (_W, off): [y]}), (f"wtree{off}_equal", {(_W, off): [x]}),
                (f"wtree{off}_opposite", {(_W, off): [x], (_W, 0): [-2 * x]}), (f"wtree{off}_left_id", {(_W, off): [x], (_W, 0): [-x]})]
    return out


def row_specs():
    """[(name, spec)] reaching every cell of replay_batched_row; at most three entries per bucket, buckets out of ROW_SLOTS only (shared_rows_case)"""
    x, y, z = _X, _Y, _Z
    c1715 = -17 * pow(15, -1, N) * x
    out = [("chain_equal", {(_W, 0): [x, x]}), ("chain_opposite", {(_W, 0): [x, -x]}), ("chain_generic", {(_W, 0): [x, y]}), ("chain_identity_base", {(_W, 0): [x, 0, x]}),
           ("run_equal", {(_W, 15): [x], (_W, 14): [x]}), ("run_opposite", {(_W, 15): [x], (_W, 14): [-x]}), ("run_generic", {(_W, 15): [x], (_W, 14): [y]}),
           ("bucket_15_only", {(_W, 15): [x]}), ("acc_opposite", {(_W, 15): [x], (_W, 14): [-2 * x]}),
           ("rr_equal", {(_W, 112): [x], (_W, 96): [x]}), ("rr_opposite", {(_W, 112): [x], (_W, 96): [-x]}), ("rr_generic", {(_W, 112): [x], (_W, 96): [y]}),
           ("bucket_112_only", {(_W, 112): [x]}), ("y_opposite", {(_W, 112): [x], (_W, 96): [-2 * x]}),
           ("final_equal", {(_W, 16): [x], (_W, 14): [x]}), ("final_opposite", {(_W, 16): [x], (_W, 14): [c1715]}), ("final_left_id", {(_W, 16): [x], (_W, 0): [-x]}),
           ("bucket_0_only", {(_W, 0): [x]}), ("final_generic", {(_W, 16): [x], (_W, 14): [y], (_W, 0): [z]}),
           ("horner_equal", {(6, 4): [x], (5, 4): [256 * x]}), ("horner_opposite", {(6, 4): [x], (5, 4): [-256 * x]}), ("horner_generic", {(6, 4): [x], (5, 4): [y]}),
           ("all_identities", {})]
    for d, b in ((4, 64), (2, 32), (1, 16)):
        out += [(f"x{d}_equal", {(_W, 0): [x], (_W, b): [x]}), (f"x{d}_opposite", {(_W, 0): [x], (_W, b): [-x]}), (f"x{d}_generic", {(_W, 0): [x], (_W, b): [y]}),
                (f"x{d}_second_only", {(_W, b): [x]})]
    return out


ROW_SLOTS = [(_W, b) for b in (0, 14, 15, 16, 32, 64, 96, 112) for _ in range(3)] + [(6, 4), (5, 4)]


def shared_rows_case(rows, n=256, seed=37):
    """(s, [(name, k_row)]) for sp_msm_shared_weights[_grouped]: ONE weight vector whose first positions are the palette ROW_SLOTS (three positions per
    bucket) and whose other weights are uniform; a row puts its spec's dlogs on the palette and the identity everywhere else. Every third row is
    uniform bases instead, so neighbouring lanes take exceptional and generic exits side by side."""
    s = [(b + 1) << (8 * w) for w, b in ROW_SLOTS] + uniform_values(n - len(ROW_SLOTS), seed)
    s[len(ROW_SLOTS)], s[len(ROW_SLOTS) + 1], s[len(ROW_SLOTS) + 2] = 0, 1, N - 1
    specs = row_specs()
    out = []
    i = 0
    for r in range(rows):
        if r % 3 == 2:
            out.append((f"uniform_{r}", [v or 1 for v in uniform_values(n, seed + 100 + r)]))
            continue
        name, spec = specs[i % len(specs)]
        i += 1
        k = [0] * n
        for slot, ds in spec.items():
            pos = [p for p, sl in enumerate(ROW_SLOTS) if sl == slot]
            assert len(ds) <= len(pos), (name, slot)
            for p, d in zip(pos, ds):
                k[p] = d % N
        out.append((name, k))
    return s, out


# ---- the fixed-base walk of h ------------------------------------------------------------------------------------------------------------------------
def fixed_base_scalars(n, seed=13):
    """n canonical scalars for ONE base: one non-zero byte in each of the 32 positions, every byte zero but two, shifted(m) restated for one base (a and
    a 256^m side by side), 0, 1, N - 1, and uniform values for the rest"""
    rng = np.random.default_rng(seed + n)
    s = [0, 1, N - 1, 255, 256]
    s += [1 << (8 * j) for j in range(32)]
    if n >= 128:
        s += [(0xFF << (8 * j)) % (1 << 255) for j in range(32)]
    for m in (16, 8, 4, 2, 1):
        a = _low(rng, min(m, 15))
        s += [a, a << (8 * m), a | (a << (8 * m))]
    for _ in range(12):
        i, j = sorted(int(v) for v in rng.choice(32, size=2, replace=False))
        s.append(((int(rng.integers(1, 256)) << (8 * i)) | (int(rng.integers(1, 128)) << (8 * j))) % N)
    assert len(s) <= n, len(s)
    s += uniform_values(n - len(s), seed + 1)
    assert all(0 <= v < N for v in s)
    return s


FB_SIZES = [70, 600]  # the mapped form and the copy form of sp_fixed_base_mul_h


# ---- families for the kernels that are not replayed ----------------------------------------------------------------------------------------------------
def twin(n, delta, seed=17, sign=1):
    """k_{i + delta} = sign k_i and s_{i + delta} = s_i for the first element of every run of 2 delta: (k, s) of n uniform values otherwise"""
    k, s = uniform_values(n, seed), uniform_values(n, seed + 1)
    k = [v or 1 for v in k]
    for i in range(n - delta):
        if (i // delta) % 2 == 0:
            k[i + delta] = sign * k[i] % N
            s[i + delta] = s[i]
    return k, s


def anti_twin(n, delta, seed=19):
    return twin(n, delta, seed, sign=-1)


def one_bucket(n, seed=23, sign=1):
    """all scalars equal: every base of a window lands in ONE signed-digit bucket, so the suffix sums of the window reduction are all equal; the bases
    come in twins (sign = 1) or anti-twins (sign = -1)"""
    k, _ = twin(n, 1, seed, sign)
    return k, [uniform_values(1, seed + 2)[0]] * n


def horner_collision(n, sign, w=3, c=5, seed=29):
    """base 0 = k H with the single digit c at window w + 1, base 1 = sign 256 k H with the digit c at window w: the window sum W_w is sign 256 times the
    Horner accumulator that meets it (acc 2^8 + W_w: the doubling exit, or the identity that is then doubled on). The other scalars are zero."""
    k = [v or 1 for v in uniform_values(n, seed)]
    s = [0] * n
    k[1] = sign * 256 * k[0] % N
    s[0], s[1] = c << (8 * (w + 1)), c << (8 * w)
    return k, s


def seg_collision(n, sign, w=2, seed=31):
    """k_msm_window_reduce_seg (kernels_msm.hpp:471-503): in window w, base 0 = k H has digit 17 (bucket 16, the first of segment 1: run_1 = acc_1 = Q)
    and base 1 has digit 15 (the last bucket of segment 0: acc_0 = 15 Q'). With Q' = Q, x = acc_0 + acc_1 = 16 Q = 16 y and the final
    jac_add(x, 16 y) takes its doubling exit; with Q' = -(17 / 15) Q, x = -16 Q and it returns the identity."""
    k = [v or 1 for v in uniform_values(n, seed)]
    s = [0] * n
    k[1] = k[0] if sign > 0 else -17 * pow(15, -1, N) * k[0] % N
    s[0], s[1] = 17 << (8 * w), 15 << (8 * w)
    return k, s


def key_dlogs(width=32, seed=41):
    """dlogs of a commitment key of `width` bases: twins in columns (0, 1) and (7, 7 + width / 2), anti-twins in (2, 3) and (9, 9 + width / 2), an
    identity column (4), uniform values elsewhere. Columns one apart meet at the last level of a tree over the columns, columns width / 2 apart at its
    first (k_msm_binary_rows kernels_msm.hpp:580-583, k_sum_rows_of_points :619-622)."""
    k = [v or 1 for v in uniform_values(width, seed)]
    h = width // 2
    k[1], k[3], k[4], k[7 + h], k[9 + h] = k[0], N - k[2], 0, k[7], N - k[9]
    return k


def key_rows(width, seed=43):
    """[(name, {column: scalar})]: rows for a key of key_dlogs(width) - a twin pair alone, an anti-twin pair alone, both distances, every column, none,
    the identity column alone; the scalars are 1 (bit rows) unless given"""
    h = width // 2
    u = uniform_values(4, seed)
    rows = [("twins_adjacent", {0: 1, 1: 1}), ("twins_half_apart", {7: 1, 7 + h: 1}), ("anti_twins_adjacent", {2: 1, 3: 1}),
            ("anti_twins_half_apart", {9: 1, 9 + h: 1}), ("all_columns", {c: 1 for c in range(width)}), ("none", {}), ("identity_column", {4: 1}),
            ("twins_and_anti_twins", {0: 1, 1: 1, 2: 1, 3: 1, 7: 1, 7 + h: 1, 9: 1, 9 + h: 1}), ("one_column", {5: 1}),
            ("full_twins_adjacent", {0: u[0], 1: u[0]}), ("full_twins_half_apart", {7: u[1], 7 + h: u[1]}), ("full_anti_twins_adjacent", {2: u[2], 3: u[2]}),
            ("full_anti_twins_half_apart", {9: u[3], 9 + h: u[3]}), ("full_all_equal", {c: u[0] for c in range(width)}),
            ("full_identity_column", {4: u[1], 6: u[2]}),
            # the blind's term is the row's own point, or its negation (key_blinds): P + P and P - P where h * blind joins the row
            ("blind_equal", {0: 1}), ("blind_opposite", {0: 1}), ("full_blind_equal", {0: u[3]}), ("full_blind_opposite", {0: u[3]})]
    return rows


def key_blinds(rows, k, kappa, seed=47):
    """a blind per row of key_rows: uniform, except that `blind_equal` / `blind_opposite` rows get +-(the row's dlog) / kappa, kappa the dlog of h"""
    out = uniform_values(len(rows), seed)
    for i, (name, cols) in enumerate(rows):
        if name.endswith(("blind_equal", "blind_opposite")):
            d = sum(v * k[c] for c, v in cols.items()) % N
            out[i] = (d if name.endswith("equal") else -d) * pow(kappa, -1, N) % N
    return out


class DlogPoints:
    """a H as affine Montgomery limbs (numpy (8,) u64; zeros for the identity) for the dlogs asked for, by the ORACLE's fixed-base multiplication - never
    by a kernel under test. One oracle call per batch of new values."""

    def __init__(self, label=b"group_edges"):
        import ctypes

        import oracle_lib as ol

        self._ol, self._ct = ol, ctypes
        self.H = np.zeros((1, 8), dtype=np.uint64)
        ol.lib().orc_from_label(label, ctypes.c_size_t(1), ol.p64(self.H))
        self.known = {0: np.zeros(8, dtype=np.uint64)}

    def need(self, dlogs):
        ol = self._ol
        new = sorted({d % N for d in dlogs} - set(self.known))
        if new:
            out = np.zeros((len(new), 8), dtype=np.uint64)
            ol.lib().orc_fixed_base_mul(ol.p64(np.ascontiguousarray(self.H[0])), ol.p64(ol.mont_array(new)), self._ct.c_size_t(len(new)), ol.p64(out))
            for d, row in zip(new, out):
                self.known[d] = row.copy()

    def point(self, d):
        self.need([d])
        return self.known[d % N]

    def points(self, dlogs):
        self.need(dlogs)
        return np.stack([self.known[d % N] for d in dlogs]) if len(dlogs) else np.zeros((0, 8), dtype=np.uint64)


def msm_families(n):
    """[(name, (k, s))] of n points for sp_msm below the Pippenger switch"""
    fams = [("one_bucket_twins", one_bucket(n)), ("one_bucket_anti_twins", one_bucket(n, sign=-1)), ("twin", twin(n, 1)), ("anti_twin", anti_twin(n, 1)),
            ("horner_equal", horner_collision(n, 1)), ("horner_opposite", horner_collision(n, -1)), ("seg_equal", seg_collision(n, 1)),
            ("seg_opposite", seg_collision(n, -1)), ("zero_scalars", (uniform_values(n, 71), [0] * n)),
            ("single", (uniform_values(n, 72), [0] * (n - 1) + [uniform_values(1, 73)[0]])), ("uniform", (uniform_values(n, 74), uniform_values(n, 75)))]
    if n >= 4:
        fams += [("twin_2", twin(n, 2)), ("anti_twin_2", anti_twin(n, 2))]
    fams += [(name + "_with_identities", with_identities(*ks)) for name, ks in fams[:4]]
    return fams


K11_SIZES = [2, 9, 64, 1000]


def k11_cases():
    """[(name, k, s)]: the bucket-content cases at their own sizes (up to 24 points) and the families at K11_SIZES"""
    out = [(name,) + spec_input(spec) for name, spec in k11_specs()]
    for n in K11_SIZES:
        out += [(f"{name}_{n}", k, s) for name, (k, s) in msm_families(n)]
    return out


def with_identities(k, s, every=5):
    """the same input with the base of every `every`-th position replaced by the identity (dlog 0)"""
    return [0 if i % every == 2 else v for i, v in enumerate(k)], list(s)
