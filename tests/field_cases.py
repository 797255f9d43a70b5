"""Designed operands and branch-path mirrors of the device field primitives.

A helper (not a conftest) shared by tests/test_field_cases.py (CPU) and the
GPU tests of the device-check library. Two things live here:

* The designed operand sets: values at the carry / borrow boundaries of the
  32-bit-limb Goldilocks arithmetic of csrc/dev_common.h and the shift
  twiddles of csrc/gl_pow2.h.
* A Python-integer mirror of each function that follows the device code
  branch for branch and returns (value, path). The CPU test proves on the
  mirror that the designed operands reach every branch path a large random
  sweep reaches; the GPU tests then run the same operands through the real
  functions and compare with plain `%` arithmetic.
"""
import ctypes as C
import random

P = 0xFFFFFFFF00000001
EPS = 0xFFFFFFFF
M64 = (1 << 64) - 1

# canonical values at the carry / borrow boundaries of the 32-bit-lane
# arithmetic (the EDGE set of test_gpu_parity.py)
EDGE = [0, 1, 2, P - 1, P - 2, EPS, EPS + 1, EPS - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 63) - 1,
        P - EPS, P - EPS - 1, P - (1 << 32), (1 << 64) - (1 << 33), P >> 1, (P >> 1) + 1]
NONCANON = [P, P + 1, P + 2, P + EPS - 1, M64 - 1, M64]  # for functions documented for "any < 2^64"
I64_EDGE = [0, 1, -1, 2, -2, (1 << 31), -(1 << 31), (1 << 32), -(1 << 32), (1 << 32) - 1, -((1 << 32) - 1),
            (1 << 62), -(1 << 62), (1 << 63) - 1, -((1 << 63) - 1)]  # gl_from_i64 documents |x| < 2^63


def _uniq(xs):
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def canonical_designed():
    """EDGE, 2^k, 2^k +- 1, p - 2^k, p - 2^k +- 1, limb patterns: all < p."""
    v = list(EDGE)
    for k in range(64):
        for d in (-1, 0, 1):
            v.append(((1 << k) + d) % P)
            v.append((P - (1 << k) + d) % P)
    for k in range(1, 32):  # both limbs at a boundary: ones below bit k of each limb, and their complements
        lo = (1 << k) - 1
        v += [(lo << 32) | lo, (lo << 32), ((EPS ^ lo) << 32) % P, (((EPS ^ lo) << 32) | (EPS ^ lo)) % P,
              ((lo << 32) | EPS) % P, ((EPS - 1) << 32) | (EPS ^ lo)]
    v += [0xAAAAAAAB00000000, 3 << 32, 1 << 48, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x00000000FFFFFFFE,
          0xFFFFFFFE00000000, 0xFFFFFFFEFFFFFFFF, 0xFFFFFFFF00000000, 0x7FFFFFFF80000000, 0x80000000FFFFFFFF]
    return _uniq(x for x in v if 0 <= x < P)


def any64_designed():
    return _uniq(canonical_designed() + NONCANON + [((1 << k) - 1) for k in range(60, 65)])


def _inv64(a):  # inverse of odd a modulo 2^64
    return pow(a, -1, 1 << 64)


# Named products at the rare branches of gl_reduce128_weak (lo, h1 = hi >> 32, h0 = hi & eps):
#   borrow needs lo < h1 (probability ~2^-33 for a random product); without a
#   later carry it also needs h0 <= 1.
MUL_NAMED = {  # name: (a, b), the (borrow, carry, canon) path in the name
    "b1_c0_n0": (1 << 48, 1 << 48),                    # 2^96: lo = 0, hi = 2^32 -> p - 1
    "b1_c0_n1": (0xAAAAAAAB00000000, 3 << 32),         # hi = 2^33 + 1, lo = 0 -> r = 2^64 - 2 >= p
    "b1_c0_n1_sq": (P - 1, P - 1),                     # (-1)^2: lo = 1 < h1, h0 = 1
    "b1_c1_n0": (1 << 63, 0xFFFFFFFF00000000),
    "b0_c1_n0": (0xFFFFFFFF00000000, (1 << 32) + 1),
    "b0_c0_n1": (EPS, (1 << 32) + 1),                  # product 2^64 - 1 in [p, 2^64)
    "b0_c0_n0": (0, P - 1),
}


def mul_pairs_designed():
    """Pairs for gl_mul / gl_mul128: designed x designed corners, the named
    products, and pairs (a, c a^-1 mod 2^64) whose low product word is the
    tiny c, so lo < hi >> 32: the borrow of gl_reduce128_weak."""
    d = any64_designed()
    small = EDGE + NONCANON
    pairs = [(a, b) for a in small for b in small]
    pairs += [(a, b) for a in d for b in (0, 1, 2, P - 1, EPS, 1 << 32, 1 << 63, M64)]
    pairs += list(MUL_NAMED.values())
    odd = [a for a in d if a & 1 and a > (1 << 33)]
    for a in odd:
        for c in (0, 1, 2, 3, EPS - 1, EPS):
            pairs.append((a, (c * _inv64(a)) & M64))
    for k in range(1, 32):  # products u v 2^64 with the low word of hi equal to 0 or 1
        u = (1 << k) + 1
        v = pow(u, -1, 1 << 32)
        pairs += [(u << 32, v << 32), (1 << (32 + k), 1 << (64 - k))]
    return _uniq(pairs)


def reduce_pairs_designed():
    """Raw (lo, hi) for gl_reduce128: every combination of limb boundaries."""
    w = [0, 1, 2, EPS - 1, EPS, 1 << 31, (1 << 31) - 1]
    words = _uniq([(h << 32) | l for h in w for l in w])
    return _uniq([(lo, hi) for lo in words for hi in words] + [(lo * hi & M64, lo * hi >> 64) for lo, hi in
                                                                mul_pairs_designed()[:4000]])


def add_envelope_designed():
    """gl_add(A, h eps): A any word, h < 2^32 at its boundaries (the shift
    twiddles' use of gl_add with a non-canonical first operand)."""
    hs = [0, 1, 2, 3, 1 << 16, 1 << 31, (1 << 31) - 1, (1 << 31) + 1, EPS - 2, EPS - 1, EPS]
    return [(a, h * EPS) for a in any64_designed() for h in hs]


def seeded(n, seed, bound=P):
    rng = random.Random(seed)
    return [rng.randrange(bound) for _ in range(n)]


# ---------------------------------------------------------------- mirrors
def add64c(a, b):
    s = a + b
    return s & M64, s >> 64


def sub64b(a, b):
    d = a - b
    return d & M64, int(d < 0)


def m_add(a, b):
    s, c1 = add64c(a, b)
    t, c2 = add64c(s, EPS)
    return (t if (c1 | c2) else s), (c1, c2)


def m_sub(a, b):
    d, br = sub64b(a, b)
    return ((d - EPS) & M64 if br else d), (br,)


def m_canon(r):
    t, c = add64c(r, EPS)
    return (t if c else r), (c,)


def m_neg(x):
    return (P - x if x else 0), (int(x != 0),)


def m_mul128(a, b):
    a0, a1, b0, b1 = a & EPS, a >> 32, b & EPS, b >> 32
    p00 = a0 * b0
    t = a0 * b1 + (p00 >> 32)
    u = a1 * b0 + (t & EPS)
    assert t <= M64 and u <= M64
    hi = a1 * b1 + ((t >> 32) + (u >> 32))
    assert hi <= M64
    lo = ((u & EPS) << 32) | (p00 & EPS)
    return lo, hi


def m_reduce128(lo, hi):
    h0, h1 = hi & EPS, hi >> 32
    t0, br = sub64b(lo, h1)
    if br:
        t0 = (t0 - EPS) & M64
    t1 = ((h0 << 32) - h0) & M64
    r, c = add64c(t0, t1)
    if c:
        r = (r + EPS) & M64
    v, (cn,) = m_canon(r)
    return v, (br, c, cn)


def m_mul(a, b):
    lo, hi = m_mul128(a, b)
    return m_reduce128(lo, hi)


def m_from_i64(x):
    return (x if x >= 0 else P - (-x)), (int(x >= 0),)


def m_pow(b, e):
    r = 1
    while e:
        if e & 1:
            r = m_mul(r, b)[0]
        b = m_mul(b, b)[0]
        e >>= 1
    return r


def m_inv(a):
    sq = lambda x: m_mul(x, x)[0]
    mul = lambda x, y: m_mul(x, y)[0]

    def pow2k(x, k):
        for _ in range(k):
            x = sq(x)
        return x
    t2 = mul(sq(a), a)
    t4 = mul(pow2k(t2, 2), t2)
    t8 = mul(pow2k(t4, 4), t4)
    t16 = mul(pow2k(t8, 8), t8)
    t24 = mul(pow2k(t16, 8), t8)
    t28 = mul(pow2k(t24, 4), t4)
    t30 = mul(pow2k(t28, 2), t2)
    t31 = mul(sq(t30), a)
    t32 = mul(sq(t31), a)
    hi = pow2k(sq(t31), 32)
    return mul(hi, t32)


def _mul_eps32(h):
    return ((h << 32) - h) & M64


def m_mul2e_lo(x, e):
    if e == 0:
        return x, ("id",)
    A = (x << e) & M64
    y2 = (x >> (64 - e)) & EPS
    return m_add(A, _mul_eps32(y2))


def m_mul2e(x, e):
    if e < 32:
        return m_mul2e_lo(x, e)
    if e < 64:
        r = e - 32
        A = (x << r) & M64 if r else x
        y2 = (x >> (64 - r)) & EPS if r else 0
        t, p1 = m_add((A << 32) & M64, _mul_eps32(A >> 32))
        if not r:
            return t, p1
        v, p2 = m_sub(t, y2)
        return v, p1 + p2
    y, p0 = m_mul2e_lo(x, e - 64)
    t, p1 = m_add((y << 32) & M64, _mul_eps32(y >> 32))
    v, p2 = m_sub(t, y)
    return v, p0 + p1 + p2


def m_mul_pow2(x, e):
    """(x 2^e mod p, signature): the signature is (e mod 96, the carry / borrow
    outcomes of the inner gl_add / gl_sub calls, and for e >= 96 gl_neg's
    zero test)."""
    if e >= 96:
        v, p = m_mul2e(x, e - 96)
        w, pn = m_neg(v)
        return w, (e - 96, p, pn)
    v, p = m_mul2e(x, e)
    return v, (e, p)


def tw_exp(inv, j, h):
    return ((114 if inv else 78) * j * (16 // h)) % 192


def tw_exp64(inv, j):
    return ((153 if inv else 39) * j) % 192


def pow2_signatures(xs, e):
    return {m_mul_pow2(x, e)[1] for x in xs}


# -------------------------------------------------- register butterflies
def _bitrev(x, m):
    r = 0
    for i in range(m):
        r |= ((x >> i) & 1) << (m - 1 - i)
    return r


def dit_stages(x, root, skip=0):
    """Radix-2 DIT stages skip .. log2(len) - 1 over x (bit-reversed input,
    natural output when skip == 0) with w_{2h}^j = root^(j len / 2h)."""
    n = len(x)
    x = list(x)
    s, h = skip, 1 << skip
    while h < n:
        for t0 in range(n):
            if not t0 & h:
                w = pow(root, (t0 & (h - 1)) * (n // (2 * h)), P)
                a, y = x[t0], x[t0 + h] * w % P
                x[t0], x[t0 + h] = (a + y) % P, (a - y) % P
        s, h = s + 1, h << 1
    return x


def dft_bitrev_in(x, root):
    """O(n^2) sum: out[k] = sum_pos x[pos] root^(bitrev(pos) k)."""
    n = len(x)
    m = n.bit_length() - 1
    return [sum(x[pos] * pow(root, _bitrev(pos, m) * k, P) for pos in range(n)) % P for k in range(n)]


def dft_bitrev_out(x, root):
    """O(n^2) sum: out[bitrev(k)] = sum_j x[j] root^(j k)."""
    n = len(x)
    m = n.bit_length() - 1
    out = [0] * n
    for k in range(n):
        out[_bitrev(k, m)] = sum(x[j] * pow(root, j * k, P) for j in range(n)) % P
    return out


# ------------------------------------------------- the device-check library
def load_devcheck(path):
    """lib/libsezkp_devcheck.so with its argument types (tests/devcheck/devcheck.hip).
    Device addresses are passed as integers (torch's data_ptr())."""
    lib = C.CDLL(path)
    u64, i32, ptr = C.c_uint64, C.c_int, C.c_void_p
    sig = {
        "sezkp_dc_unary": [i32, ptr, ptr, u64],
        "sezkp_dc_binary": [i32, ptr, ptr, ptr, u64],
        "sezkp_dc_mul128": [ptr, ptr, ptr, ptr, u64],
        "sezkp_dc_reduce128": [ptr, ptr, ptr, u64],
        "sezkp_dc_mul_pow2_ct": [ptr, ptr, u64],
        "sezkp_dc_mul_pow2_rt": [ptr, ptr, ptr, u64],
        "sezkp_dc_tw_small": [i32, ptr, ptr, i32, ptr, u64],
        "sezkp_dc_tw64": [i32, ptr, ptr, ptr, u64],
        "sezkp_dc_fft_regs": [i32, i32, i32, i32, ptr, ptr, u64],
        "sezkp_dc_fold": [u64, u64, i32, u64, u64],
        "sezkp_dc_foldm": [u64, ptr, u64, i32, i32],
        "sezkp_dc_fri_tail": [u64, i32, u64, ptr, ptr, ptr, i32],
        "sezkp_dc_forest16": [i32, ptr, ptr, ptr, ptr, ptr, i32, i32, i32, u64, i32, u64, ptr, ptr, ptr, i32, u64],
        "sezkp_dc_layer16": [u64, u64, i32, i32, u64, u64, u64, u64, i32, i32, i32],
        "sezkp_dc_upper_jobs": [u64, u64, i32, i32, i32, i32, u64, u64, i32, ptr],
        "sezkp_dc_leaf_subtree": [u64, u64, i32, i32, u64, u64, u64, u64, i32],
        "sezkp_dc_tree_upper": [u64, u64, i32, i32, i32, u64, u64, i32],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.entry_points = sorted(sig)
    return lib
