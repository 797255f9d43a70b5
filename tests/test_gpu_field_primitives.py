"""The inline device functions of csrc/dev_common.h and csrc/gl_pow2.h, one
at a time on the GPU (lib/libsezkp_devcheck.so, tests/devcheck/devcheck.hip),
against Python-integer arithmetic mod p. Operands: the designed sets of
tests/field_cases.py (tests/test_field_cases.py proves on the CPU that they
take every branch path) together with seeded random ones. Everything compared
is an exact integer; where a function's contract says canonical, the result
must be < p, which equality with `% p` implies.
"""
import os
import random

import numpy as np
import pytest

import field_cases as F
from conftest import PKG

pytestmark = pytest.mark.gpu
P, EPS, M64 = F.P, F.EPS, F.M64
NRAND = 20000
U_CANON, U_NEG, U_SQR, U_INV, U_FROM_I64 = range(5)
B_ADD, B_SUB, B_MUL, B_POW = range(4)


@pytest.fixture(scope="module")
def dc(gpu_ok):
    return F.load_devcheck(os.path.join(PKG, "lib", "libsezkp_devcheck.so"))


def _dev(torch, xs, dtype=np.uint64):
    a = np.array(xs, dtype=dtype)
    return torch.from_numpy(a.view(np.int64) if dtype == np.uint64 else a).cuda()


def _out(torch, n):
    return torch.zeros(max(int(n), 1), dtype=torch.int64, device="cuda")


def _host(t, n):
    return t.cpu().numpy().view(np.uint64)[:n]


def _same(got, want, describe):
    want = np.array(want, dtype=np.uint64)
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d mismatches, first at %d: got %#x want %#x (%s)" % (
        bad.size, bad[0], int(got[bad[0]]), int(want[bad[0]]), describe(int(bad[0])))


def _unary(torch, dc, op, xs):
    x, out = _dev(torch, xs), _out(torch, len(xs))
    assert dc.sezkp_dc_unary(op, x.data_ptr(), out.data_ptr(), len(xs)) == 0
    return _host(out, len(xs))


def _binary(torch, dc, op, pairs):
    a, b, out = _dev(torch, [p[0] for p in pairs]), _dev(torch, [p[1] for p in pairs]), _out(torch, len(pairs))
    assert dc.sezkp_dc_binary(op, a.data_ptr(), b.data_ptr(), out.data_ptr(), len(pairs)) == 0
    return _host(out, len(pairs))


@pytest.fixture(scope="module")
def canon():
    return F.canonical_designed()


@pytest.fixture(scope="module")
def canon_pairs(canon):
    rnd = F.seeded(2 * NRAND, 11)
    return [(a, b) for a in canon for b in F.EDGE] + [(b, a) for a in canon for b in F.EDGE] + \
        list(zip(rnd[::2], rnd[1::2]))


def test_gl_add_sub_canonical_operands(gpu_ok, dc, canon_pairs):
    pr = canon_pairs
    _same(_binary(gpu_ok, dc, B_ADD, pr), [(a + b) % P for a, b in pr], lambda i: "gl_add%r" % (pr[i],))
    _same(_binary(gpu_ok, dc, B_SUB, pr), [(a - b) % P for a, b in pr], lambda i: "gl_sub%r" % (pr[i],))


def test_gl_add_any_word_plus_h_eps_is_canonical(gpu_ok, dc):
    """The envelope the shift twiddles rely on: gl_add(A, h eps) = (A + h eps)
    mod p, canonical, for ANY word A and h < 2^32. Outside it (B < p in
    general) gl_add is not canonical: the device returns what the mirror says
    for A = 2^64 - 1, B = p - 1."""
    rng = random.Random(12)
    pr = F.add_envelope_designed() + [(rng.randrange(1 << 64), rng.randrange(1 << 32) * EPS) for _ in range(NRAND)]
    got = _binary(gpu_ok, dc, B_ADD, pr)
    _same(got, [(a + b) % P for a, b in pr], lambda i: "gl_add%r" % (pr[i],))
    assert int(got.max()) < P
    assert int(_binary(gpu_ok, dc, B_ADD, [(M64, P - 1)])[0]) == F.m_add(M64, P - 1)[0] == M64 - 1


def test_gl_canon_neg_from_i64(gpu_ok, dc, canon):
    rng = random.Random(13)
    a64 = F.any64_designed() + [rng.randrange(1 << 64) for _ in range(NRAND)]
    _same(_unary(gpu_ok, dc, U_CANON, a64), [x % P for x in a64], lambda i: "gl_canon(%#x)" % a64[i])
    cs = canon + F.seeded(NRAND, 14)
    _same(_unary(gpu_ok, dc, U_NEG, cs), [-x % P for x in cs], lambda i: "gl_neg(%#x)" % cs[i])
    iv = F.I64_EDGE + [rng.randrange(-(1 << 63) + 1, 1 << 63) for _ in range(NRAND)]
    got = _unary(gpu_ok, dc, U_FROM_I64, [x & M64 for x in iv])
    _same(got, [x % P for x in iv], lambda i: "gl_from_i64(%d)" % iv[i])


@pytest.fixture(scope="module")
def mul_pairs():
    rng = random.Random(15)
    return F.mul_pairs_designed() + [(rng.randrange(1 << 64), rng.randrange(1 << 64)) for _ in range(NRAND)] + \
        list(zip(F.seeded(NRAND, 16), F.seeded(NRAND, 17)))


def test_gl_mul128_mul_sqr(gpu_ok, dc, mul_pairs):
    """Any a, b < 2^64 -> the exact 128-bit product and the canonical a b mod
    p, over all six (borrow, carry, canon) paths of the reduction (the named
    products of field_cases.MUL_NAMED among them)."""
    torch, pr, n = gpu_ok, mul_pairs, len(mul_pairs)
    a, b = _dev(torch, [p[0] for p in pr]), _dev(torch, [p[1] for p in pr])
    lo, hi = _out(torch, n), _out(torch, n)
    assert dc.sezkp_dc_mul128(a.data_ptr(), b.data_ptr(), lo.data_ptr(), hi.data_ptr(), n) == 0
    _same(_host(lo, n), [(x * y) & M64 for x, y in pr], lambda i: "gl_mul128 lo %r" % (pr[i],))
    _same(_host(hi, n), [(x * y) >> 64 for x, y in pr], lambda i: "gl_mul128 hi %r" % (pr[i],))
    _same(_binary(torch, dc, B_MUL, pr), [x * y % P for x, y in pr], lambda i: "gl_mul%r" % (pr[i],))
    for name, (x, y) in F.MUL_NAMED.items():
        assert int(_binary(torch, dc, B_MUL, [(x, y)])[0]) == x * y % P, name
    sq = [p[0] for p in pr]
    _same(_unary(torch, dc, U_SQR, sq), [x * x % P for x in sq], lambda i: "gl_sqr(%#x)" % sq[i])


def test_gl_reduce128_raw_words(gpu_ok, dc):
    torch = gpu_ok
    rng = random.Random(18)
    pr = F.reduce_pairs_designed() + [(rng.randrange(1 << 64), rng.randrange(1 << 64)) for _ in range(NRAND)]
    # tiny lo under a random hi: the borrow, which random (lo, hi) reach with probability 2^-32
    pr += [(rng.randrange(4), rng.randrange(1 << 64)) for _ in range(2000)]
    pr += [(rng.randrange(1 << 32), (rng.randrange(1 << 32) << 32) | rng.randrange(2)) for _ in range(2000)]
    n = len(pr)
    lo, hi, out = _dev(torch, [p[0] for p in pr]), _dev(torch, [p[1] for p in pr]), _out(torch, n)
    assert dc.sezkp_dc_reduce128(lo.data_ptr(), hi.data_ptr(), out.data_ptr(), n) == 0
    _same(_host(out, n), [((h << 64) | l) % P for l, h in pr], lambda i: "gl_reduce128%r" % (pr[i],))


def test_gl_inv_and_pow(gpu_ok, dc, canon):
    """gl_inv(0) = 0 (0^(p-2)), a value like any other; gl_pow_dev for any
    exponent word."""
    xs = [0] + canon + F.NONCANON + F.seeded(4000, 19)
    _same(_unary(gpu_ok, dc, U_INV, xs), [pow(x, P - 2, P) for x in xs], lambda i: "gl_inv(%#x)" % xs[i])
    rng = random.Random(20)
    es = [0, 1, 2, 3, 2047, 2048, 4095, 4096, P - 2, P - 1, P, M64, 1 << 63, EPS]
    pr = [(b, e) for b in F.EDGE + F.NONCANON for e in es] + [(rng.randrange(P), rng.randrange(1 << 64)) for _ in range(4000)]
    _same(_binary(gpu_ok, dc, B_POW, pr), [pow(b, e, P) for b, e in pr], lambda i: "gl_pow_dev%r" % (pr[i],))


@pytest.fixture(scope="module")
def shift_operands(canon):
    return canon + F.seeded(600, 21)


def test_gl_mul_pow2_every_exponent_compile_time(gpu_ok, dc, shift_operands):
    """gl_mul_pow2(x, E), E = 0..191 a template argument (the form the unrolled
    butterflies see), over the designed operands that reach every signature."""
    torch, xs, n = gpu_ok, shift_operands, len(shift_operands)
    x, out = _dev(torch, xs), _out(torch, 192 * n)
    assert dc.sezkp_dc_mul_pow2_ct(x.data_ptr(), out.data_ptr(), n) == 0
    want = [v * pow(2, e, P) % P for e in range(192) for v in xs]
    _same(_host(out, 192 * n), want, lambda i: "gl_mul_pow2<%d>(%#x)" % (i // n, xs[i % n]))


def test_gl_mul_pow2_every_exponent_run_time(gpu_ok, dc, shift_operands):
    torch, xs = gpu_ok, shift_operands
    n = len(xs)
    es = [e for e in range(192) for _ in range(n)]
    vs = xs * 192
    x, e, out = _dev(torch, vs), _dev(torch, es, np.int32), _out(torch, len(vs))
    assert dc.sezkp_dc_mul_pow2_rt(x.data_ptr(), e.data_ptr(), out.data_ptr(), len(vs)) == 0
    want = [v * pow(2, k, P) % P for v, k in zip(vs, es)]
    _same(_host(out, len(vs)), want, lambda i: "gl_mul_pow2(%#x, %d)" % (vs[i], es[i]))


@pytest.fixture(scope="module")
def roots():
    """The oracle's roots of unity, after checking they are the powers of two
    the shift twiddles assume: w_32 = 2^78, w_64 = 2^39 (2 has order 192)."""
    import sezkp_oracle_py as O
    assert O.root_2exp(5) == pow(2, 78, P) and O.root_2exp(6) == pow(2, 39, P)
    assert pow(O.root_2exp(5), -1, P) == pow(2, 114, P) and pow(O.root_2exp(6), -1, P) == pow(2, 153, P)
    for k in range(1, 6):
        assert O.root_2exp(k) == pow(2, (78 << (5 - k)) % 192, P)
    return {k: O.root_2exp(k) for k in range(1, 7)}


@pytest.mark.parametrize("inv", [0, 1])
def test_tw_small_and_tw_exp64(gpu_ok, dc, roots, canon, inv):
    """tw_small<INV>(x, j, h) = x w_{2h}^(+-j) for h = 1..16 and
    gl_mul_pow2(x, tw_exp64<INV>(j)) = x w_64^(+-j), the roots the oracle's."""
    torch = gpu_ok
    rng = random.Random(22 + inv)
    xs = canon + F.seeded(300, 23)
    for h in (1, 2, 4, 8, 16):
        w = roots[(2 * h).bit_length() - 1]
        w = pow(w, -1, P) if inv else w
        js = list(range(2 * h)) + [1, 7, 15 * 7, 127]
        vs = [x for x in xs for _ in js]
        jj = [j for _ in xs for j in js]
        x, j, out = _dev(torch, vs), _dev(torch, jj, np.int32), _out(torch, len(vs))
        assert dc.sezkp_dc_tw_small(inv, x.data_ptr(), j.data_ptr(), h, out.data_ptr(), len(vs)) == 0
        _same(_host(out, len(vs)), [v * pow(w, k, P) % P for v, k in zip(vs, jj)],
              lambda i: "tw_small<%d>(%#x, %d, %d)" % (inv, vs[i], jj[i], h))
    w = pow(roots[6], -1, P) if inv else roots[6]
    js = list(range(64)) + [63 * 7, 7 * 7, 100] + [rng.randrange(442) for _ in range(8)]
    vs = [x for x in xs for _ in js]
    jj = [j for _ in xs for j in js]
    x, j, out = _dev(torch, vs), _dev(torch, jj, np.int32), _out(torch, len(vs))
    assert dc.sezkp_dc_tw64(inv, x.data_ptr(), j.data_ptr(), out.data_ptr(), len(vs)) == 0
    _same(_host(out, len(vs)), [v * pow(w, k, P) % P for v, k in zip(vs, jj)],
          lambda i: "tw_exp64<%d>(%#x, %d)" % (inv, vs[i], jj[i]))


def _vectors(logf, seed):
    """Batches of 2^logf-element vectors: edge-heavy, constant p - 1, single
    spikes, random; more than one workgroup of lanes."""
    n = 1 << logf
    rng = random.Random(seed)
    vecs = [[P - 1] * n, [0] * n, [1] * n]
    vecs += [[(P - 1 if k == s else 0) for k in range(n)] for s in range(n)]
    vecs += [[rng.choice(F.EDGE) for _ in range(n)] for _ in range(150)]
    vecs += [[rng.choice(F.EDGE) if rng.random() < 0.5 else rng.randrange(P) for _ in range(n)] for _ in range(60)]
    vecs += [[rng.randrange(P) for _ in range(n)] for _ in range(60)]
    assert len(vecs) > 256
    return vecs


def _run_fft(torch, dc, dif, logf, inv, skip, vecs):
    flat = [v for vec in vecs for v in vec]
    x, out = _dev(torch, flat), _out(torch, len(flat))
    assert dc.sezkp_dc_fft_regs(dif, logf, inv, skip, x.data_ptr(), out.data_ptr(), len(vecs)) == 0
    return _host(out, len(flat)).reshape(len(vecs), 1 << logf)


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("logf", [3, 4])
def test_fft_dit_regs(gpu_ok, dc, roots, logf, inv):
    """fft_dit_regs<LOGF, INV, SKIP>: SKIP = 0 against the O(n^2) DFT sum over
    the bit-reversed input (no 1/n for INV), SKIP > 0 against the product of
    the remaining stage matrices, both from the oracle's root of order 2^LOGF."""
    root = pow(roots[logf], -1, P) if inv else roots[logf]
    vecs = _vectors(logf, 30 + logf)
    for skip in range(4):
        got = _run_fft(gpu_ok, dc, 0, logf, inv, skip, vecs)
        want = [F.dft_bitrev_in(v, root) if skip == 0 else F.dit_stages(v, root, skip) for v in vecs]
        _same(got.reshape(-1), [x for w in want for x in w],
              lambda i: "fft_dit_regs<%d,%d,%d> vector %d slot %d" % (logf, inv, skip, i >> logf, i & ((1 << logf) - 1)))


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("logf", [2, 3, 4])
def test_fft_dif_regs(gpu_ok, dc, roots, logf, inv):
    """fft_dif_regs<LOGF, INV>: natural in, bit-reversed out, against the
    O(n^2) DFT sum (no 1/n for INV)."""
    root = pow(roots[logf], -1, P) if inv else roots[logf]
    vecs = _vectors(logf, 40 + logf)
    got = _run_fft(gpu_ok, dc, 1, logf, inv, 0, vecs)
    want = [F.dft_bitrev_out(v, root) for v in vecs]
    _same(got.reshape(-1), [x for w in want for x in w],
          lambda i: "fft_dif_regs<%d,%d> vector %d slot %d" % (logf, inv, i >> logf, i & ((1 << logf) - 1)))
