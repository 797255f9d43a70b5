"""CPU side of the device field-primitive tests: the Python mirrors of
tests/field_cases.py are the device functions' arithmetic, and the designed
operands reach every branch path of them. These are conditions on the test
inputs, so the GPU tests (test_gpu_field_primitives.py) cannot quietly skip a
branch: what they feed the kernels is shown here to take every path.
"""
import os

import pytest

import field_cases as F
from conftest import PKG

P = F.P
DEVCHECK = os.path.join(PKG, "lib", "libsezkp_devcheck.so")


@pytest.fixture(scope="module")
def canon():
    return F.canonical_designed()


def test_designed_sets_are_what_they_claim(canon):
    assert set(F.EDGE) <= set(canon) and all(0 <= x < P for x in canon)
    a64 = F.any64_designed()
    assert set(F.NONCANON) <= set(a64) and all(0 <= x < 1 << 64 for x in a64)
    for k in range(64):
        assert {(1 << k) % P, ((1 << k) + 1) % P, ((1 << k) - 1) % P, (P - (1 << k)) % P} <= set(canon)
    for a, b in F.mul_pairs_designed() + F.reduce_pairs_designed() + F.add_envelope_designed():
        assert 0 <= a < 1 << 64 and 0 <= b < 1 << 64
    assert all(b <= F.EPS * F.EPS for _, b in F.add_envelope_designed())
    assert all(-(1 << 63) < x < (1 << 63) for x in F.I64_EDGE)


def test_mirror_is_modular_arithmetic(canon):
    rnd = F.seeded(300, 1)
    vals = canon + rnd
    small = F.EDGE + rnd[:20]
    for a in vals:
        assert F.m_canon(a)[0] == a % P and F.m_neg(a)[0] == -a % P
        for b in small:
            assert F.m_add(a, b)[0] == (a + b) % P
            assert F.m_sub(a, b)[0] == (a - b) % P
    for r in F.any64_designed():
        assert F.m_canon(r)[0] == r % P
    for a, b in F.mul_pairs_designed() + list(zip(rnd, reversed(rnd))):
        lo, hi = F.m_mul128(a, b)
        assert (hi << 64) | lo == a * b
        assert F.m_mul(a, b)[0] == a * b % P
    for lo, hi in F.reduce_pairs_designed():
        assert F.m_reduce128(lo, hi)[0] == ((hi << 64) | lo) % P
    for a, b in F.add_envelope_designed():
        assert F.m_add(a, b)[0] == (a + b) % P  # canonical although a is any word
    assert F.m_add((1 << 64) - 1, P - 1)[0] == (1 << 64) - 2  # outside the envelope gl_add is not canonical
    for x in F.I64_EDGE:
        assert F.m_from_i64(x)[0] == x % P
    for a in F.EDGE + F.NONCANON + rnd[:10]:
        assert F.m_inv(a) == pow(a, P - 2, P)
        for e in (0, 1, 2, P - 2, P - 1, (1 << 64) - 1, 2048 * 5 + 3):
            assert F.m_pow(a, e) == pow(a, e, P)
    assert F.m_inv(0) == 0


def test_shift_mirror_is_modular_arithmetic(canon):
    vals = canon + F.seeded(50, 2)
    for e in range(192):
        k = pow(2, e, P)
        for x in vals:
            assert F.m_mul_pow2(x, e)[0] == x * k % P
    assert pow(2, 192, P) == 1 and pow(2, 96, P) == P - 1
    for inv in (0, 1):
        for h in (1, 2, 4, 8, 16):
            w = pow(2, 114 if inv else 78, P)  # w_32^-1, w_32
            for j in range(0, 130):
                assert pow(2, F.tw_exp(inv, j, h), P) == pow(w, j * (16 // h), P)
        for j in range(0, 450):
            assert pow(2, F.tw_exp64(inv, j), P) == pow(2, (153 if inv else 39) * j, P)


def test_designed_operands_reach_every_primitive_path(canon):
    """gl_add: 3 reachable paths (both carries cannot happen together for
    canonical operands), gl_sub 2, gl_canon 2, gl_mul all 6 (borrow, carry,
    canon) paths: a carry leaves r < 2^64 - 2^32 + eps < p, so (., 1, 1) does
    not exist."""
    assert {F.m_add(a, b)[1] for a in canon for b in F.EDGE} == {(0, 0), (0, 1), (1, 0)}
    assert {F.m_add(a, b)[1] for a, b in F.add_envelope_designed()} == {(0, 0), (0, 1), (1, 0)}
    assert {F.m_sub(a, b)[1] for a in canon for b in F.EDGE} == {(0,), (1,)}
    assert {F.m_canon(r)[1] for r in F.any64_designed()} == {(0,), (1,)}
    assert {F.m_neg(a)[1] for a in canon} == {(0,), (1,)}
    assert {F.m_from_i64(x)[1] for x in F.I64_EDGE} == {(0,), (1,)}
    six = {(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0)}
    assert {F.m_mul(a, b)[1] for a, b in F.mul_pairs_designed()} == six
    assert {F.m_reduce128(lo, hi)[1] for lo, hi in F.reduce_pairs_designed()} == six
    for name, (a, b) in F.MUL_NAMED.items():
        br, c, n = F.m_mul(a, b)[1]
        assert name.startswith("b%d_c%d_n%d" % (br, c, n)), name
    # what random data reaches: two of the six (the borrow needs lo < hi >> 32)
    rnd = F.seeded(20000, 3)
    assert {F.m_mul(a, b)[1] for a, b in zip(rnd[::2], rnd[1::2])} < six


def test_designed_operands_reach_every_shift_signature(canon):
    """For every e in 0..191 the designed operands reach every (e mod 96, inner
    add / sub path, gl_neg zero test) signature of gl_mul_pow2 that the designed
    set together with 10^4 seeded random operands reaches.

    Counts found by the mirror: 914 signatures over e = 0..191 (with gl_neg's
    zero test), 409 distinct (e mod 96, add / sub path) ones; the designed set
    reaches all of them, the 10^4 random operands per e alone reach 370 of the 914."""
    total, proj, rnd_only = 0, set(), 0
    for e in range(192):
        designed = F.pow2_signatures(canon, e)
        rnd = F.pow2_signatures(F.seeded(10000, 1000 + e), e)
        assert rnd <= designed, (e, sorted(rnd - designed))
        total += len(designed)
        rnd_only += len(rnd)
        proj |= {s[:2] for s in designed}
    print("gl_mul_pow2 signatures: %d over e = 0..191, %d distinct (e mod 96, path); random alone reaches %d"
          % (total, len(proj), rnd_only))
    assert rnd_only < total
    assert len(proj) >= 96 and total >= 192


def test_butterfly_references_agree():
    """The stage-matrix product with skip = 0 is the O(n^2) DFT sum."""
    import sezkp_oracle_py as O
    for logf in (2, 3, 4):
        root = O.root_2exp(logf)
        x = F.seeded(1 << logf, 40 + logf)
        assert F.dit_stages(x, root) == F.dft_bitrev_in(x, root)
        nat = [x[F._bitrev(i, logf)] for i in range(1 << logf)]
        assert F.dft_bitrev_in(x, root) == O.dft(nat, root)
        br = F.dft_bitrev_out(nat, root)
        assert [br[F._bitrev(k, logf)] for k in range(1 << logf)] == O.dft(nat, root)


def test_devcheck_library_loads_and_exports():
    assert os.path.exists(DEVCHECK), "lib/libsezkp_devcheck.so is not built (make in the package)"
    lib = F.load_devcheck(DEVCHECK)  # getattr on every entry point: a missing export raises here
    assert len(lib.entry_points) == 17
    exported = set(lib.entry_points)
    assert {"sezkp_dc_unary", "sezkp_dc_mul_pow2_ct", "sezkp_dc_fft_regs", "sezkp_dc_foldm", "sezkp_dc_fri_tail",
            "sezkp_dc_forest16", "sezkp_dc_layer16", "sezkp_dc_upper_jobs", "sezkp_dc_leaf_subtree",
            "sezkp_dc_tree_upper"} <= exported
