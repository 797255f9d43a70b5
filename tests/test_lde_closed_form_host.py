"""The closed-form first stages of the DEEP-polynomial LDE (DeepPoly,
csrc/sezkp_internal.h) on the CPU.

The first b = log(E/n) DIT stages of the LDE's first pass combine the 2^b
inputs of one group, positions 2^b g + s. A Python model of those stages, with
the kernel's own butterflies (fft_dit_regs: bit-reversed in, natural out, the
twiddle of stage h a power of two, 2^(78 j 16/h) = w_{2h}^j) runs on the inputs
the point-by-point load forms,

    slot s:  [t = 0] qv + c' rho^(e0 + t n) - [t = 0] kappa rho^e0,  t = bitrev_b(s),

and must equal qv + rho^e0 (c' G[s] - kappa) with
G[s] = sum_{t < 2^b} (rho^n w_{2^b}^s)^t, which is what dp_load_closed forms
from the constants of deep_constants (checked here through the sanitized
tools/proof_host_check.cpp against the same formula in Python integers).
"""
import itertools
import json
import os
import random
import subprocess

import pytest

from conftest import PKG, ROOT

P = 2**64 - 2**32 + 1
EDGE = [P - 1, 1, 2**32 - 1, 2**63]


def tw_exp(j, h):  # gl_pow2.h, forward
    return (78 * j * (16 // h)) % 192


def dit_stages(x, b):
    """fft_dit_regs<LOGF, false, 0> cut after its first b stages (in place)."""
    x = list(x)
    for s in range(b):
        h = 1 << s
        for t0 in range(len(x)):
            if t0 & h:
                continue
            j = t0 & (h - 1)
            y = x[t0 + h] * pow(2, tw_exp(j, h), P) % P
            a = x[t0]
            x[t0], x[t0 + h] = (a + y) % P, (a - y) % P
    return x


def bitrev(v, bits):
    return int(format(v, "0%db" % bits)[::-1], 2) if bits else 0


def G_of(rho_n, b):
    w = pow(7, (P - 1) >> b, P)
    return [sum(pow(rho_n * pow(w, s, P) % P, t, P) for t in range(1 << b)) % P for s in range(1 << b)]


def test_register_twiddles_are_the_field_roots():
    # 2 has order 192 and 2^78 = w_32: the stages below use the transform's own roots
    assert pow(2, 192, P) == 1 and pow(2, 96, P) == P - 1
    assert pow(2, 78, P) == pow(7, (P - 1) >> 5, P)
    for h in (1, 2, 4, 8):
        for j in range(h):
            assert pow(2, tw_exp(j, h), P) == pow(pow(7, (P - 1) // (2 * h), P), j, P)


def cases():
    rnd = random.Random(20)
    out = [tuple(rnd.randrange(P) for _ in range(4)) for _ in range(24)]
    # every edge value in every role, the others random; and all four roles at one edge value
    for i, v in itertools.product(range(4), EDGE):
        c = [rnd.randrange(1, P) for _ in range(4)]
        c[i] = v
        out.append(tuple(c))
    out += [(v, v, v, v) for v in EDGE]
    out += list(itertools.islice(itertools.product(EDGE, repeat=4), 0, 256, 5))
    return out


@pytest.mark.parametrize("b", [1, 2, 3])
def test_first_stages_equal_closed_form(b):
    rnd = random.Random(b)
    for rho, cp, kappa, qv in cases():
        for logn in (4, 13):
            n = 1 << logn
            g = rnd.randrange(n)
            e0 = bitrev(g, logn)
            re0 = pow(rho, e0, P)
            # slot s of group g holds coefficient e = bitrev_{logn + b}(2^b g + s) = e0 + bitrev_b(s) n
            x = []
            for s in range(1 << b):
                t = bitrev(s, b)
                assert bitrev((g << b) + s, logn + b) == e0 + t * n
                v = cp * pow(rho, e0 + t * n, P)
                if t == 0:
                    v += qv - kappa * re0
                x.append(v % P)
            got = dit_stages(x, b)
            G = G_of(pow(rho, n, P), b)
            want = [(qv + re0 * ((cp * G[s] - kappa) % P)) % P for s in range(1 << b)]
            assert got == want, (b, rho, cp, kappa, qv, logn, g)


@pytest.mark.parametrize("b", [1, 2, 3])
def test_stages_of_a_wider_register_fft_stay_inside_the_group(b):
    """The 16-point register FFT's first b stages act on each run of 2^b slots
    alone, so a thread's 16 >> b groups are independent."""
    rnd = random.Random(100 + b)
    x = [rnd.randrange(P) for _ in range(16)]
    got = dit_stages(x, b)
    for g in range(16 >> b):
        assert got[g << b:(g + 1) << b] == dit_stages(x[g << b:(g + 1) << b], b)


RANKS = [(1, 0), (2, 1), (4, 3), (8, 5)]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("lde_closed")
    exe = str(d / "proof_host_check")
    csrc = os.path.join(PKG, "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "proof_host_check.cpp"),
                    os.path.join(csrc, "proof_host.cpp"), os.path.join(csrc, "host_crypto.cpp")], check=True)

    def run(proof, tau, step_start):
        src, dst = str(d / "proof.bin"), str(d / "image.bin")
        with open(src, "wb") as f:
            f.write(proof)
        r = subprocess.run([exe, src, dst, str(tau), ",".join("%d:%d" % pr for pr in RANKS)] +
                           [str(int(x)) for x in step_start], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        return json.loads(r.stdout)

    return run


@pytest.mark.parametrize("n", [16, 4096])
def test_deep_constants_G(host_check, oracle, product, n):
    """deep_constants' Gs for one device (b = 3), P = 2 (every rank evaluates
    the whole domain: b = 3), P = 4 (b = 1) and P = 8 (b = 0: Gs[0] = 1)."""
    tau = 1
    blocks = product.synthetic_blocks(n, min(n, 256), tau, 7)
    L = host_check(oracle.prove_v1(blocks, blocks.manifest_root()), tau, blocks.step_start)
    for d in L["deep"]:
        E = 8 * n if d["full_lde"] or d["P"] == 1 else 8 * n // d["P"]
        b = (E // n).bit_length() - 1
        assert b == {1: 3, 2: 3, 4: 1, 8: 0}[d["P"]]
        assert d["Gs"] == G_of(pow(d["rho"], n, P), b) + [0] * (8 - (1 << b))
