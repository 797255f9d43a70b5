"""The host half of a proof (csrc/proof_host.h) on the CPU, against the
oracle's proofs: the stand-alone tools/proof_host_check.cpp, built with the
address and undefined-behaviour sanitizers and linked with proof_host.cpp and
host_crypto.cpp (no HIP; nothing is loaded into Python), takes from an oracle
proof what the device would send home (column roots, FRI roots, final value,
manifest root), replays the three Fiat-Shamir rounds and writes the
host-written fields into a zeroed image. Every such field must equal the
oracle proof's bytes at the same offsets, and the DEEP constants must equal
Python integer arithmetic mod p."""
import json
import os
import subprocess

import pytest

from conftest import PKG, ROOT

P_GL = 2**64 - 2**32 + 1
NQ = 30
RANKS = [(1, 0), (2, 1), (4, 3), (8, 5)]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("proof_host")
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
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        assert r.stderr == "", r.stderr[-2000:]  # a sanitizer report
        return json.loads(r.stdout), open(dst, "rb").read()

    return run


@pytest.fixture(scope="module")
def replay(host_check, oracle, product):
    """(layout and challenges, image, oracle proof) per (n, tau), computed once."""
    cache = {}

    def get(n, tau):
        if (n, tau) not in cache:
            blocks = product.synthetic_blocks(n, min(n, 256), tau, 7)
            want = oracle.prove_v1(blocks, blocks.manifest_root())
            out, image = host_check(want, tau, blocks.step_start)
            cache[(n, tau)] = (out, image, want)
        return cache[(n, tau)]

    return get


def u64(b, at):
    return int.from_bytes(b[at:at + 8], "little")


@pytest.mark.parametrize("tau", [1, 2])
@pytest.mark.parametrize("n", [1, 16, 1024, 4096])
def test_host_fields_match_oracle(replay, n, tau):
    L, image, want = replay(n, tau)
    assert len(image) == len(want) == L["hdr_bytes"] + L["total"]
    k, hdr = L["k"], L["hdr_bytes"]
    assert (L["n"], L["N"], k) == (n, 8 * n, n.bit_length() - 1 + 3)
    host = []  # (offset in the body, length) of every host-written field

    def same(at, ln, what):
        assert image[hdr + at:hdr + at + ln] == want[hdr + at:hdr + at + ln], (what, at)
        host.append((at, ln))

    same(0, 8, "query count")
    assert u64(want, hdr) == NQ
    for q in range(NQ):
        same(8 + q * L["q_bytes"], 16, "rows[%d] and tau" % q)
        assert u64(image, hdr + 8 + q * L["q_bytes"]) == L["rows"][q] < n
        assert u64(image, hdr + 8 + q * L["q_bytes"] + 8) == tau
    same(L["fr_off"], 8 + 32 * (k + 1), "FRI roots block")
    assert u64(image, hdr + L["fr_off"]) == k + 1
    same(L["fq_off"], 8, "FRI query count")
    for q in range(NQ):
        at = L["fq_off"] + 8 + q * L["fq_bytes"]
        same(at, 8 + 8 * (k + 1), "k + 1 and the positions of query %d" % q)
        same(at + 8 + 8 * (k + 1), 8, "k of query %d" % q)
        assert u64(image, hdr + at + 8) == L["frows"][q] < 8 * n
    same(L["tail_off"], 40, "final value and manifest root")
    assert L["tail_off"] + 40 == L["total"]
    # the header with its column roots, and nothing written outside the host's fields
    assert image[:hdr] == want[:hdr]
    body = bytearray(image[hdr:])
    for at, ln in host:
        body[at:at + ln] = bytes(ln)
    assert not any(body)
    # the requests of the single device: every path record and every opening
    assert (L["nf"], L["no"]) == (NQ * 2 * k, NQ * (9 * tau + 3))


@pytest.mark.parametrize("tau", [1, 2])
@pytest.mark.parametrize("n", [1, 16, 1024, 4096])
def test_deep_constants_match_integer_arithmetic(replay, n, tau):
    L, _, _ = replay(n, tau)
    p, N, k, z = P_GL, 8 * n, L["k"], L["z"]
    inv = lambda x: pow(x, p - 2, p)
    assert 0 < z < p and pow(z * inv(3) % p, N, p) != 1  # the nudge: z off the LDE coset
    assert L["zn"] == pow(z, n, p)
    assert all(0 <= x < p for x in L["alpha"] + L["mask"] + L["beta"]) and len(L["beta"]) == k
    w_N = pow(7, (p - 1) >> k, p)
    assert [(d["P"], d["rank"]) for d in L["deep"]] == RANKS
    for d in L["deep"]:
        P, g = d["P"], d["rank"]
        assert d["full_lde"] == int(P == 2)  # plan_shape: sharded and P = 2
        cP, cg = (1, 0) if d["full_lde"] else (P, g)  # the coset this rank evaluates
        rho = 3 * inv(z) * pow(w_N, cg, p) % p
        G = sum(pow(rho, t * (N // cP), p) for t in range(cP)) % p
        assert d["rho"] == rho and d["rho4096"] == pow(rho, 4096, p)
        assert d["K1"] == (1 - pow(z, n, p)) * inv(n) % p
        assert d["K2"] == pow(z, N - 1, p) * inv((pow(3, N, p) - pow(z, N, p)) % p) * G % p
        assert d["K3"] == pow(z, n - 1, p) * inv(n) % p


def test_challenges_match_python_transcript(replay):
    """One case replayed by the oracle's pure-Python transcript: the values
    that go into the challenge record (alphas, mask, z, betas) and the query
    rows, not only their ranges."""
    import sezkp_oracle_py as py
    n, tau = 16, 2
    L, _, want = replay(n, tau)
    p, k, hdr = P_GL, L["k"], L["hdr_bytes"]
    # the header: N, tau, ncols, then (label length, label, root) per column
    assert (u64(want, 0), u64(want, 8)) == (8 * n, tau)
    ncols, at, colroots = u64(want, 16), 24, []
    for _ in range(ncols):
        at += 8 + u64(want, at)
        colroots.append(want[at:at + 32])
        at += 32
    assert at == hdr and ncols == 3 + 7 * tau
    roots = [want[hdr + L["fr_off"] + 8 + 32 * r:hdr + L["fr_off"] + 40 + 32 * r] for r in range(k + 1)]
    mroot = want[hdr + L["tail_off"] + 8:hdr + L["tail_off"] + 40]
    le = lambda b, i: int.from_bytes(b[8 * i:8 * i + 8], "little")
    tr = py.Transcript("sezkp-stark/v1")
    tr.absorb("manifest_root", mroot)
    tr.absorb_u64("n", n)
    tr.absorb_u64("tau", tau)
    tr.absorb_u64("n_cols", ncols)
    for r in colroots:
        tr.absorb("col_root", r)
    ab = tr.challenge("alphas", 64)
    assert L["alpha"] == [le(ab, i) % p for i in range(8)]
    tr.absorb("masks", b"masks")
    tr.absorb_u64("n_masks", 1)
    tr.absorb_u64("deg", 4)
    assert L["mask"] == [le(tr.challenge("mask_coeff", 8), 0) % p for _ in range(4)]
    z = le(tr.challenge("ood_point", 8), 0) % p
    while pow(z * pow(3, p - 2, p) % p, 8 * n, p) == 1:
        z = (z + 1) % p
    assert L["z"] == z
    tr.absorb("fri_layer_root", roots[0])
    bb = tr.challenge("fri_betas", 8 * k)
    assert L["beta"] == [le(bb, r) % p for r in range(k)]
    for r in range(1, k + 1):
        tr.absorb("fri_layer_root", roots[r])
    qb = tr.challenge("row_queries", 8 * NQ)
    assert L["rows"] == [le(qb, i) % n for i in range(NQ)]
    fb = tr.challenge("row_queries", 8 * NQ)
    assert L["frows"] == [le(fb, i) % (8 * n) for i in range(NQ)]
