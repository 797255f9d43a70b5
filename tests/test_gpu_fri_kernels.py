"""The FRI fold / tail / forest / layer / tree kernels of csrc/fri_fold.hip,
fri_forest.hip and merkle_tree.hip driven
directly through the product's own launchers (lib/libsezkp_devcheck.so), with
boundary values and boundary challenges: what the prover feeds them only by
chance. Values come from the EDGE set with runs of p - 1; betas are the
boundary set {0, 1, p - 1, eps, 2^63, p - 2^32} together with random ones.
Reference: the fold in Python integers, and the oracle's hash_leaf_u64 /
merkle_nodes for every stored tree level and the root. Shapes are the smallest
that select each form.
"""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import field_cases as F
from conftest import PKG

pytestmark = pytest.mark.gpu
P, EPS = F.P, F.EPS
BETAS = [0, 1, P - 1, EPS, 1 << 63, P - (1 << 32)]
LSTORE_FRI = 6
TAIL_MAX = 12
GUARD = 64  # words after every output buffer that must stay untouched
HIP_INVALID_VALUE = 1


@pytest.fixture(scope="module")
def dc(gpu_ok):
    return F.load_devcheck(os.path.join(PKG, "lib", "libsezkp_devcheck.so"))


@functools.lru_cache(maxsize=None)
def values(n, seed):
    """n canonical values: EDGE draws, random ones, and runs of p - 1 (a run
    longer than a lane's 16 leaves, runs across workgroup boundaries)."""
    rng = random.Random(seed)
    v = [rng.choice(F.EDGE) if rng.random() < 0.6 else rng.randrange(P) for _ in range(n)]
    for _ in range(max(2, n // 256)):
        at, ln = rng.randrange(n), rng.choice([1, 2, 3, 17, 40])
        for i in range(at, min(n, at + ln)):
            v[i] = P - 1
    if n >= 2:
        v[n // 2 - 1] = v[n // 2] = P - 1  # a run across the fold's two halves
    return tuple(v)


def fold(y, beta):
    h = len(y) // 2
    return tuple((y[i] + beta * y[i + h]) % P for i in range(h))


@functools.lru_cache(maxsize=None)
def _tree_cached(vals):
    import oracle_ctypes as O
    leaves = b"".join(O.hash_leaf_u64(v) for v in vals)
    return O.merkle_nodes(leaves)


def tree_levels(vals):
    """Every level of the oracle's tree over the u64 leaves, bottom -> top."""
    nodes, n, off, out = _tree_cached(tuple(vals)), len(vals), 0, []
    while True:
        out.append(nodes[32 * off:32 * (off + n)])
        off += n
        if n == 1:
            break
        n //= 2
    assert 32 * off == len(nodes)
    return out


def stored_nodes(logLen, lstore):
    return (1 << (logLen - lstore + 1)) - 1 if logLen >= lstore else 0


def level_off(logLen, lstore, l):
    return (1 << (logLen - lstore + 1)) - (1 << (logLen - l + 1))


class Buf:
    """A device buffer of n words followed by GUARD sentinel words."""

    def __init__(self, torch, n, dtype):
        self.n, self.dtype = n, dtype
        self.fill = 0x5A5A5A5A if dtype == torch.int32 else 0x5A5A5A5A5A5A5A5A
        self.t = torch.full((n + GUARD,), self.fill, dtype=dtype, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        a = self.t.cpu().numpy()
        assert (a[self.n:] == self.fill).all(), "a kernel wrote past the end of its buffer"
        return a[:self.n].view(np.uint32 if a.dtype == np.int32 else np.uint64)


class Tree:
    def __init__(self, torch, logLen, lstore):
        self.logLen, self.lstore = logLen, lstore
        self.nodes = Buf(torch, 8 * max(1, stored_nodes(logLen, lstore)), torch.int32)
        self.root = Buf(torch, 8, torch.int32)

    def check(self, vals, what):
        assert len(vals) == 1 << self.logLen
        want = tree_levels(vals)
        nodes, root = self.nodes.host().tobytes(), self.root.host().tobytes()
        assert root == want[self.logLen], what + ": root"
        for l in range(self.lstore, self.logLen + 1):
            o = 32 * level_off(self.logLen, self.lstore, l)
            assert nodes[o:o + 32 * (1 << (self.logLen - l))] == want[l], "%s: level %d" % (what, l)

    def raw(self):
        return self.nodes.host().tobytes() + self.root.host().tobytes()


def dev_u64(torch, xs):
    return torch.from_numpy(np.array(xs, dtype=np.uint64).view(np.int64)).cuda()


def ptrs(objs):
    return (C.c_uint64 * len(objs))(*[o.ptr for o in objs])


def beta_sets(k, seed, count):
    """`count` challenge tuples of length k: windows of the boundary set first
    (every boundary beta at every fold position for count >= 6), then random."""
    rng = random.Random(seed)
    out = []
    for s in range(count):
        if s < len(BETAS):
            out.append(tuple((BETAS * 3)[s + m] if (m < 6 or rng.random() < 0.3) else rng.randrange(P)
                             for m in range(k)))
        else:
            out.append(tuple(rng.randrange(P) for _ in range(k)))
    return out


# ------------------------------------------------------------------- folds
@pytest.mark.parametrize("logL", [1, 9, 12])
@pytest.mark.parametrize("nf", [2, 3, 4])
def test_foldm_every_intermediate_layer(gpu_ok, dc, nf, logL):
    """k_foldm<F>: output length 2 (one live lane), 2^9 (exactly one
    workgroup), 2^12; every intermediate layer compared."""
    torch = gpu_ok
    src = values(1 << (logL + nf), 100 + nf)
    d_src = dev_u64(torch, src)
    for betas in beta_sets(nf, 200 + logL, 8 if logL < 12 else 7):
        outs = [Buf(torch, 1 << (logL + nf - m), torch.int64) for m in range(1, nf + 1)]
        d_beta = dev_u64(torch, betas)
        assert dc.sezkp_dc_foldm(d_src.data_ptr(), ptrs(outs), d_beta.data_ptr(), nf, logL) == 0
        y = src
        for m in range(nf):
            y = fold(y, betas[m])
            got = outs[m].host()
            assert got.tolist() == list(y), "k_foldm<%d> L=2^%d betas %r: layer %d" % (nf, logL, betas, m + 1)


@pytest.mark.parametrize("logL", [2, 9, 12])
def test_fold_boundary_betas(gpu_ok, dc, logL):
    """k_fold (4 values per lane) at output length 4 (its smallest: one live
    lane), 2^9, 2^12, beta by value and from device memory."""
    torch = gpu_ok
    src = values(2 << logL, 110)
    d_src = dev_u64(torch, src)
    for s, beta in enumerate(BETAS + F.seeded(3, 111)):
        out = Buf(torch, 1 << logL, torch.int64)
        d_beta = dev_u64(torch, [beta])
        by_dev = s & 1
        assert dc.sezkp_dc_fold(d_src.data_ptr(), out.ptr, logL, 0 if by_dev else beta,
                                d_beta.data_ptr() if by_dev else 0) == 0
        assert out.host().tolist() == list(fold(src, beta)), "k_fold L=2^%d beta %#x" % (logL, beta)


def test_fold_refuses_two_outputs(gpu_ok, dc):
    """A lane of k_fold reads and writes 4 consecutive values, so an output of
    2 is not a shape it has: launch_fold refuses it and writes nothing."""
    torch = gpu_ok
    d_src = dev_u64(torch, values(4, 112))
    out = Buf(torch, 2, torch.int64)
    assert dc.sezkp_dc_fold(d_src.data_ptr(), out.ptr, 1, 1, 0) == HIP_INVALID_VALUE
    assert (out.host() == 0x5A5A5A5A5A5A5A5A).all()


# --------------------------------------------------------------- the tails
def tail_reference(src, betas):
    layers, y = [], src
    for b in betas:
        y = fold(y, b)
        layers.append(y)
    return layers


class TailRun:
    """Buffers of one tail: layer Ls - j for j = 0..Ls."""

    def __init__(self, torch, Ls, lstore):
        self.Ls = Ls
        self.vals = [Buf(torch, 1 << (Ls - j), torch.int64) for j in range(Ls + 1)]
        self.trees = [Tree(torch, Ls - j, lstore) for j in range(Ls + 1)]

    def args(self):
        return ptrs(self.vals), ptrs([t.nodes for t in self.trees]), ptrs([t.root for t in self.trees])

    def check(self, want, what):
        for j in range(self.Ls + 1):
            assert self.vals[j].host().tolist() == list(want[j]), "%s: layer %d values" % (what, self.Ls - j)
            self.trees[j].check(want[j], "%s: layer %d" % (what, self.Ls - j))

    def raw(self):
        return [v.host().tobytes() for v in self.vals] + [t.raw() for t in self.trees]


@pytest.mark.parametrize("lstore", [LSTORE_FRI, 0])
@pytest.mark.parametrize("Ls", [11, 3])
def test_fri_tail(gpu_ok, dc, Ls, lstore):
    """k_fri_tail, one launch: workgroup j folds down to layer Ls - j and builds
    its tree. Ls = 11: 2048..1 leaves, every leaves-per-lane case and the
    layers of fewer than 256 leaves; Ls = 3. lstore = 0 keeps every level."""
    torch = gpu_ok
    src = values(2 << Ls, 120)
    d_src = dev_u64(torch, src)
    for betas in beta_sets(Ls + 1, 121 + Ls, 3):
        run = TailRun(torch, Ls, lstore)
        d_beta = dev_u64(torch, betas)
        assert dc.sezkp_dc_fri_tail(d_src.data_ptr(), Ls, d_beta.data_ptr(), *run.args(), lstore) == 0
        run.check(tail_reference(src, betas), "k_fri_tail Ls=%d betas %r" % (Ls, betas[:4]))


def _finish(dc, tree, frm):
    """the upper-level jobs that complete a tree reduced to level `frm`"""
    if frm < tree.logLen:
        n = C.c_int(0)
        assert dc.sezkp_dc_upper_jobs(tree.nodes.ptr, tree.root.ptr, tree.logLen, tree.lstore, frm, 0, 0, 0, 0,
                                      C.byref(n)) == 0
        assert n.value >= 1


@pytest.mark.parametrize("wg_log", [12, 11, 10])
@pytest.mark.parametrize("has_tail", [1, 0])
def test_forest16_with_and_without_tail(gpu_ok, dc, has_tail, wg_log):
    """k_forest16<., TAIL>: one 2^12-leaf forest layer (plus a 2^13-leaf one in
    front, so the workgroup -> layer search runs) and, with a tail, the Ls = 11
    small layers in the same launch (fri_tail_wg): values and trees against the
    reference, and byte for byte what k_fri_tail builds from the same input."""
    torch = gpu_ok
    Ls = 11
    big, src = values(1 << 13, 130), values(1 << 12, 131)
    d_big, d_src = dev_u64(torch, big), dev_u64(torch, src)
    betas = beta_sets(Ls + 1, 132, 2)[1]
    d_beta = dev_u64(torch, betas)
    trees = [Tree(torch, 13, LSTORE_FRI), Tree(torch, 12, LSTORE_FRI)]
    vals = (C.c_uint64 * 2)(d_big.data_ptr(), d_src.data_ptr())
    logs, stops = (C.c_int32 * 2)(13, 12), (C.c_int32 * 2)(wg_log, wg_log)
    run = TailRun(torch, Ls, LSTORE_FRI)
    tailbuf = Buf(torch, TAIL_MAX << TAIL_MAX, torch.int64)
    tv, tn, tr = run.args()
    assert dc.sezkp_dc_forest16(2, vals, ptrs([t.nodes for t in trees]), ptrs([t.root for t in trees]), logs, stops,
                                LSTORE_FRI, wg_log, has_tail, d_src.data_ptr(), Ls, d_beta.data_ptr(), tv, tn, tr,
                                LSTORE_FRI, tailbuf.ptr) == 0
    for t, v in zip(trees, (big, src)):
        _finish(dc, t, wg_log)
        t.check(v, "k_forest16 wg_log=%d tail=%d logLen=%d" % (wg_log, has_tail, t.logLen))
    tailbuf.host()  # guard words only
    if not has_tail:
        assert all((v.host() == v.fill).all() for v in run.vals), "no tail, but tail layers were written"
        return
    run.check(tail_reference(src, betas), "fri_tail_wg wg_log=%d" % wg_log)
    alone = TailRun(torch, Ls, LSTORE_FRI)
    assert dc.sezkp_dc_fri_tail(d_src.data_ptr(), Ls, d_beta.data_ptr(), *alone.args(), LSTORE_FRI) == 0
    assert run.raw() == alone.raw(), "fri_tail_wg and k_fri_tail differ"


# ---------------------------------------------------------------- layer16
@pytest.mark.parametrize("logLen", [12, 13])
@pytest.mark.parametrize("fold_in", [0, 1])
@pytest.mark.parametrize("stop_at", ["wg", "lstore"])
@pytest.mark.parametrize("wg_log", [10, 11, 12])
def test_layer16_forms(gpu_ok, dc, wg_log, stop_at, fold_in, logLen):
    """k_layer16<2 / 3 / 4>: the workgroup reduces to its run root (stop =
    wg_log) or to level LSTORE_FRI, the upper-level jobs build the rest; with
    and without the fused fold; one and several workgroups."""
    torch = gpu_ok
    stop = wg_log if stop_at == "wg" else LSTORE_FRI
    beta = BETAS[(wg_log + logLen + (stop_at == "wg")) % len(BETAS)] if fold_in else 0
    src = values((2 if fold_in else 1) << logLen, 140 + logLen)
    want = fold(src, beta) if fold_in else src
    d_src = dev_u64(torch, src)
    out = Buf(torch, (1 << logLen) if fold_in else 1, torch.int64)
    tree = Tree(torch, logLen, LSTORE_FRI)
    d_beta = dev_u64(torch, [beta])
    by_dev = fold_in and (wg_log & 1)
    assert dc.sezkp_dc_layer16(d_src.data_ptr(), out.ptr, logLen, fold_in, 0 if by_dev else beta,
                               d_beta.data_ptr() if by_dev else 0, tree.nodes.ptr, tree.root.ptr, LSTORE_FRI, stop,
                               wg_log) == 0
    _finish(dc, tree, stop)
    what = "k_layer16 wg_log=%d stop=%d fold=%d logLen=%d beta=%#x" % (wg_log, stop, fold_in, logLen, beta)
    if fold_in:
        assert out.host().tolist() == list(want), what + ": folded values"
    else:
        out.host()
    tree.check(want, what)


@pytest.mark.parametrize("wg_log", [10, 11, 12])
def test_layer16_fold_boundary_betas(gpu_ok, dc, wg_log):
    """The fused fold of k_layer16 at every boundary challenge."""
    torch = gpu_ok
    logLen = 12
    src = values(2 << logLen, 150)
    d_src = dev_u64(torch, src)
    for beta in BETAS + F.seeded(1, 151 + wg_log):
        out, tree = Buf(torch, 1 << logLen, torch.int64), Tree(torch, logLen, LSTORE_FRI)
        assert dc.sezkp_dc_layer16(d_src.data_ptr(), out.ptr, logLen, 1, beta, 0, tree.nodes.ptr, tree.root.ptr,
                                   LSTORE_FRI, wg_log, wg_log) == 0
        _finish(dc, tree, wg_log)
        want = fold(src, beta)
        assert out.host().tolist() == list(want), "k_layer16 wg_log=%d beta=%#x" % (wg_log, beta)
        tree.check(want, "k_layer16 wg_log=%d beta=%#x" % (wg_log, beta))


# ------------------------------------------------------------ upper jobs
@pytest.mark.parametrize("logLen,frm", [(12, 12), (13, 12), (18, 6)])
def test_upper_jobs_from_gathered_roots(gpu_ok, dc, logLen, frm):
    """k_upper_jobs reading level `frm` from gathered run roots: the one-node
    cap (`gath && from == top`: the job copies the root into the cap and its
    root slot), a two-node cap, and from level 6 of a 2^18 tree (4 nodes per
    lane, two passes); rank-major gathered order for P = 1 and 2."""
    torch = gpu_ok
    rng = random.Random(160 + logLen)
    cnt = 1 << (logLen - frm)
    import oracle_ctypes as O
    level = [rng.randbytes(32) for _ in range(cnt)]
    upper = O.merkle_nodes(b"".join(level))  # the levels above `frm`, whatever lies below it
    for logP in ([0] if cnt == 1 else [0, 1]):
        nrun = cnt >> logP
        gath = [None] * cnt
        for g in range(cnt):  # cap node g = root g >> logP of rank g & (P - 1)
            gath[(g & ((1 << logP) - 1)) * nrun + (g >> logP)] = level[g]
        d_gath = torch.from_numpy(np.frombuffer(b"".join(gath), dtype=np.int32).copy()).cuda()
        tree = Tree(torch, logLen, frm)
        n = C.c_int(0)
        assert dc.sezkp_dc_upper_jobs(tree.nodes.ptr, tree.root.ptr, logLen, frm, frm, 0, d_gath.data_ptr(), nrun, logP,
                                      C.byref(n)) == 0
        assert n.value >= 1
        nodes, root = tree.nodes.host().tobytes(), tree.root.host().tobytes()
        assert nodes == upper, "cap levels %d..%d (logP=%d)" % (frm, logLen, logP)
        assert root == upper[-32:]


# ------------------------------------------- whole trees and upper levels
@pytest.mark.parametrize("lstore", [LSTORE_FRI, 0])
@pytest.mark.parametrize("fold_in", [0, 1])
@pytest.mark.parametrize("logLen", [0, 1, 2, 3, 8, 9, 10, 11, 12, 13])
def test_leaf_subtree_every_level(gpu_ok, dc, logLen, fold_in, lstore):
    """launch_leaf_subtree: k_leaf_subtree with 1, 2 (its scalar branch) and 4
    leaves per lane, fewer than 256 active lanes (2^8), exactly one workgroup
    (2^10), two workgroups and one upper launch (2^11), and the hand-over to
    k_layer16<4> alone (2^12) and with an upper launch (2^13). Every stored
    level and the root; with the fused fold also the folded values, the
    challenge by value and from device memory."""
    torch = gpu_ok
    src = values((2 if fold_in else 1) << logLen, 170 + logLen)
    d_src = dev_u64(torch, src)
    picks = [BETAS[(logLen + lstore) % len(BETAS)], BETAS[(logLen + lstore + 3) % len(BETAS)]] if fold_in else [0]
    for by_dev, beta in enumerate(picks):
        want = fold(src, beta) if fold_in else src
        out = Buf(torch, (1 << logLen) if fold_in else 1, torch.int64)
        tree = Tree(torch, logLen, lstore)
        d_beta = dev_u64(torch, [beta])
        assert dc.sezkp_dc_leaf_subtree(d_src.data_ptr(), out.ptr, logLen, fold_in, 0 if by_dev else beta,
                                        d_beta.data_ptr() if by_dev else 0, tree.nodes.ptr, tree.root.ptr,
                                        lstore) == 0
        what = "launch_leaf_subtree logLen=%d fold=%d lstore=%d beta=%#x by_dev=%d" % (logLen, fold_in, lstore, beta,
                                                                                     by_dev)
        if fold_in:
            assert out.host().tolist() == list(want), what + ": folded values"
        else:
            assert (out.host() == out.fill).all(), what + ": no fold, but values were written"
        tree.check(want, what)
        if logLen < lstore:
            assert (tree.nodes.host() == tree.nodes.fill).all(), what + ": no stored level, but nodes were written"


@pytest.mark.parametrize("logLen,frm,ntrees", [(6, 6, 1), (7, 6, 2), (16, 6, 1), (17, 6, 1)])
def test_tree_upper_from_stored_level(gpu_ok, dc, logLen, frm, ntrees):
    """launch_tree_upper from random level-`frm` nodes: the single-node root
    job, one parent (two trees of one shape, their nodes and roots spaced by
    strides that leave gaps), exactly one step of 10 levels, two launches."""
    torch = gpu_ok
    import oracle_ctypes as O
    rng = random.Random(180 + logLen)
    cnt, stored = 1 << (logLen - frm), stored_nodes(logLen, frm)
    tstride, rstride = (stored + 3, 12) if ntrees > 1 else (0, 0)  # nodes, words
    nodes = Buf(torch, 8 * (tstride * (ntrees - 1) + stored), torch.int32)
    roots = Buf(torch, rstride * (ntrees - 1) + 8, torch.int32)
    want = []
    for t in range(ntrees):
        level = b"".join(rng.randbytes(32) for _ in range(cnt))
        want.append(O.merkle_nodes(level))  # levels frm .. logLen, bottom -> top: the stored layout
        assert len(want[t]) == 32 * stored
        nodes.t[8 * tstride * t:8 * (tstride * t + cnt)] = torch.from_numpy(
            np.frombuffer(level, dtype=np.int32).copy()).cuda()
    assert dc.sezkp_dc_tree_upper(nodes.ptr, roots.ptr, logLen, frm, ntrees, tstride, rstride, frm) == 0
    got, got_roots = nodes.host(), roots.host()
    for t in range(ntrees):
        what = "launch_tree_upper logLen=%d from=%d tree %d" % (logLen, frm, t)
        assert got[8 * tstride * t:8 * (tstride * t + stored)].tobytes() == want[t], what + ": levels"
        assert got_roots[rstride * t:rstride * t + 8].tobytes() == want[t][-32:], what + ": root"
    for t in range(ntrees - 1):  # the gaps between the trees and between the roots
        assert (got[8 * (tstride * t + stored):8 * tstride * (t + 1)] == nodes.fill).all()
        assert (got_roots[rstride * t + 8:rstride * (t + 1)] == roots.fill).all()
