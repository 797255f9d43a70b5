"""GPU tests of the wide head ladder: 8-row head groups committed from a
value-keyed table that a context keeps across proofs.

A head column with a delta plan commits an aligned 8-row group from one
table node L3[first head, 7 moves] instead of two 4-row nodes and a merge.
The table spans the head range of the last completed proof widened by 8
values on each side, is built by the second proof of a dictionary epoch and
kept after that; a group it does not cover (a block starting in rows 1..7 of
the group, a first head outside the span) takes the 4-row nodes, so the
bytes never depend on the table. `ProverContext.head_wide_stats()` reports
the span, the entries built and the groups taken either way.

Every proof here is compared byte for byte with the oracle's, and the proof
of every trace with `SEZKP_HEAD_WIDE=0` on a fresh context is too (so the two
arms are equal to each other). The expected stats come from `Model`, which
restates the host's decision (csrc/prove_plan.h) and counts the groups from
the trace: a path that fell back everywhere, or never built, fails the counts.

Sizes: tau = 2; T = 2^14 and 2^15 are one and two full commit workgroups per
column at a = 0 (256 lanes of 64 rows), T = 2^13 ends inside a workgroup.
The plan-rows hook at 22 is lowered by the prover to 20 / 21 for these row
counts (a stays 0: `lane_tree_pf<3>`); a = 1 (`lane_tree_pf<4>`) needs 2^16
real rows, which one case has, and its plan is asserted to say a = 1.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import ORACLE, PKG, free_port
from test_gpu_dict_forms import Trace, _heads, _iid, _walk

pytestmark = pytest.mark.gpu

ROOT = hashlib.sha256(b"wide head ladder").digest()
ENV_KEYS = ("SEZKP_TEST_DICT_PLAN_ROWS_LOG", "SEZKP_HEAD_WIDE", "SEZKP_HEAD_WIDE_CAP", "SEZKP_DICT_CACHE",
            "SEZKP_DICT_TAB_CAP")
MARGIN, RESPAN, CAP = 8, 64, 1 << 19


def _walk_trace(product, n, b, seed, bounds, step=1):
    """tau = 2: both heads are {-step..step} walks per block, reflected into
    [-bounds[t], bounds[t]] for step = 1 (so a trace's head range is its
    bound, both sides of zero); the other columns are small iid ranges."""
    rng = np.random.default_rng(seed)
    if step == 1:
        heads = [_walk(rng, n, b, bounds[0]), _walk(rng, n, b, bounds[1])]
    else:
        heads = [_heads(rng.integers(-step, step + 1, n), b) for _ in range(2)]
    one = np.ones(n, np.int64)
    return Trace(product, b, _iid(rng, n, -1, 3), heads=heads, mvs=[None, None], flags=[one, one],
                 syms=[_iid(rng, n, 0, 4), _iid(rng, n, 0, 4)])


BUILDERS = {
    # one context, T = 2^14, b = 512: the span is A's range + 8; C stays inside
    # the margin and touches both ends of the span (first and last head code),
    # D leaves it by one value on both sides, E by far
    "A": lambda p: _walk_trace(p, 1 << 14, 512, 31, (20, 12)),
    "C": lambda p: _walk_trace(p, 1 << 14, 512, 32, (28, 20)),
    "D": lambda p: _walk_trace(p, 1 << 14, 512, 33, (29, 21)),
    "E": lambda p: _walk_trace(p, 1 << 14, 512, 34, (60, 40)),
    "A333": lambda p: _walk_trace(p, 1 << 14, 333, 35, (20, 12)),
    "A1023": lambda p: _walk_trace(p, 1 << 14, 1023, 36, (20, 12)),
    "S": lambda p: _walk_trace(p, 1 << 13, 512, 37, (20, 12)),
    "L": lambda p: _walk_trace(p, 1 << 15, 512, 38, (20, 12)),
    "X": lambda p: _walk_trace(p, 1 << 16, 512, 40, (20, 12)),
    "M2": lambda p: _walk_trace(p, 1 << 14, 128, 41, None, step=2),
}


def _sizes(span, dR, dmin, cap):
    """head_wide_sizes: (L3 entries, lower-level entries) or None."""
    if span == 0 or dR == 0 or dR ** 7 > cap or span > cap // dR ** 7:
        return None
    dmax = dmin + dR - 1
    sw = span + 7 * (max(dmax, 0) - min(dmin, 0))
    return span * dR ** 7, sw * (1 + dR + dR ** 3)


class Model:
    """The host's ladder state of one context and the stats a proof must
    report. Restates head_wide_decide / head_wide_observe and the slot rule
    of the prover (a larger slot moves, and so rebuilds, every ladder)."""

    def __init__(self):
        self.cols = {t: dict(epoch=0, olo=0, span=0, dmin=0, dR=0, seen=None, seen_epoch=0, respan=False)
                     for t in range(2)}
        self.slot = 0

    def _decide(self, c, epoch, cap):
        if c["epoch"] == epoch and not c["respan"]:
            sz = _sizes(c["span"], c["dR"], c["dmin"], cap)
            if sz is None:  # the cap was lowered: the ladder is dropped
                c["epoch"] = 0
            return (sz is not None, False, sz)
        s = c["seen"]
        if c["seen_epoch"] != epoch or s is None:
            if c["epoch"] != epoch:
                c["epoch"] = 0
            return (False, False, None)
        lo, hi, mlo, mhi = s[0] - MARGIN, s[1] + MARGIN, s[2], s[3]
        if c["epoch"] == epoch:
            ulo, uhi = min(lo, c["olo"]), max(hi, c["olo"] + c["span"] - 1)
            umlo, umhi = min(mlo, c["dmin"]), max(mhi, c["dmin"] + c["dR"] - 1)
            if _sizes(uhi - ulo + 1, umhi - umlo + 1, umlo, cap):
                lo, hi, mlo, mhi = ulo, uhi, umlo, umhi
        c["respan"], c["epoch"] = False, 0
        sz = _sizes(hi - lo + 1, mhi - mlo + 1, mlo, cap)
        if sz is None:
            return (False, False, None)
        c.update(epoch=epoch, olo=lo, span=hi - lo + 1, dmin=mlo, dR=mhi - mlo + 1)
        return (True, True, sz)

    def prove(self, tr, epoch, r0=0, r1=None, cap=CAP, on=True):
        """Expected head_wide_stats() after proving rows [r0, r1) of tr."""
        r1 = r1 or tr.T
        dec = {t: (self._decide(c, epoch, cap) if on else (False, False, None)) for t, c in self.cols.items()}
        slot = max([sum(d[2]) for d in dec.values() if d[0]] + [0])
        slot = (slot + 4095) & ~4095
        if any(d[1] for d in dec.values()) and slot > self.slot:
            self.slot = slot
            dec = {t: (d[0], d[0], d[2]) for t, d in dec.items()}
        out = []
        for t, c in self.cols.items():
            use, build, sz = dec[t]
            in_place = c["epoch"] == epoch and c["span"] != 0
            head, mv = tr.cols[(6, t)][r0:r1], tr.cols[(3, t)][r0:r1]
            start = (np.arange(r0, r1) % tr.b == 0).reshape(-1, 8)[:, 1:].any(axis=1)
            h0 = head.reshape(-1, 8)[:, 0]
            mlo, mhi = int(mv.min()), int(mv.max())
            if in_place and use and on:
                moves_in = mlo >= c["dmin"] and mhi < c["dmin"] + c["dR"]
                outside = ~start & ((h0 < c["olo"]) | (h0 >= c["olo"] + c["span"]) | (not moves_in))
                fb_start, fb_span = int(start.sum()), int(outside.sum())
                wide = h0.size - fb_start - fb_span
            else:
                wide = fb_start = fb_span = 0
            out.append({"tape": t, "origin": c["olo"] if in_place else 0, "span": c["span"] if in_place else 0,
                        "dR": c["dR"] if in_place else 0, "R": int(head.max() - head.min()) + 1,
                        "entries_built": sum(sz) if build else 0, "groups_wide": wide,
                        "groups_fallback": fb_start + fb_span, "groups_out_of_span": fb_span,
                        "table_bytes": self.slot * 32 if in_place else 0})
            # head_wide_observe
            c["seen"], c["seen_epoch"] = (int(head.min()), int(head.max()), mlo, mhi), epoch
            if c["epoch"] == epoch and fb_span * RESPAN > wide + fb_start + fb_span:
                c["respan"] = True
        return out


def _stats(ctx):
    return [{k: v for k, v in s.items() if k != "col"} for s in ctx.head_wide_stats()]


class Cases:
    def __init__(self, product, oracle):
        self.product, self.oracle, self.traces = product, oracle, {}

    def trace(self, name):
        """The trace, its oracle proof, and (checked once) its proof with the
        ladder switched off."""
        if name not in self.traces:
            tr = BUILDERS[name](self.product)
            tr.want = self.oracle.prove_v1(tr.blocks, ROOT)
            self.traces[name] = tr
            old = os.environ.get("SEZKP_HEAD_WIDE")
            os.environ["SEZKP_HEAD_WIDE"] = "0"
            ctx = self.product.ProverContext(0)
            try:
                ctx.upload(tr.blocks)
                for _ in range(2):
                    assert ctx.prove(ROOT).proof_bytes == tr.want, name
                    assert all(s["span"] == 0 and s["groups_wide"] == 0 and s["entries_built"] == 0
                               for s in ctx.head_wide_stats())
            finally:
                ctx.close()
                if old is None:
                    del os.environ["SEZKP_HEAD_WIDE"]
                else:
                    os.environ["SEZKP_HEAD_WIDE"] = old
        return self.traces[name]

    def prove(self, ctx, model, name, epoch, staged=True, **kw):
        tr = self.trace(name)
        if staged:
            ctx.upload(tr.blocks)
        assert ctx.prove(ROOT).proof_bytes == tr.want, name
        want = model.prove(tr, epoch, **kw)
        assert _stats(ctx) == want, name
        plans = {(p["kind"], p["tape"]): p for p in ctx.dict_plans()}
        assert all(plans[(6, t)]["delta"] == 1 for t in range(2)), name
        return want


@pytest.fixture(scope="module")
def cases(product, oracle):
    return Cases(product, oracle)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name,hook", [("A", None), ("L", None), ("S", None), ("A", "22"), ("L", "22"), ("X", "22"),
                                       ("A333", None), ("A1023", None), ("A333", "22")])
def test_built_by_the_second_proof(gpu_ok, product, cases, monkeypatch, name, hook):
    """One trace three times on one context: the first proof builds nothing
    and takes no group wide, the second builds both ladders and takes every
    eligible group wide, the third reuses them. The groups that must fall
    back are counted from the trace: none at b = 512, the block starts in
    rows 1..7 of a group at b = 333 and 1023."""
    if hook:
        monkeypatch.setenv("SEZKP_TEST_DICT_PLAN_ROWS_LOG", hook)
    tr, model = cases.trace(name), Model()
    ctx = product.ProverContext(0)
    try:
        ctx.upload(tr.blocks)
        assert ctx.head_wide_stats() == []
        first = cases.prove(ctx, model, name, 1, staged=False)
        assert all(s["span"] == 0 and s["entries_built"] == 0 and s["groups_wide"] == 0 for s in first)
        second = cases.prove(ctx, model, name, 1, staged=False)
        third = cases.prove(ctx, model, name, 1, staged=False)
        a = {(p["kind"], p["tape"]): p["a"] for p in ctx.dict_plans()}
        assert a[(6, 0)] == a[(6, 1)] == (1 if name == "X" else 0)
    finally:
        ctx.close()
    starts = {512: 0, 333: None, 1023: None}[tr.b]
    for s2, s3 in zip(second, third):
        assert s2["entries_built"] > 0 and s3["entries_built"] == 0
        assert s2["span"] == s2["R"] + 2 * MARGIN and s2["origin"] < 0 and s2["dR"] == 3
        assert s2["groups_wide"] + s2["groups_fallback"] == tr.T // 8 and s2["groups_out_of_span"] == 0
        if starts is None:
            assert 0 < s2["groups_fallback"] < tr.T // 8 // 16
        else:
            assert s2["groups_fallback"] == 0
        assert {k: v for k, v in s3.items() if k != "entries_built"} == \
            {k: v for k, v in s2.items() if k != "entries_built"}


def test_span_margin_fallback_and_respan(gpu_ok, product, cases):
    """A, A (build), C inside the margin with heads on the first and the last
    value of the span (reused, nothing outside), D one value outside on both
    sides (a few groups fall back, below the threshold: reused), E far
    outside (a known count falls back: same bytes), then A: the ladder is
    re-spanned over both ranges, and E fits it."""
    model = Model()
    ctx = product.ProverContext(0)
    try:
        cases.prove(ctx, model, "A", 1)
        built = cases.prove(ctx, model, "A", 1)
        for t in range(2):
            hc = cases.trace("C").cols[(6, t)]
            assert hc.min() == built[t]["origin"] and hc.max() == built[t]["origin"] + built[t]["span"] - 1
        c = cases.prove(ctx, model, "C", 1)
        assert all(s["entries_built"] == 0 and s["groups_fallback"] == 0 for s in c)
        d = cases.prove(ctx, model, "D", 1)
        assert all(s["entries_built"] == 0 and 0 < s["groups_out_of_span"] * RESPAN <= 2048 for s in d)
        c = cases.prove(ctx, model, "C", 1)
        assert all(s["entries_built"] == 0 and s["span"] == built[t]["span"] for t, s in enumerate(c))
        e = cases.prove(ctx, model, "E", 1)
        assert all(s["entries_built"] == 0 and s["groups_out_of_span"] * RESPAN > 2048 for s in e)
        a = cases.prove(ctx, model, "A", 1)
        for t, s in enumerate(a):
            he = cases.trace("E").cols[(6, t)]
            assert s["entries_built"] > 0 and s["groups_fallback"] == 0
            lo = min(he.min() - MARGIN, built[t]["origin"])
            hi = max(he.max() + MARGIN, built[t]["origin"] + built[t]["span"] - 1)
            assert s["origin"] == lo and s["span"] == hi - lo + 1
        e = cases.prove(ctx, model, "E", 1)
        assert all(s["entries_built"] == 0 and s["groups_fallback"] == 0 for s in e)
    finally:
        ctx.close()


def test_not_qualifying(gpu_ok, product, cases, monkeypatch):
    """Moves of range 2 (dR = 5: 5^7 entries per head value) and a cap below
    span * 3^7 build no ladder; the cap lifted, the next proof builds it; the
    cap lowered again, the ladder is dropped."""
    model = Model()
    ctx = product.ProverContext(0)
    try:
        for _ in range(3):
            s = cases.prove(ctx, model, "M2", 1)
            assert all(x["span"] == 0 and x["groups_wide"] == 0 for x in s)
    finally:
        ctx.close()
    model = Model()
    ctx = product.ProverContext(0)
    low = 30 * 3 ** 7  # A's spans are 41 + 16 and 25 + 16
    try:
        monkeypatch.setenv("SEZKP_HEAD_WIDE_CAP", str(low))
        for _ in range(2):
            s = cases.prove(ctx, model, "A", 1, cap=low)
            assert all(x["span"] == 0 and x["groups_wide"] == 0 for x in s)
        monkeypatch.delenv("SEZKP_HEAD_WIDE_CAP")
        s = cases.prove(ctx, model, "A", 1)
        assert all(x["entries_built"] > 0 and x["groups_wide"] == 2048 for x in s)
        monkeypatch.setenv("SEZKP_HEAD_WIDE_CAP", str(low))
        s = cases.prove(ctx, model, "A", 1, cap=low)
        assert all(x["span"] == 0 and x["groups_wide"] == 0 for x in s)
    finally:
        ctx.close()


def test_switch_off_keeps_the_ladder_and_epoch_rebuilds(gpu_ok, product, cases, monkeypatch):
    """SEZKP_HEAD_WIDE=0 for one proof takes no group wide and leaves the
    ladder in place for the next; another n on the same context is another
    epoch: its first proof builds nothing, its second builds again."""
    model = Model()
    ctx = product.ProverContext(0)
    try:
        cases.prove(ctx, model, "A", 1)
        cases.prove(ctx, model, "A", 1)
        monkeypatch.setenv("SEZKP_HEAD_WIDE", "0")
        s = cases.prove(ctx, model, "A", 1, on=False)
        assert all(x["groups_wide"] == 0 for x in s)
        monkeypatch.delenv("SEZKP_HEAD_WIDE")
        s = cases.prove(ctx, model, "C", 1)
        assert all(x["entries_built"] == 0 and x["groups_wide"] == 2048 for x in s)
        s = cases.prove(ctx, model, "L", 2)
        assert all(x["span"] == 0 and x["entries_built"] == 0 and x["groups_wide"] == 0 for x in s)
        s = cases.prove(ctx, model, "L", 2)
        assert all(x["entries_built"] > 0 and x["groups_wide"] == 4096 for x in s)
    finally:
        ctx.close()


def test_stats_arguments(gpu_ok, product, cases):
    import ctypes as C
    from sezkp_amd._lib import HeadWideInfo
    buf = (HeadWideInfo * 2)()
    ctx = product.ProverContext(0)
    try:
        assert product.lib.sezkp_ctx_head_wide_stats(None, buf, 2) == -1
        assert product.lib.sezkp_ctx_head_wide_stats(ctx._h, None, 2) == -1
        assert product.lib.sezkp_ctx_head_wide_stats(ctx._h, buf, -1) == -1
        assert product.lib.sezkp_ctx_head_wide_stats(ctx._h, buf, 2) == 0
        ctx.upload(cases.trace("A").blocks)
        ctx.prove(ROOT)
        assert product.lib.sezkp_ctx_head_wide_stats(ctx._h, buf, 1) == 1
        assert product.lib.sezkp_ctx_head_wide_stats(ctx._h, None, 0) == 0
    finally:
        ctx.close()


def _sharded_worker(rank, world, port, q):
    sys.path[:0] = [PKG, ORACLE, os.path.dirname(os.path.abspath(__file__))]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sezkp_amd
        tr = BUILDERS["L"](sezkp_amd)
        ctx = sezkp_amd.ShardedProverContext(rank, world, device=0, comm="host")
        ctx.upload(tr.blocks)
        out = []
        for _ in range(3):
            proof = ctx.prove(ROOT).proof_bytes
            out.append((hashlib.sha256(proof).hexdigest(), _stats(ctx)))
        ctx.close()
        q.put((rank, out))
    except Exception as e:
        q.put((rank, f"ERR {type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


def test_sharded_p2_host_collectives(gpu_ok, product, cases):
    """P = 2 over host collectives, T = 2^15: each rank keeps the ladder of
    its own 2^14 rows; every rank returns the single-device bytes."""
    import torch.multiprocessing as mp
    tr = cases.trace("L")
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = free_port()
    ps = [mpc.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=300) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    for rank, out in res:
        assert not isinstance(out, str), (rank, out)
        model = Model()
        for digest, stats in out:
            assert digest == hashlib.sha256(tr.want).hexdigest(), rank
            assert stats == model.prove(tr, 1, rank << 14, (rank + 1) << 14), rank
        assert all(s["groups_wide"] == 2048 and s["entries_built"] == 0 for s in out[2][1]), rank
