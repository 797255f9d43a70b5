"""GPU tests of the dictionary table reuse across the proofs of one context.

A dictionary column's tables T_0..T_K depend on the column's value range (a
head column's also on its tape's move range) and on host-side inputs (rows,
the rows planned for, the table cap, the column's label and table slot), not
on the rows. `k_dict_plan` keeps, per column, the key its tables were last
built from and marks the column reused when the new key equals it;
`ProverContext.dict_cache_stats()` reports the columns rebuilt and reused and
the table entries rebuilt by the last prove.

Every proof here is compared with the oracle's bytes and every `dict_plans()`
with that of a fresh context proving the same trace under the same
environment. The expected rebuild sets are derived from the traces' own
ranges (`_key`): a column rebuilds exactly when its key differs from the one
of the previous proof on the context, and the expected entry count is the sum
of the rebuilt columns' table sizes by the restated planner
(`test_gpu_dict_forms.model_plan`), so the counts pin which columns rebuilt
and not only how many.

Traces: tau = 2, T = 2^12 (b = 512 and 333) and 2^13, with designed ranges.
The case where K moves down and back needs a plan with K = 4 for a column of
range 2, which the planner only chooses from 2^21 planned rows on, and the
plan-rows hook reaches 2^21 from 2^15 real rows on: that one case has
T = 2^15.

The refused proof in between uses the guard hook of the sharded tests
(`SEZKP_DEBUG_TRIP_GUARD=<rank>`, read per prove): a refusal without a fault
on a small trace.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import ORACLE, PKG, free_port
from test_gpu_dict_forms import DICT_CAP, Trace, _iid, _plant, model_plan

pytestmark = pytest.mark.gpu

ROOTS = [bytes(32), bytes(range(32)), hashlib.sha256(b"dictionary cache").digest()]
ENV_KEYS = ("SEZKP_TEST_DICT_PLAN_ROWS_LOG", "SEZKP_DICT_TAB_CAP", "SEZKP_DICT_CACHE")


def _steps(rng, n):
    return rng.integers(-1, 2, n)


def _build(product, n, b, seed, head0, sym1, imv_r=16, flag0_r=2):
    """tau = 2. Tape 0: a designed head of range head0 = (lo, R) (its moves
    are derived, so the move range follows the head's); tape 1: moves in
    {-1, 0, 1} (the head's range is the walk's, it moves with the seed).
    Flags: tape 0 of range flag0_r, tape 1 constant 1; symbols: tape 0 of
    range 16, tape 1 of range sym1; input moves of range imv_r."""
    rng = np.random.default_rng(seed)
    one = np.ones(n, np.int64)
    mv1 = _plant(_steps(rng, n), -1, 1)
    flag0 = _plant(rng.integers(0, flag0_r, n), 0, flag0_r - 1)
    return Trace(product, b, _iid(rng, n, -(imv_r // 2), imv_r),
                 heads=[_iid(rng, n, head0[0], head0[1]), None], mvs=[None, mv1],
                 flags=[flag0, one], syms=[_iid(rng, n, 0, 16), _iid(rng, n, 0, sym1)])


BUILDERS = {
    # A and B: B differs in tape 1's symbol range, tape 0's move range and both head ranges
    "A": lambda p: _build(p, 1 << 12, 512, 11, (-2, 4), 4),
    "B": lambda p: _build(p, 1 << 12, 512, 12, (-3, 6), 5),
    "A333": lambda p: _build(p, 1 << 12, 333, 13, (-2, 4), 4),
    "B333": lambda p: _build(p, 1 << 12, 333, 14, (-3, 6), 5),
    "L": lambda p: _build(p, 1 << 13, 512, 15, (-2, 4), 4),
    # K down and back: the input-move column (int8) has range 2, then 3
    "K2": lambda p: _build(p, 1 << 15, 512, 16, (-2, 4), 4, imv_r=2),
    "K3": lambda p: _build(p, 1 << 15, 512, 17, (-2, 4), 4, imv_r=3),
}
B_DIFFERS = {(5, 1), (3, 0), (6, 0), (6, 1)}


def _key(tr, col):
    """What the device keys the column's tables by: its range and, for a head
    column, its tape's move range."""
    return tr.range_of(col) + (tr.range_of((3, col[1])) if col[0] == 6 else ())


def _entries(tr, col, nrows, cap=DICT_CAP):
    """Table entries of the column's plan: R^(2^k) for k <= K, or R + R^2 +
    R dR^3 for a delta plan."""
    lo, hi = tr.range_of(col)
    mvr = tr.range_of((3, col[1])) if col[0] == 6 else None
    p = model_plan(lo, hi, mvr, tr.T, nrows, cap)
    if p["delta"]:
        return p["R"] + p["R"] ** 2 + p["R"] * p["dR"] ** 3
    return sum(p["R"] ** (1 << k) for k in range(p["K"] + 1))


def _plan_rows(tr, nrows=None):
    """The rows the planner prices: the hook's 2^v, lowered as prove_body
    lowers it for a device with few rows, else the device's rows."""
    nrows = nrows or tr.T
    v = os.environ.get("SEZKP_TEST_DICT_PLAN_ROWS_LOG")
    if v is None:
        return nrows
    lg = nrows.bit_length() - 1
    v_max = 40 if lg >= 16 else 20 + max(0, lg - 14)
    return 1 << min(int(v), v_max)


class Want:
    """The oracle's proof of one trace per manifest root, computed on first use."""

    def __init__(self, oracle, blocks):
        self.oracle, self.blocks, self.got = oracle, blocks, {}

    def __getitem__(self, root):
        if root not in self.got:
            self.got[root] = self.oracle.prove_v1(self.blocks, ROOTS[root])
        return self.got[root]


class Cases:
    """The traces, their oracle proofs, and the plans of fresh contexts."""

    def __init__(self, product, oracle):
        self.product, self.oracle = product, oracle
        self.traces, self.fresh = {}, {}

    def trace(self, name):
        if name not in self.traces:
            tr = BUILDERS[name](self.product)
            tr.want = Want(self.oracle, tr.blocks)
            self.traces[name] = tr
        return self.traces[name]

    def fresh_plans(self, name):
        """dict_plans() of a fresh context proving the trace under the
        environment of the moment."""
        env = tuple(os.environ.get(k) for k in ENV_KEYS[:2])
        if (name, env) not in self.fresh:
            tr = self.trace(name)
            ctx = self.product.ProverContext(0)
            try:
                ctx.upload(tr.blocks)
                assert ctx.prove(ROOTS[0]).proof_bytes == tr.want[0]
                self.fresh[(name, env)] = ctx.dict_plans()
                st = ctx.dict_cache_stats()
                assert (st["cols_rebuilt"], st["cols_reused"]) == (len(tr.cols), 0)
            finally:
                ctx.close()
        return self.fresh[(name, env)]

    def prove(self, ctx, name, root, prev, everything=False):
        """One proof of trace `name` on ctx. prev: the trace the context's
        tables were last built from (None or everything=True: all columns
        rebuild). Checks bytes, plans and the reuse counts; returns the name."""
        tr = self.trace(name)
        assert ctx.prove(ROOTS[root]).proof_bytes == tr.want[root], (name, root)
        self.check(ctx, name, prev, everything)
        return name

    def check(self, ctx, name, prev, everything=False):
        tr = self.trace(name)
        assert ctx.dict_plans() == self.fresh_plans(name), name
        old = None if everything or prev is None else self.trace(prev)
        rebuilt = [c for c in tr.cols if old is None or _key(old, c) != _key(tr, c)]
        cap = int(os.environ.get("SEZKP_DICT_TAB_CAP", DICT_CAP))
        entries = sum(_entries(tr, c, _plan_rows(tr), cap) for c in rebuilt)
        assert ctx.dict_cache_stats() == {"cols_rebuilt": len(rebuilt), "cols_reused": len(tr.cols) - len(rebuilt),
                                          "entries_rebuilt": entries}, (name, prev, sorted(rebuilt))


@pytest.fixture(scope="module")
def cases(product, oracle):
    return Cases(product, oracle)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV_KEYS + ("SEZKP_DEBUG_TRIP_GUARD",):
        monkeypatch.delenv(k, raising=False)


def test_designed_differences(cases):
    """B differs from A in exactly tape 1's symbols, tape 0's moves and both
    heads; the K traces in the input moves only besides the walk's head."""
    for a, b in (("A", "B"), ("A333", "B333")):
        ta, tb = cases.trace(a), cases.trace(b)
        assert {c for c in ta.cols if _key(ta, c) != _key(tb, c)} == B_DIFFERS
    k2, k3 = cases.trace("K2"), cases.trace("K3")
    assert k2.range_of((0, 0)) == (-1, 0) and k3.range_of((0, 0)) == (-1, 1)


@pytest.mark.parametrize("name", ["A", "A333"])
def test_warm_reuse(gpu_ok, product, cases, name):
    """A, A, A under three manifest roots: the first prove rebuilds every
    column, the later ones none (0 entries)."""
    ctx = product.ProverContext(0)
    try:
        ctx.upload(cases.trace(name).blocks)
        assert ctx.dict_cache_stats() == {"cols_rebuilt": 0, "cols_reused": 0, "entries_rebuilt": 0}
        prev = None
        for root in range(3):
            prev = cases.prove(ctx, name, root, prev)
            st = ctx.dict_cache_stats()
            assert (st["cols_rebuilt"], st["entries_rebuilt"] == 0) == ((9, False) if root == 0 else (0, True))
    finally:
        ctx.close()


@pytest.mark.parametrize("a,b", [("A", "B"), ("A333", "B333")])
def test_partial_change_staged(gpu_ok, product, cases, a, b):
    """A, then B staged: exactly tape 1's symbols, tape 0's moves and the two
    heads rebuild (tape 0's head also because its key holds the move range);
    B again: none; A staged again: the same four."""
    ctx = product.ProverContext(0)
    try:
        ctx.upload(cases.trace(a).blocks)
        prev = cases.prove(ctx, a, 0, None)
        ctx.stage(cases.trace(b).blocks)
        prev = cases.prove(ctx, b, 1, prev)
        assert ctx.dict_cache_stats()["cols_rebuilt"] == len(B_DIFFERS)
        prev = cases.prove(ctx, b, 2, prev)
        assert ctx.dict_cache_stats()["cols_rebuilt"] == 0
        ctx.stage(cases.trace(a).blocks)
        cases.prove(ctx, a, 1, prev)
        assert ctx.dict_cache_stats()["cols_rebuilt"] == len(B_DIFFERS)
    finally:
        ctx.close()


def test_level_moves_down_and_back(gpu_ok, product, cases, monkeypatch):
    """A column of range 2 (K = 4 when 2^21 rows are planned for), then of
    range 3 (K = 3: T_4 of the first trace stays in place, stale), then of
    range 2 again: its levels 0..4 are rebuilt, the bytes match at every step."""
    monkeypatch.setenv("SEZKP_TEST_DICT_PLAN_ROWS_LOG", "21")
    k_of = lambda plans: [p["K"] for p in plans if p["kind"] == 0][0]
    ctx = product.ProverContext(0)
    try:
        ctx.upload(cases.trace("K2").blocks)
        prev = cases.prove(ctx, "K2", 0, None)
        assert k_of(ctx.dict_plans()) == 4
        for name, K in (("K3", 3), ("K2", 4), ("K2", 4)):
            ctx.stage(cases.trace(name).blocks)
            prev = cases.prove(ctx, name, 1, prev)
            assert k_of(ctx.dict_plans()) == K
        assert ctx.dict_cache_stats()["cols_rebuilt"] == 0
    finally:
        ctx.close()


def test_host_side_key(gpu_ok, product, cases, monkeypatch):
    """SEZKP_DICT_TAB_CAP (16, 4) and the plan-rows hook between proves of one
    trace: each change rebuilds every column, and so does switching back; an
    unchanged setting reuses all."""
    ctx = product.ProverContext(0)
    try:
        ctx.upload(cases.trace("A").blocks)
        cases.prove(ctx, "A", 0, None)
        for key, values in (("SEZKP_DICT_TAB_CAP", ("16", "4")), ("SEZKP_TEST_DICT_PLAN_ROWS_LOG", ("20", "12"))):
            for v in values:
                monkeypatch.setenv(key, v)
                cases.prove(ctx, "A", 1, "A", everything=True)
                cases.prove(ctx, "A", 2, "A")
                assert ctx.dict_cache_stats()["cols_rebuilt"] == 0
            monkeypatch.delenv(key)
            cases.prove(ctx, "A", 0, "A", everything=True)
            cases.prove(ctx, "A", 1, "A")
    finally:
        ctx.close()


def test_off_switch(gpu_ok, product, cases, monkeypatch):
    """SEZKP_DICT_CACHE=0: every prove rebuilds every column, with the bytes
    of the cache; switched on again, the tables the last prove built are
    reused."""
    ctx = product.ProverContext(0)
    try:
        ctx.upload(cases.trace("A").blocks)
        cases.prove(ctx, "A", 0, None)
        monkeypatch.setenv("SEZKP_DICT_CACHE", "0")
        for root in range(3):
            cases.prove(ctx, "A", root, "A", everything=True)
        monkeypatch.setenv("SEZKP_DICT_CACHE", "1")
        cases.prove(ctx, "A", 0, "A")
        assert ctx.dict_cache_stats()["cols_rebuilt"] == 0
    finally:
        ctx.close()


def test_refused_proof_in_between(gpu_ok, product, cases, monkeypatch):
    """Good, refused, good: SEZKP_DEBUG_TRIP_GUARD=0 (read per prove) sets the
    context's guard word behind the column commitment, so the proof is refused
    without a fault after its plan kernel has stored the keys. The next proof
    must not trust them: it rebuilds every column, and matches; the one after
    it reuses all."""
    ctx = product.ProverContext(0)
    try:
        ctx.upload(cases.trace("A").blocks)
        cases.prove(ctx, "A", 0, None)
        cases.prove(ctx, "A", 1, "A")
        assert ctx.dict_cache_stats()["cols_rebuilt"] == 0
        monkeypatch.setenv("SEZKP_DEBUG_TRIP_GUARD", "0")
        with pytest.raises(product.SezkpError):
            ctx.prove(ROOTS[2])
        monkeypatch.delenv("SEZKP_DEBUG_TRIP_GUARD")
        cases.prove(ctx, "A", 2, "A", everything=True)
        assert ctx.dict_cache_stats()["cols_rebuilt"] == 9
        cases.prove(ctx, "A", 0, "A")
        assert ctx.dict_cache_stats()["cols_rebuilt"] == 0
    finally:
        ctx.close()


def test_uploads(gpu_ok, product, cases):
    """An upload of the same shape keeps the reuse of the columns whose key
    repeats; an upload of another shape (2^13 rows) rebuilds every column, and
    so does going back to the first shape."""
    ctx = product.ProverContext(0)
    try:
        ctx.upload(cases.trace("A").blocks)
        cases.prove(ctx, "A", 0, None)
        ctx.upload(cases.trace("B").blocks)
        assert ctx.dict_cache_stats() == {"cols_rebuilt": 0, "cols_reused": 0, "entries_rebuilt": 0}
        cases.prove(ctx, "B", 1, "A")
        assert ctx.dict_cache_stats()["cols_rebuilt"] == len(B_DIFFERS)
        ctx.upload(cases.trace("L").blocks)
        cases.prove(ctx, "L", 0, "B", everything=True)
        cases.prove(ctx, "L", 1, "L")
        ctx.upload(cases.trace("B").blocks)
        cases.prove(ctx, "B", 2, "L", everything=True)
        cases.prove(ctx, "B", 0, "B")
        assert ctx.dict_cache_stats()["cols_rebuilt"] == 0
    finally:
        ctx.close()


def test_async_two_contexts(gpu_ok, product, cases):
    """Two prove_async / wait_view rounds on two contexts at once; the counts
    are each context's own, and refused while its proof is in flight."""
    ta, tb = cases.trace("A"), cases.trace("B")
    c1, c2 = product.ProverContext(0), product.ProverContext(0)
    try:
        c1.upload(ta.blocks)
        c2.upload(tb.blocks)
        c1.prove_async(ROOTS[0])
        c2.prove_async(ROOTS[0])
        with pytest.raises(product.SezkpError, match="in flight"):
            c1.dict_cache_stats()
        assert bytes(c1.wait_view()) == ta.want[0] and bytes(c2.wait_view()) == tb.want[0]
        cases.check(c1, "A", None)
        cases.check(c2, "B", None)
        c1.stage(tb.blocks)
        c1.prove_async(ROOTS[1])
        c2.prove_async(ROOTS[1])
        assert bytes(c1.wait_view()) == tb.want[1] and bytes(c2.wait_view()) == tb.want[1]
        cases.check(c1, "B", "A")
        cases.check(c2, "B", "B")
        assert c1.dict_cache_stats()["cols_rebuilt"] == len(B_DIFFERS)
        assert c2.dict_cache_stats()["cols_rebuilt"] == 0
    finally:
        c1.close()
        c2.close()


def test_no_dict_reports_zeros(gpu_ok, product, cases, monkeypatch):
    """With SEZKP_NO_DICT=1 there are no dictionary columns: all counts 0; the
    C entry point refuses null arguments."""
    import ctypes as C
    tr = cases.trace("A")
    ctx = product.ProverContext(0)
    try:
        ctx.upload(tr.blocks)
        ctx.prove(ROOTS[0])
        u, w = C.c_uint32(), C.c_uint64()
        assert product.lib.sezkp_ctx_dict_cache_stats(ctx._h, None, C.byref(u), C.byref(w)) == -1
        assert product.lib.sezkp_ctx_dict_cache_stats(ctx._h, C.byref(u), C.byref(u), None) == -1
        assert product.lib.sezkp_ctx_dict_cache_stats(None, C.byref(u), C.byref(u), C.byref(w)) == -1
        monkeypatch.setenv("SEZKP_NO_DICT", "1")
        ctx.upload(tr.blocks)
        assert ctx.prove(ROOTS[1]).proof_bytes == tr.want[1]
        assert ctx.dict_cache_stats() == {"cols_rebuilt": 0, "cols_reused": 0, "entries_rebuilt": 0}
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
        for root in ROOTS[:2]:
            proof = ctx.prove(root).proof_bytes
            out.append((hashlib.sha256(proof).hexdigest(), ctx.dict_cache_stats(), ctx.dict_plans()))
        ctx.close()
        q.put((rank, out))
    except Exception as e:
        q.put((rank, f"ERR {type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


def test_sharded_p2_host_collectives(gpu_ok, product, cases):
    """P = 2 over host collectives (two ranks sharing the GPU), T = 2^13: the
    second proof rebuilds no column on either rank, the plans stay, and every
    rank returns the bytes of the single-device proof (the oracle's)."""
    import torch.multiprocessing as mp
    tr = cases.trace("L")
    single = product.ProverContext(0)
    try:
        single.upload(tr.blocks)
        want = [single.prove(r).proof_bytes for r in ROOTS[:2]]
    finally:
        single.close()
    assert want == [tr.want[0], tr.want[1]]
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
        (d1, s1, p1), (d2, s2, p2) = out
        assert [d1, d2] == [hashlib.sha256(w).hexdigest() for w in want], rank
        assert (s1["cols_rebuilt"], s1["cols_reused"]) == (9, 0) and s1["entries_rebuilt"] > 0, (rank, s1)
        assert s2 == {"cols_rebuilt": 0, "cols_reused": 9, "entries_rebuilt": 0}, (rank, s2)
        assert p1 == p2 and len(p1) == 9, rank
