"""GPU parity of the dictionary commitment's large-shape forms at 2^16 and 2^17 rows.

`make_plan` (csrc/dict_commit.hip) gives a commit lane 2^(6 + a) rows, and `a` > 0
needs a device with 2^21 rows or more, so below that only the `a` = 0 forms of
`dict_lane`, `k_col_commit_dict` and `k_col_open` run. The test hook
`SEZKP_TEST_DICT_PLAN_ROWS_LOG=<v>` makes the planner choose K and `a` as on a
device with 2^v rows; `ProverContext.dict_plans()` reports what it chose.
Every trace here is built so that each column lands on a chosen form, the
plan is asserted against the hand-derived ladder below, and the proof is
compared with `oracle.prove_v1` under three manifest roots (the query rows
move with the root) at v = 22, 21 and 20 on one resident context. The ladder
and the oracle's bytes are the checks; `model_plan` restates `make_plan` line
by line, so its agreement with the device is no independent evidence: it
pins the fields the ladder does not name (R, dR, min) and shows where the
ladder and the code part ways.

T = 2^16 = 2^(14 + 2): every commit workgroup (256 lanes) is full at a <= 2,
as in production, and a column at a = 2 is ONE workgroup. The fourth trace
has T = 2^17: at v = 22 its K >= 3 columns are committed by two full a = 2
workgroups (the second one's rows, chunk roots, stored levels and openings
start at 2^16) and its K = 2 and delta columns by four a = 1 workgroups.

The ladder (cost of level K = table entries + rows / 2^K, lower K on ties;
(K, a) per v = 22 / 21 / 20; keys: int8 input_mv and mv, uint8 write flag,
uint16 wsym, int32 head):

    R = 1            (4,2) (4,1) (4,0)
    R = 2            (4,2) (4,1) (3,0)    costs tie at v = 20
    R = 3, 4         (3,2) (3,1) (3,0)    R = 4: T_3 is exactly full (65536)
    R = 5..16        (2,1) (2,0) (2,0)    R = 16: T_2 is exactly full
    R = 17..256      (1,0)                R = 256: T_1 is exactly full
    R = 257..65536   (0,0)
    R > 65536        (-1,0)               leaves hashed
    head, 17 <= R <= 256 and R dR^3 <= 65536:
                     delta plan, K = 2: (2,1) (2,0) (2,0)

a = max(0, extra(K) - (22 - v)) with extra = 2, 2, 1 for K = 4, 3, 2. With
SEZKP_DICT_TAB_CAP = c the tables above level 0 hold at most c entries (at
v = 22; no head of these traces then has R^2 <= c, so no delta plan):

    c = 16:  R = 1 (4,2)   R = 2 (2,1)   R = 3, 4 (1,0)   R = 5..65536 (0,0)
    c = 4:   R = 1 (4,2)   R = 2 (1,0)   R = 3..65536 (0,0)

Forms the union of the observed (key, K, a, delta) tuples must cover
(`REQUIRED`, asserted by test_dict_forms_covered):

    int8   (1,0) (2,1) (2,0) (3,2) (3,1) (3,0) (4,2) (4,1) (4,0)
    uint16 the same and (0,0)
    uint8  (4,2) (4,1), and (2,1) / (1,0) with SEZKP_DICT_TAB_CAP = 16 / 4
    int32  (4,2) (4,1) (3,2) (3,1) (2,1) (1,0) (0,0) (-1,0), not delta
    int32  delta (2,1) (2,0), blocks of 333 and 1023 rows (a block starts at
           each inner position of a 4-row head group), dmin = -1, min < 0

Column data: values are drawn uniformly over the range, with runs of 32 rows
of the largest and of the smallest value planted at both sides of every
multiple of 2^14 rows (2^16 among them) and at both ends of the trace: the
first and the last lane of every workgroup (at a = 0, 1, 2) gather the last and the first entry
of the table at every level. Heads are designed as values and the moves
derived from them, so a head range is exact.
"""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VS = (22, 21, 20)
ROOTS = [bytes(32), bytes(range(32)), hashlib.sha256(b"dictionary forms").digest()]
KEY = {0: "int8", 3: "int8", 4: "uint8", 5: "uint16", 6: "int32"}
DICT_CAP = 65536


def _ladder(R, v, cap=DICT_CAP, delta=False):
    """The hand-derived (K, a) of a column of range R (module docstring)."""
    if delta:
        K = 2
    elif R > DICT_CAP:
        K = -1
    elif cap == DICT_CAP:
        K = 4 if R == 1 else (3 if v == 20 else 4) if R == 2 else 3 if R <= 4 else 2 if R <= 16 else 1 if R <= 256 else 0
    elif cap == 16:
        K = 4 if R == 1 else 2 if R == 2 else 1 if R <= 4 else 0
    else:
        assert cap == 4
        K = 4 if R == 1 else 1 if R == 2 else 0
    return K, max(0, {4: 2, 3: 2, 2: 1}.get(K, 0) - (22 - v))


REQUIRED = (
    {("int8", K, a, 0) for K, a in [(1, 0), (2, 1), (2, 0), (3, 2), (3, 1), (3, 0), (4, 2), (4, 1), (4, 0)]}
    | {("uint16", K, a, 0) for K, a in [(0, 0), (1, 0), (2, 1), (2, 0), (3, 2), (3, 1), (3, 0), (4, 2), (4, 1), (4, 0)]}
    | {("uint8", K, a, 0) for K, a in [(4, 2), (4, 1), (2, 1), (1, 0)]}
    | {("int32", K, a, 0) for K, a in [(4, 2), (4, 1), (3, 2), (3, 1), (2, 1), (1, 0), (0, 0), (-1, 0)]}
    | {("int32", 2, 1, 1), ("int32", 2, 0, 1)}
)


def model_plan(lo, hi, mv_range, n, nrows, cap=DICT_CAP):
    """make_plan (csrc/dict_commit.hip) restated line by line: the plan of a column
    with values in [lo, hi] (mv_range: the tape's move range, head columns
    only). Not an independent check of K and a (the ladder is); it supplies
    the expected R, dR and min."""
    R = hi - lo + 1
    K, delta, dR = -1, 0, 0
    if R <= DICT_CAP:
        best, tabcost, sz, is_open = 2 * nrows, 0, R, True
        for k in range(5):
            is_open = is_open and (1 << k) <= n and sz <= (cap if k else DICT_CAP)
            if is_open:
                tabcost += sz
                if tabcost + (nrows >> k) < best:
                    best, K = tabcost + (nrows >> k), k
                sz *= sz
        if mv_range is not None:
            d = mv_range[1] - mv_range[0] + 1
            if K <= 1 and n >= 4 and R * R <= cap and d <= 256 and R * d ** 3 <= cap:
                K, delta, dR = 2, 1, d
    a = 2 if K >= 3 else (1 if K == 2 else 0)
    r = nrows
    while r < (1 << 22) and a > 0:
        a -= 1
        r <<= 1
    return {"K": K, "a": a, "delta": delta, "R": R if R <= DICT_CAP else 0, "dR": dR, "min": lo}


# ------------------------------------------------------------------ trace data
def _plant(col, lo, hi):
    """Runs of 32 rows of hi before and of lo after every multiple of 2^14
    rows, and both in the first and the last 64 rows."""
    col = np.array(col)
    n = col.shape[0]
    for m in range(0, n + 1, 1 << 14):
        if m > 0:
            col[m - 32:m] = hi
        if m < n:
            col[m:m + 32] = lo
    col[32:64] = hi
    col[n - 64:n - 32] = lo
    return col


def _iid(rng, n, lo, R):
    return _plant(rng.integers(lo, lo + R, n), lo, lo + R - 1)


def _moves(head, b):
    """The moves whose block-local running sum is `head` (blocks of b rows)."""
    prev = np.concatenate([[0], head[:-1]])
    prev[np.arange(head.size) % b == 0] = 0
    return head - prev


def _heads(mv, b):
    """Post-move heads: the running sum of mv, restarting at every block."""
    c = np.cumsum(mv.astype(np.int64))
    start = (np.arange(mv.size) // b) * b
    return c - np.where(start > 0, c[start - 1], 0)


def _walk(rng, n, b, bound):
    """A {-1, 0, 1} walk per block, reflected into [-bound, bound] (a reflected
    lattice walk keeps its step sizes)."""
    x = _heads(rng.integers(-1, 2, n), b)
    z = (x + bound) % (4 * bound)
    return np.where(z <= 2 * bound, z, 4 * bound - z) - bound


class Trace:
    def __init__(self, product, b, imv, heads, mvs, flags, syms):
        """Per tape: heads[t] (values, moves derived) or mvs[t] (moves);
        flags[t] / syms[t]: the write flag and the symbol (committed as
        flag * symbol)."""
        self.b, self.tau, self.T = b, len(flags), len(imv)
        mv = np.zeros((self.T, self.tau), np.int64)
        for t in range(self.tau):
            mv[:, t] = _moves(heads[t], b) if heads[t] is not None else mvs[t]
        assert np.abs(mv).max() <= 127 and -128 <= imv.min() and imv.max() <= 127
        hw = np.stack(flags, axis=1).astype(np.uint8)
        ws = (np.stack(syms, axis=1) * hw).astype(np.uint16)
        self.blocks = product.partition(np.asarray(imv, np.int8), mv.astype(np.int8), hw, ws, b)
        # what the device commits, per (kind, tape)
        self.cols = {(0, 0): np.asarray(imv, np.int64)}
        for t in range(self.tau):
            self.cols[(3, t)] = mv[:, t]
            self.cols[(4, t)] = hw[:, t].astype(np.int64)
            self.cols[(5, t)] = ws[:, t].astype(np.int64)
            self.cols[(6, t)] = _heads(mv[:, t], b)
            if heads[t] is not None:
                assert (self.cols[(6, t)] == heads[t]).all()
        self.want = {}

    def range_of(self, key):
        c = self.cols[key]
        return int(c.min()), int(c.max())


def _trace_ladder_a(product):
    """T = 2^16, b = 512. Heads of range 2, 4, 16 (K = 4, 3, 2 on int32 keys,
    min < 0) and a drifting head (K = 0); int8 ranges 256 (min = -128), 3, 7,
    31, 2; uint16 ranges 65536, 4, 257 (min = 1000), 1; flags of range 1, 2,
    1, 1."""
    rng = np.random.default_rng(101)
    n = 1 << 16
    one, zero = np.ones(n, np.int64), np.zeros(n, np.int64)
    tr = Trace(product, 512, _iid(rng, n, -128, 256),
               heads=[_iid(rng, n, -1, 2), _iid(rng, n, -2, 4), _iid(rng, n, -8, 16), None],
               mvs=[None, None, None, _plant((rng.random(n) < 0.75).astype(np.int64), 0, 1)],
               flags=[one, _plant(rng.integers(0, 2, n), 0, 1), one, zero],
               syms=[_iid(rng, n, 0, 65536), _iid(rng, n, 0, 4), _iid(rng, n, 1000, 257), zero])
    tr.ranges = {(0, 0): (-128, 256), (6, 0): (-1, 2), (3, 0): (-1, 3), (5, 0): (0, 65536), (4, 0): (1, 1),
                 (6, 1): (-2, 4), (3, 1): (-3, 7), (4, 1): (0, 2), (5, 1): (0, 4),
                 (6, 2): (-8, 16), (3, 2): (-15, 31), (5, 2): (1000, 257), (4, 2): (1, 1),
                 (3, 3): (0, 2), (4, 3): (0, 1), (5, 3): (0, 1)}
    tr.delta = set()
    lo, hi = tr.range_of((6, 3))  # the drifting head: some range above 256
    assert 256 < hi - lo + 1 <= DICT_CAP
    return tr


def _trace_ladder_b(product):
    """T = 2^16, b = 333: blocks start at every position of a 4-row group.
    Tape 0: a reflected walk in [-12, 12] (delta plan, dmin = -1, min = -12);
    tape 1: +1 per row (head 1..333: K = 0; mv R = 1); tape 2: head of range
    64 with moves of range 127 (K = 1, R dR^3 > 65536: not delta); tape 3:
    head of range 3, moves of range 5. int8 input range 16; uint16 ranges 16,
    17, 5 (min = 7), 3."""
    rng = np.random.default_rng(202)
    n = 1 << 16
    one = np.ones(n, np.int64)
    tr = Trace(product, 333, _iid(rng, n, -8, 16),
               heads=[_walk(rng, n, 333, 12), None, _iid(rng, n, -32, 64), _iid(rng, n, -1, 3)],
               mvs=[None, one, None, None],
               flags=[_plant(rng.integers(0, 2, n), 0, 1), one, one, _plant(rng.integers(0, 2, n), 0, 1)],
               syms=[_iid(rng, n, 0, 16), _iid(rng, n, 0, 17), _iid(rng, n, 7, 5), _iid(rng, n, 0, 3)])
    tr.ranges = {(0, 0): (-8, 16), (6, 0): (-12, 25), (3, 0): (-1, 3), (4, 0): (0, 2), (5, 0): (0, 16),
                 (3, 1): (1, 1), (6, 1): (1, 333), (4, 1): (1, 1), (5, 1): (0, 17),
                 (6, 2): (-32, 64), (3, 2): (-63, 127), (4, 2): (1, 1), (5, 2): (7, 5),
                 (6, 3): (-1, 3), (3, 3): (-2, 5), (4, 3): (0, 2), (5, 3): (0, 3)}
    tr.delta = {(6, 0)}
    return tr


def _trace_ladder_c(product):
    """T = 2^16, b = 1023. Tape 0: +127 per row (head range 129795 > 65536:
    K = -1); tape 1: a {-1, 0, 1} walk over 1023-row blocks (delta plan, a
    wide T_1); tape 2: head of range 4 with min = 0 (T_3 exactly full). int8
    input range 4 (T_3 exactly full on int8 keys); uint16 ranges 2, 1 (the
    constant 0xFFFF), 256."""
    rng = np.random.default_rng(303)
    n = 1 << 16
    one = np.ones(n, np.int64)
    tr = Trace(product, 1023, _iid(rng, n, -2, 4),
               heads=[None, _walk(rng, n, 1023, 100), _iid(rng, n, 0, 4)],
               mvs=[127 * one, None, None],
               flags=[one, one, one],
               syms=[_iid(rng, n, 0, 2), 0xFFFF * one, _iid(rng, n, 0, 256)])
    tr.ranges = {(0, 0): (-2, 4), (3, 0): (127, 1), (6, 0): (127, 1023 * 127 - 126), (4, 0): (1, 1), (5, 0): (0, 2),
                 (3, 1): (-1, 3), (4, 1): (1, 1), (5, 1): (0xFFFF, 1),
                 (6, 2): (0, 4), (3, 2): (-3, 7), (4, 2): (1, 1), (5, 2): (0, 256)}
    tr.delta = {(6, 1)}
    lo, hi = tr.range_of((6, 1))  # the walk's range: data, within the delta plan's bounds
    assert lo < 0 and 17 <= hi - lo + 1 <= 256
    return tr


def _trace_two_workgroups(product):
    """T = 2^17, b = 701 (not a multiple of 4). At v = 22 every K >= 3 column
    takes two full a = 2 workgroups and every K = 2 / delta column four a = 1
    workgroups, with runs of extreme codes on both sides of row 2^16 (the
    last lanes of one workgroup, the first of the next), so the second
    workgroup's row offset, chunk-root and stored-level indices and the
    openings of its chunks are compared with the oracle. int8: input range 2
    (K = 4), moves of range 7, 3, 3; heads of range 4 (T_3 full, min = -3),
    41 (reflected walk: delta plan) and 2; flags of range 2, 1, 1; uint16
    ranges 3, 16 (T_2 full), 4 (min = 100, T_3 full)."""
    rng = np.random.default_rng(404)
    n = 1 << 17
    one = np.ones(n, np.int64)
    tr = Trace(product, 701, _iid(rng, n, -1, 2),
               heads=[_iid(rng, n, -3, 4), _walk(rng, n, 701, 20), _iid(rng, n, 0, 2)],
               mvs=[None, None, None],
               flags=[_plant(rng.integers(0, 2, n), 0, 1), one, one],
               syms=[_iid(rng, n, 0, 3), _iid(rng, n, 0, 16), _iid(rng, n, 100, 4)])
    tr.ranges = {(0, 0): (-1, 2), (6, 0): (-3, 4), (3, 0): (-3, 7), (4, 0): (0, 2), (5, 0): (0, 3),
                 (6, 1): (-20, 41), (3, 1): (-1, 3), (4, 1): (1, 1), (5, 1): (0, 16),
                 (6, 2): (0, 2), (3, 2): (-1, 3), (4, 2): (1, 1), (5, 2): (100, 4)}
    tr.delta = {(6, 1)}
    return tr


BUILDERS = {"a_b512": _trace_ladder_a, "b_b333": _trace_ladder_b, "c_b1023": _trace_ladder_c,
            "d_2p17_b701": _trace_two_workgroups}


def _check_plans(tr, plans, v, cap=DICT_CAP):
    """Every dictionary column's plan against the ladder (K, a, delta) and
    the restated planner (R, dR, min too); returns the forms seen."""
    assert len(plans) == 1 + 4 * tr.tau
    assert {(p["kind"], p["tape"]) for p in plans} == set(tr.cols)
    seen = set()
    for p in plans:
        key = (p["kind"], p["tape"])
        lo, hi = tr.range_of(key)
        delta = key in tr.delta and cap == DICT_CAP
        K, a = _ladder(hi - lo + 1, v, cap, delta)
        assert (p["K"], p["a"], p["delta"]) == (K, a, int(delta)), (key, v, cap, p)
        mvr = tr.range_of((3, key[1])) if key[0] == 6 else None
        got = {f: p[f] for f in ("K", "a", "delta", "R", "dR", "min")}
        assert got == model_plan(lo, hi, mvr, tr.T, 1 << v, cap), (key, v, cap)
        seen.add((KEY[key[0]], p["K"], p["a"], p["delta"]))
    return seen


class Forms:
    """The traces, their oracle proofs and the forms observed so far: built
    and run once per module, whichever test asks first."""

    def __init__(self, product, oracle):
        self.product, self.oracle = product, oracle
        self.traces, self.done, self.observed = {}, set(), set()

    def trace(self, name):
        if name not in self.traces:
            tr = BUILDERS[name](self.product)
            for key, (lo, R) in tr.ranges.items():  # the data has the designed ranges
                assert tr.range_of(key) == (lo, lo + R - 1), (name, key)
            tr.want = [self.oracle.prove_v1(tr.blocks, r) for r in ROOTS]
            self.traces[name] = tr
        return self.traces[name]

    def run(self, name, monkeypatch):
        """v = 22, 21, 20 on one resident context (each prove replans and
        rebuilds the tables), three roots each."""
        if name in self.done:
            return
        tr = self.trace(name)
        ctx = self.product.ProverContext(0)
        try:
            ctx.upload(tr.blocks)
            assert ctx.dict_plans() == []  # nothing proved yet on this upload
            for v in VS:
                monkeypatch.setenv("SEZKP_TEST_DICT_PLAN_ROWS_LOG", str(v))
                for root, want in zip(ROOTS, tr.want):
                    assert ctx.prove(root).proof_bytes == want, (name, v, root[:4].hex())
                self.observed |= _check_plans(tr, ctx.dict_plans(), v)
        finally:
            ctx.close()
        self.done.add(name)

    def run_caps(self, monkeypatch):
        """Trace a at v = 22 with SEZKP_DICT_TAB_CAP = 16 and 4."""
        if "caps" in self.done:
            return
        tr = self.trace("a_b512")
        monkeypatch.setenv("SEZKP_TEST_DICT_PLAN_ROWS_LOG", "22")
        ctx = self.product.ProverContext(0)
        try:
            ctx.upload(tr.blocks)
            for cap, form in ((16, (2, 1)), (4, (1, 0))):
                monkeypatch.setenv("SEZKP_DICT_TAB_CAP", str(cap))
                for root, want in zip(ROOTS, tr.want):
                    assert ctx.prove(root).proof_bytes == want, (cap, root[:4].hex())
                plans = ctx.dict_plans()
                seen = _check_plans(tr, plans, 22, cap)
                flag = [p for p in plans if (p["kind"], p["tape"]) == (4, 1)][0]
                assert (flag["R"], flag["K"], flag["a"]) == (2,) + form
                self.observed |= {s for s in seen if s[0] == "uint8"}
        finally:
            ctx.close()
        self.done.add("caps")


@pytest.fixture(scope="module")
def forms(product, oracle):
    return Forms(product, oracle)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_dict_forms_bit_exact(gpu_ok, forms, monkeypatch, name):
    """Each designed trace at v = 22, 21, 20 under three manifest roots: the
    plans are the ladder's and every proof equals the oracle's."""
    forms.run(name, monkeypatch)


def test_dict_forms_table_caps(gpu_ok, forms, monkeypatch):
    """SEZKP_DICT_TAB_CAP = 16 and 4 at v = 22: every column follows the
    capped ladder (the flag column of range 2 drops to K = 2, a = 1 and to
    K = 1); same bytes."""
    forms.run_caps(monkeypatch)


def test_dict_forms_staged_and_reproved(gpu_ok, product, oracle, forms, monkeypatch):
    """The b = 333 trace at v = 22 as a staged upload over another trace of
    the same shape (whose plans and tables the workspace still holds), proved
    twice on the resident context."""
    tr = forms.trace("b_b333")
    monkeypatch.setenv("SEZKP_TEST_DICT_PLAN_ROWS_LOG", "22")
    other = product.synthetic_blocks(tr.T, tr.b, tr.tau, 5)
    ctx = product.ProverContext(0)
    try:
        ctx.upload(other)
        assert ctx.prove(ROOTS[1]).proof_bytes == oracle.prove_v1(other, ROOTS[1])
        ctx.stage(tr.blocks)
        assert ctx.prove(ROOTS[1]).proof_bytes == tr.want[1]
        _check_plans(tr, ctx.dict_plans(), 22)
        assert ctx.prove(ROOTS[2]).proof_bytes == tr.want[2]
        assert ctx.prove(ROOTS[1]).proof_bytes == tr.want[1]
    finally:
        ctx.close()


def test_dict_plans_off_and_in_flight(gpu_ok, product, monkeypatch):
    """dict_plans() is empty with SEZKP_NO_DICT=1 and refused while a proof
    is in flight; the C entry point refuses a null output and a negative
    count, and writes no more than `max` entries."""
    from sezkp_amd._lib import DictPlanInfo
    blocks = product.synthetic_blocks(1 << 12, 512, 2, 3)
    root = blocks.manifest_root()
    ctx = product.ProverContext(0)
    try:
        ctx.upload(blocks)
        ctx.prove_async(root)
        with pytest.raises(product.SezkpError, match="in flight"):
            ctx.dict_plans()
        ctx.wait_view()
        assert len(ctx.dict_plans()) == 9
        buf = (DictPlanInfo * 9)()
        assert product.lib.sezkp_ctx_dict_plans(ctx._h, None, 9) == -1
        assert product.lib.sezkp_ctx_dict_plans(ctx._h, buf, -1) == -1
        assert product.lib.sezkp_ctx_dict_plans(ctx._h, None, 0) == 0
        buf[2].col = 0xFFFF
        assert product.lib.sezkp_ctx_dict_plans(ctx._h, buf, 2) == 2 and buf[2].col == 0xFFFF
        monkeypatch.setenv("SEZKP_NO_DICT", "1")
        ctx.upload(blocks)
        ctx.prove(root)
        assert ctx.dict_plans() == []
    finally:
        ctx.close()


def test_dict_plan_hook_keeps_workgroups_full(gpu_ok, product, oracle, monkeypatch):
    """Below 2^16 rows the hook lowers v so that no commit workgroup is partly
    filled at a > 0: 2^15 rows at v = 22 plan as at v = 21 (a <= 1), 2^14 rows
    and fewer as at v = 20 (a = 0). Same bytes."""
    monkeypatch.setenv("SEZKP_TEST_DICT_PLAN_ROWS_LOG", "22")
    ctx = product.ProverContext(0)
    try:
        for logt, a_max in ((15, 1), (14, 0), (12, 0)):
            blocks = product.synthetic_blocks(1 << logt, 333, 2, logt)
            root = blocks.manifest_root()
            ctx.upload(blocks)
            assert ctx.prove(root).proof_bytes == oracle.prove_v1(blocks, root)
            plans = ctx.dict_plans()
            # moves in {-1, 0, 1} and flags: K >= 3, which a full-size device gives a = 2
            assert all(p["K"] >= 3 for p in plans if p["kind"] in (0, 3, 4))
            assert max(p["a"] for p in plans) == a_max, (logt, plans)
            assert all(p["a"] == a_max for p in plans if p["K"] >= 3), (logt, plans)
    finally:
        ctx.close()


def test_dict_forms_covered(gpu_ok, forms, monkeypatch):
    """The union of the observed (key, K, a, delta) tuples covers REQUIRED
    (whatever the other tests of this module have not run yet runs here)."""
    for name in sorted(BUILDERS):
        forms.run(name, monkeypatch)
    forms.run_caps(monkeypatch)
    assert REQUIRED <= forms.observed, sorted(REQUIRED - forms.observed)
