"""Full-trace AIR audit (sezkp_ctx_air_audit / k_air_audit) against a numpy
restatement of the five per-cell terms, itself anchored to the oracle's
compose() (air.rs:49-136 with the alpha reuse of prover.rs:86-98).

Families (SEZKP_AIR_FAMILIES order): mv_domain, head_range, slack_range,
sym_range, boundary. A row is violating when a cell of a family is non-zero,
rejectable when the sum over the tapes of term 0 or of term 4 is non-zero in
the field (the reference verifier's opened-row check, verify.rs:156-182).
"""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG

P = 0xFFFFFFFF00000001
NO_ROW = (1 << 64) - 1
FAMS = ("mv_domain", "head_range", "slack_range", "sym_range", "boundary")
# unit alpha of compose() that isolates the family's sum over the tapes:
# a[1] mv_domain, a[4] head reconstruct, a[6] slack reconstruct, a[0] bool_flag
# (identically 0) + symbol reconstruct, a[2] head_update (identically 0) +
# both boundary terms
ALPHA_OF = (1, 4, 6, 0, 2)
HI48 = np.uint64(0xFFFFFFFFFFFF0000)
NEG1_HI = (P - 1) & ~0xFFFF  # canonical -1 minus its low 16 bits

SYNTH = [(4096, 512, 8, 42), (2048, 100, 3, 2), (256, 1, 1, 3), (8, 8, 2, 4), (2, 2, 1, 5), (1, 1, 1, 6),
         (512, 512, 0, 7), (1 << 13, 8192, 4, 8)]


# ------------------------------------------------------------ restatement
def _canon(x):
    """int64 array -> canonical Goldilocks values (u64); |x| < 2^63 << p."""
    x = np.asarray(x, np.int64)
    u = x.astype(np.uint64)
    return np.where(x >= 0, u, u + np.uint64(P))  # 2^64 + x + p wraps to p + x


class Cells:
    """t[k, i, r]: canonical term of family k at row i, tape r; nz[k, i, r]:
    the cell counts for family k; s0 / s4: the integer sums over the tapes of
    the mv_domain and boundary terms (below p in magnitude, so zero in the
    field iff zero)."""

    def __init__(self, blocks):
        tau, nb = blocks.tau, blocks.n_blocks
        ss = blocks.step_start.astype(np.int64)
        n = int(ss[-1])
        blk = np.repeat(np.arange(nb), np.diff(ss))
        row = np.arange(n, dtype=np.int64)
        m = blocks.mv.reshape(n, tau).astype(np.int64)
        f = blocks.has_write.reshape(n, tau) != 0
        s = np.where(f, blocks.wsym.reshape(n, tau), 0).astype(np.uint64)
        c = np.concatenate([np.zeros((1, tau), np.int64), np.cumsum(m, axis=0)])
        h = c[1:] - c[ss[:-1]][blk]  # block-local post-move head (openings.rs:209-220)
        wl = (np.abs(blocks.win_right.astype(np.int64) - blocks.win_left.astype(np.int64)) + 1).reshape(nb, tau)
        off_in = blocks.off_in.astype(np.int64).reshape(nb, tau)
        off_out = blocks.off_out.astype(np.int64).reshape(nb, tau)
        first = (row == ss[:-1][blk])[:, None]
        last = (row + 1 == ss[1:][blk])[:, None]
        z = np.uint64(0)
        t0i = m * m * m - m
        bf, bl = first * (h - m - off_in[blk]), last * (h - off_out[blk])
        t4i = bf + bl
        self.t = np.stack([
            _canon(t0i),
            np.where(f, _canon(h) & HI48, z),
            np.where(f, _canon(wl[blk] - 1 - h) & HI48, z),
            np.where(f, s & np.uint64(0xFFF0), z),
            _canon(t4i),
        ])
        self.n, self.tau = n, tau
        self.s0, self.s4 = t0i.sum(axis=1), t4i.sum(axis=1)
        # counted cells: the term is non-zero; a boundary cell also when its two
        # terms cancel (a one-row block: -1 + 1). First cells go by the term.
        self.nz = self.t != 0
        self.nz[4] = (bf != 0) | (bl != 0)
        self.viol = self.nz.any(axis=(0, 2))
        self.rej = (self.s0 != 0) | (self.s4 != 0)


def air_cells(blocks):
    return Cells(blocks)


def expected(blocks, c=None):
    """Every field of sezkp_air_audit and both bitmaps, from the restatement."""
    c = c or air_cells(blocks)
    fams = {}
    for k, name in enumerate(FAMS):
        nz = c.nz[k]
        idx = np.flatnonzero((c.t[k] != 0).reshape(-1))  # (row, tape) order
        r, tp = divmod(int(idx[0]), c.tau) if idx.size else (NO_ROW, 0)
        fams[name] = {"cells": int(nz.sum()), "rows": int(nz.any(axis=1).sum()), "first_row": r, "first_tape": tp,
                      "first_value": int(c.t[k][r, tp]) if idx.size else 0}
    first = lambda b: int(np.flatnonzero(b)[0]) if b.any() else NO_ROW
    return {"n_rows": c.n, "tau": c.tau, "families": fams, "rows_violating": int(c.viol.sum()),
            "first_violating": first(c.viol), "rows_rejectable": int(c.rej.sum()), "first_rejectable": first(c.rej),
            "violating_bits": np.packbits(c.viol, bitorder="little").tobytes(),
            "rejectable_bits": np.packbits(c.rej, bitorder="little").tobytes()}


def as_dict(a):
    return {k: getattr(a, k) for k in ("n_rows", "tau", "families", "rows_violating", "first_violating",
                                       "rows_rejectable", "first_rejectable", "violating_bits", "rejectable_bits")}


def check(a, blocks):
    c = air_cells(blocks)
    want = expected(blocks, c)
    got = as_dict(a)
    for k in want:
        assert got[k] == want[k], k
    np.testing.assert_array_equal(a.violating_rows(), np.flatnonzero(c.viol))
    np.testing.assert_array_equal(a.rejectable_rows(), np.flatnonzero(c.rej))
    assert a.ok == (want["rows_violating"] == 0)
    return want


# ------------------------------------------------------------ traces
def clean_arrays(T, tau, seed=1):
    """The valid trace of test_host_abi._valid_trace: moves in {0, 1} (heads
    stay >= 0), symbols < 16."""
    rng = np.random.default_rng(seed)
    mv = rng.integers(0, 2, (T, tau), dtype=np.int8)
    hw = (rng.random((T, tau)) < 0.5).astype(np.uint8)
    ws = (rng.integers(0, 16, (T, tau)) * hw).astype(np.uint16)
    return rng.integers(-1, 2, T, dtype=np.int8), mv, hw, ws


def clean_trace(product, T=512, tau=2, b=64, seed=1):
    return product.partition(*clean_arrays(T, tau, seed), b)


def wide_trace(product):
    """The trace of test_prove_wide_values_bit_exact."""
    rng = np.random.default_rng(11)
    T, tau = 1024, 3
    imv = rng.integers(-128, 128, T, dtype=np.int8)
    mv = rng.integers(-128, 128, (T, tau), dtype=np.int8)
    hw = (rng.random((T, tau)) < 0.7).astype(np.uint8)
    ws = (rng.integers(0, 65536, (T, tau)) * hw).astype(np.uint16)
    blocks = product.partition(imv, mv, hw, ws, 128)
    blocks.win_left[:] = rng.integers(-(1 << 40), 1 << 40, blocks.win_left.size)
    blocks.off_out[:] = 0xFFFFFFFF
    return blocks


def golden_blocks(product):
    return product.BlockSoA.from_cbor(open(os.path.join(GOLDEN, "ref_blocks.cbor"), "rb").read())


def one_block_64k(product):
    """T = 2^16 in a single block (the grid-stride loop, 1024 bitmap words):
    heads wander below 0 and symbols reach 31, every family fires."""
    rng = np.random.default_rng(9)
    T, tau = 1 << 16, 2
    imv = np.zeros(T, np.int8)
    mv = rng.integers(-1, 2, (T, tau), dtype=np.int8)
    mv[rng.integers(0, T, 40), rng.integers(0, tau, 40)] = 2
    hw = (rng.random((T, tau)) < 0.3).astype(np.uint8)
    ws = (rng.integers(0, 32, (T, tau)) * hw).astype(np.uint16)
    return product.partition(imv, mv, hw, ws, T)


def audit_of(product, blocks, ctx=None):
    own = ctx is None
    if own:
        ctx = product.ProverContext(0)
    try:
        ctx.upload(blocks)
        return ctx.air_audit(bitmaps=True)
    finally:
        if own:
            ctx.close()


# ------------------------------------------------------------ the anchor (CPU)
def anchor_cases(product):
    yield "golden", golden_blocks(product)
    yield "wide", wide_trace(product)
    yield "clean", clean_trace(product)
    yield "planted", planted(product, together(0, 2, 1), off_in=True)
    for T, b, tau, seed in SYNTH:
        if T <= 2048:
            yield f"synthetic{(T, b, tau, seed)}", product.synthetic_blocks(T, b, tau, seed)


def test_restatement_matches_oracle_compose(product):
    """The sum over the tapes of each family's terms equals the oracle's
    compose() with the unit alpha that isolates it, on every row of every case
    of at most 2048 rows; the integer form of the rejectable condition equals
    the field one."""
    import cbor_min
    import sezkp_oracle_py as O
    for name, blocks in anchor_cases(product):
        c = air_cells(blocks)
        rows, tau = O.row_snapshots(cbor_min.loads(blocks.to_cbor()))
        assert (len(rows), tau) == (c.n, c.tau), name
        sums = [[sum(int(x) for x in c.t[k][i]) % P for i in range(c.n)] for k in range(5)]
        for k, ak in enumerate(ALPHA_OF):
            e = [0] * 8
            e[ak] = 1
            for i in range(c.n):
                assert O.compose(rows, tau, i, e) == sums[k][i], (name, FAMS[k], i)
        for i in range(c.n):
            assert bool(c.rej[i]) == (sums[0][i] != 0 or sums[4][i] != 0), (name, i)


# ------------------------------------------------------------ clean traces
@pytest.mark.gpu
@pytest.mark.parametrize("T,tau,b", [(512, 2, 64), (1, 1, 1)])
def test_clean_trace_is_clean(gpu_ok, product, T, tau, b):
    blocks = clean_trace(product, T, tau, b)
    a = audit_of(product, blocks)
    assert a.ok and (a.n_rows, a.tau) == (T, tau)
    assert a.rows_violating == 0 and a.rows_rejectable == 0
    assert a.first_violating == NO_ROW and a.first_rejectable == NO_ROW
    for name in FAMS:
        assert a.families[name] == {"cells": 0, "rows": 0, "first_row": NO_ROW, "first_tape": 0, "first_value": 0}
    assert a.violating_bits == bytes((T + 7) // 8) and a.rejectable_bits == bytes((T + 7) // 8)
    assert a.violating_rows().size == 0 and a.rejectable_rows().size == 0
    assert a.verify_reject_probability() == 0.0
    check(a, blocks)


# ------------------------------------------------------------ parity
@pytest.mark.gpu
@pytest.mark.parametrize("T,b,tau,seed", SYNTH)
def test_parity_synthetic(gpu_ok, product, T, b, tau, seed):
    blocks = product.synthetic_blocks(T, b, tau, seed)
    check(audit_of(product, blocks), blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("make", [wide_trace, golden_blocks, one_block_64k])
def test_parity_edge_traces(gpu_ok, product, make):
    blocks = make(product)
    want = check(audit_of(product, blocks), blocks)
    assert want["rows_violating"] > 0  # these traces do break the AIR


@pytest.mark.gpu
@pytest.mark.parametrize("rows_per_lane", ["1", "2", "4"])
def test_parity_every_kernel_form(gpu_ok, product, monkeypatch, rows_per_lane):
    """k_air_audit takes 2 adjacent rows per lane (1 when n = 1) and has
    forms of 1 and 4; SEZKP_AUDIT_ROWS forces a form, so each one sees more than one
    workgroup, the grid-stride loop, a partial word (n < 64) and every family."""
    monkeypatch.setenv("SEZKP_AUDIT_ROWS", rows_per_lane)
    ctx = product.ProverContext(0)
    for blocks in (one_block_64k(product), wide_trace(product), planted(product, together(0, 2, 1), off_in=True),
                   product.synthetic_blocks(8, 8, 2, 4), product.synthetic_blocks(2, 2, 1, 5),
                   # 4096 workgroups' worth of rows for the form: several trips of the capped grid
                   product.synthetic_blocks(1 << {"1": 20, "2": 21, "4": 22}[rows_per_lane], 4096, 1, 6)):
        check(audit_of(product, blocks, ctx), blocks)
    ctx.close()


# ------------------------------------------------------------ planted violations
EDGE_ROWS =(0, 63, 64, 255, 256, 1023)  # wave and workgroup edges, block starts and ends (b = 256)


def planted(product, plants, off_in=False):
    """The clean T = 1024, tau = 3, b = 256 trace with violations planted at
    (kind, row, tape): 0 a move of 2, 1 a write at head -1, 2 a write with
    slack -1 (win_right shrunk below the head), 3 a symbol 16. Kinds 1 and 2
    shape their tape's moves from the block start on (and a block has one
    window per tape), so plants go in from the last row to the first, and
    kinds 0, 1 and 2 cannot share a tape: together() gives each its own."""
    T, tau, b = 1024, 3, 256
    plants = sorted(plants, key=lambda p: -p[1])
    imv, mv, hw, ws = clean_arrays(T, tau)
    blocks = product.partition(imv, mv, hw, ws, b)  # windows and offsets of the clean trace
    mv, hw, ws = (x.reshape(T, tau) for x in (blocks.mv, blocks.has_write, blocks.wsym))
    for kind, r, tp in plants:
        bs = r - r % b
        if kind == 0:
            mv[r, tp] = 2
        elif kind == 1:  # the block steps to -1 and stays there up to row r; only row r writes
            mv[bs:r + 1, tp] = 0
            mv[bs, tp] = -1
            hw[bs:r + 1, tp] = 0
            ws[bs:r + 1, tp] = 0
            hw[r, tp], ws[r, tp] = 1, 3
        elif kind == 2:  # head >= 1 at the written row, window one short of it
            mv[r, tp] = 1
            hw[r, tp], ws[r, tp] = 1, 3
            h = int(mv[bs:r + 1, tp].astype(np.int64).sum())
            blocks.win_right[(r // b) * tau + tp] = blocks.win_left[(r // b) * tau + tp] + h - 1
        else:
            hw[r, tp], ws[r, tp] = 1, 16
    if off_in:
        blocks.off_in[1 * tau + 0] = 1
    return blocks


@pytest.mark.gpu
def test_planted_violations_one_at_a_time(gpu_ok, product):
    ctx = product.ProverContext(0)
    value = {0: 6, 1: NEG1_HI, 2: NEG1_HI, 3: 16}
    for kind in range(4):
        for r in EDGE_ROWS:
            for tp in (0, 2):
                blocks = planted(product, [(kind, r, tp)])
                a = audit_of(product, blocks, ctx)
                check(a, blocks)
                fam = a.families[FAMS[kind]]
                assert (fam["first_row"], fam["first_tape"], fam["first_value"]) == (r, tp, value[kind]), (kind, r, tp)
                assert fam["cells"] >= 1 and r in a.violating_rows()
                if kind == 0:  # the only bad move; it shifts the block's later heads (slack, boundary_last)
                    assert fam["cells"] == 1 and a.first_violating == r and a.first_rejectable == r
                if kind == 3:  # touches nothing else, and no verifier sees a symbol
                    assert fam["cells"] == 1 and (a.rows_violating, a.first_violating) == (1, r)
                    assert a.rows_rejectable == 0
    blocks = planted(product, [], off_in=True)
    a = audit_of(product, blocks, ctx)
    check(a, blocks)
    assert a.families["boundary"] == {"cells": 1, "rows": 1, "first_row": 256, "first_tape": 0, "first_value": P - 1}
    assert (a.rows_violating, a.first_violating, a.rows_rejectable, a.first_rejectable) == (1, 256, 1, 256)
    ctx.close()


def together(x, y, z):
    """Every kind at every edge row: the move of 2 and the symbol 16 on tape
    x, the writes at head -1 on tape y, the writes outside the window on z."""
    return [p for r in EDGE_ROWS for p in ((0, r, x), (3, r, x), (1, r, y), (2, r, z))]


@pytest.mark.gpu
def test_planted_violations_all_together(gpu_ok, product):
    import itertools
    ctx = product.ProverContext(0)
    for x, y, z in itertools.permutations(range(3)):  # each kind on tape 0 and on the last tape, twice
        blocks = planted(product, together(x, y, z), off_in=True)
        a = audit_of(product, blocks, ctx)
        check(a, blocks)
        assert a.families["mv_domain"]["cells"] == 6 and a.families["mv_domain"]["first_tape"] == x
        assert a.families["sym_range"]["cells"] == 6 and a.families["sym_range"]["first_value"] == 16
        for name, tp in (("head_range", y), ("slack_range", z)):
            assert a.families[name]["cells"] >= 6, name
            assert (a.families[name]["first_row"], a.families[name]["first_tape"]) == (0, tp), name
            assert a.families[name]["first_value"] == NEG1_HI, name
        assert a.families["boundary"]["cells"] >= 1
        assert a.first_violating == 0 and a.first_rejectable == 0
        assert set(EDGE_ROWS) <= set(int(r) for r in a.violating_rows())
    ctx.close()


# ------------------------------------------------------------ cancellation
@pytest.mark.gpu
def test_cancellation_across_tapes(gpu_ok, product):
    """Cells that cancel in the verifier's sums over the tapes: the row
    violates the AIR, and no query of it makes the verifier reject."""
    T, tau = 64, 2
    z8, z16 = np.zeros((T, tau), np.uint8), np.zeros((T, tau), np.uint16)
    mv = np.zeros((T, tau), np.int8)
    mv[5] = (2, -2)  # 6 + (-6) = 0
    mv[6] = (-2, 2)  # heads back to 0, and -6 + 6 = 0
    blocks = product.partition(np.zeros(T, np.int8), mv, z8, z16, T)
    # partition's offsets follow the window (off_in = -left = 2 on tape 1):
    # without them the boundary holds, the heads start and end at 0
    blocks.off_in[:] = 0
    blocks.off_out[:] = 0
    a = audit_of(product, blocks)
    check(a, blocks)
    assert a.families["mv_domain"] == {"cells": 4, "rows": 2, "first_row": 5, "first_tape": 0, "first_value": 6}
    assert all(a.families[name]["cells"] == 0 for name in FAMS[1:])
    assert list(a.violating_rows()) == [5, 6] and a.rows_rejectable == 0 and a.first_rejectable == NO_ROW
    assert not a.ok and a.verify_reject_probability() == 0.0


@pytest.mark.gpu
def test_cancellation_inside_a_boundary_cell(gpu_ok, product):
    """One-row blocks, one tape, mv = 1 (h = 1). With off_in = 0, off_out = 1
    both boundary terms vanish. Block 2 with off_in = 1, off_out = 0 has
    is_first (h - m - in_off) = -1 and is_last (h - out_off) = +1: both
    constraints fail, their sum under the prover's single alpha is 0, so the
    row violates the AIR, no verifier query rejects it, and the family has a
    counted cell but no first cell (the first-cell search goes by the sum)."""
    T = 4
    mv = np.ones((T, 1), np.int8)
    blocks = product.partition(np.zeros(T, np.int8), mv, np.zeros((T, 1), np.uint8), np.zeros((T, 1), np.uint16), 1)
    blocks.off_in[:] = 0
    blocks.off_out[:] = 1
    assert audit_of(product, blocks).ok
    blocks.off_in[2], blocks.off_out[2] = 1, 0
    a = audit_of(product, blocks)
    check(a, blocks)
    assert a.families["boundary"] == {"cells": 1, "rows": 1, "first_row": NO_ROW, "first_tape": 0, "first_value": 0}
    assert list(a.violating_rows()) == [2] and (a.rows_violating, a.first_violating) == (1, 2)
    assert a.rows_rejectable == 0 and a.rejectable_rows().size == 0


# ------------------------------------------------------------ the verifier
def _queries(proof):
    import sezkp_oracle_py as O
    return [q["row"] for q in O.parse_proof_v1(proof)["queries"]]


@pytest.mark.gpu
def test_audit_predicts_the_verifier(gpu_ok, product, oracle):
    every = clean_trace(product, 64, 2, 1)
    every.off_in[:] = 1  # -1 on each tape of every (one-row) block: all rows rejectable
    traces = {"clean": clean_trace(product), "every": every, "generator": product.reference_blocks(1024, 64, 2, 42)}
    roots = {"clean": [bytes([k]) * 32 for k in range(3)], "every": [bytes([k]) * 32 for k in range(3)]}
    # the generator's trace: roots chosen on the CPU, with the oracle's proof
    # and the restatement, so that both verdicts occur
    gen = traces["generator"]
    rej = air_cells(gen).rej
    assert 0 < rej.sum() < rej.size
    picked = {}
    for k in range(64):
        root = bytes([k]) * 32
        hit = any(rej[r] for r in _queries(oracle.prove_v1(gen, root)))
        picked.setdefault(hit, []).append(root)
        if len(picked.get(True, [])) >= 2 and len(picked.get(False, [])) >= 2:
            break
    assert len(picked.get(True, [])) >= 1 and len(picked.get(False, [])) >= 1
    roots["generator"] = picked[True][:2] + picked[False][:2]
    verdicts = set()
    for name, blocks in traces.items():
        ctx = product.ProverContext(0)
        ctx.upload(blocks)
        a = ctx.air_audit(bitmaps=True)
        check(a, blocks)
        for root in roots[name]:
            art = ctx.prove(root)
            bad = a.first_rejected_query(_queries(art.proof_bytes))
            if name == "clean":
                assert bad is None
            if name == "every":
                assert bad is not None
            if bad is None:
                product.StarkV1.verify(art, blocks, root)
            else:
                with pytest.raises(product.SezkpError, match=f"AIR composition non-zero at row {bad}$"):
                    product.StarkV1.verify(art, blocks, root)
            if name == "generator":
                verdicts.add(bad is None)
        ctx.close()
    assert verdicts == {True, False}


# ------------------------------------------------------------ context hygiene
@pytest.mark.gpu
def test_audit_leaves_the_context_as_it_was(gpu_ok, product, oracle):
    blocks = product.synthetic_blocks(4096, 512, 8, 42)
    root = blocks.manifest_root()
    want = oracle.prove_v1(blocks, root)
    ctx = product.ProverContext(0)
    ctx.upload(blocks)
    a1 = ctx.air_audit(bitmaps=True)  # before any prove: the audit expands the rows itself
    assert ctx.prove(root).proof_bytes == want
    a2 = ctx.air_audit(bitmaps=True)
    a3 = ctx.air_audit(bitmaps=True)
    assert as_dict(a1) == as_dict(a2) == as_dict(a3)
    a4 = ctx.air_audit()
    assert a4.violating_bits is None and a4.violating_rows() is None and a4.rejectable_rows() is None
    assert a4.families == a1.families and a4.rows_rejectable == a1.rows_rejectable
    assert ctx.prove(root).proof_bytes == want
    # another shape on the same context (the audit's buffers follow n)
    small = product.synthetic_blocks(256, 64, 2, 3)
    check(audit_of(product, small, ctx), small)
    # a staged trace: refused while pending, audited once a prove has consumed it
    nxt = product.synthetic_blocks(256, 64, 2, 4)
    ctx.stage(nxt)
    with pytest.raises(product.SezkpError) as e:
        ctx.air_audit()
    assert e.value.code == -1
    assert ctx.prove(bytes(32)).proof_bytes == oracle.prove_v1(nxt, bytes(32))
    check(ctx.air_audit(bitmaps=True), nxt)
    ctx.close()


@pytest.mark.gpu
def test_audit_refusals(gpu_ok, product):
    ctx = product.ProverContext(0)
    with pytest.raises(product.SezkpError, match="no trace uploaded") as e:
        ctx.air_audit()
    assert e.value.code == -1
    ctx.close()
    solo = product.ShardedProverContext(0, 2, device=0, comm="solo")
    solo.upload(product.synthetic_blocks(1 << 13, 512, 2, 3))
    with pytest.raises(product.SezkpError, match="sharded") as e:
        solo.air_audit()
    assert e.value.code == -1
    solo.close()


@pytest.mark.gpu
def test_audit_head_guard_does_not_poison_the_context(gpu_ok, product, oracle):
    """The input of test_prove_rejects_head_outside_i32: the audit's own
    k_expand trips the i32 head guard; the audit reports it as prove does and
    clears it, and a clean trace uploaded next proves bit-exact."""
    T = 1 << 25
    imv = np.zeros(T, np.int8)
    hw = np.zeros((T, 1), np.uint8)
    ws = np.zeros((T, 1), np.uint16)
    blocks = product.partition(imv, np.full((T, 1), 127, np.int8), hw, ws, T)
    ctx = product.ProverContext(0)
    ctx.upload(blocks)
    with pytest.raises(product.SezkpError, match="i32 range") as e:
        ctx.air_audit()
    assert e.value.code == -1
    good = clean_trace(product)
    root = good.manifest_root()
    ctx.upload(good)
    assert ctx.prove(root).proof_bytes == oracle.prove_v1(good, root)
    assert ctx.air_audit().ok
    ctx.close()


# ------------------------------------------------------------ stateless entry point, CLI
@pytest.mark.gpu
def test_stateless_entry_point_and_cli(gpu_ok, product, tmp_path):
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    clean = clean_trace(product)
    golden = golden_blocks(product)
    for blocks in (clean, golden):
        a = audit_of(product, blocks)
        assert as_dict(product.StarkV1.air_audit(blocks, bitmaps=True)) == as_dict(a)
        s = product.StarkV1.air_audit(blocks)
        assert s.violating_bits is None and s.families == a.families
    path = tmp_path / "clean.cbor"
    path.write_bytes(clean.to_cbor())
    for p, blocks, code in ((str(path), clean, 0), (os.path.join(GOLDEN, "ref_blocks.cbor"), golden, 3)):
        a = audit_of(product, blocks)
        r = subprocess.run([cli, "audit", "--blocks", p, "--json"], capture_output=True, text=True)
        assert r.returncode == code, r.stderr
        j = json.loads(r.stdout)
        none = lambda v: NO_ROW if v is None else v
        assert (j["n_rows"], j["tau"], j["ok"]) == (a.n_rows, a.tau, a.ok)
        for name in FAMS:
            got = dict(j["families"][name])
            got["first_row"] = none(got["first_row"])
            assert got == a.families[name], name
        assert (j["rows_violating"], none(j["first_violating"]), j["rows_rejectable"], none(j["first_rejectable"])) == \
            (a.rows_violating, a.first_violating, a.rows_rejectable, a.first_rejectable)
        assert j["verify_reject_probability"] == pytest.approx(a.verify_reject_probability(), rel=1e-12, abs=0)
        t = subprocess.run([cli, "audit", "--blocks", p], capture_output=True, text=True)
        assert t.returncode == code
        for name in FAMS:
            assert f"{name:<12} cells={a.families[name]['cells']} rows={a.families[name]['rows']}" in t.stdout
        assert f"violating rows:  {a.rows_violating}" in t.stdout
        assert f"rejectable rows: {a.rows_rejectable}" in t.stdout
