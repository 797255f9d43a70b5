"""GPU parity of the piecewise columns' U tables keyed by value (col_commit.hip,
k_col_tables / pw_unit).

A per-block column (win_len, in_off, out_off) whose signed range over the
device's blocks holds fewer values than the device has blocks builds one table
unit per value (unit v - lo) instead of one per block; a wider range keeps one
unit per block. The device decides per column and per proof, so both forms
and the changes between them are reached through the traces alone. Every
proof must equal the oracle's bytes, and `pw_table_stats()` (the form words
the device sends home with the column roots) must name the forms and the
units that the traces' own ranges give (`_want_stats`).

tau = 2. With blocks of b steps a tape's offsets lie in [0, b] and its window
length in [1, b + 1]:
  generator traces, T = 2^12: b = 64 (64 blocks, offsets of a 64-step walk:
    fewer values than blocks, by value) and b = 512 (8 blocks: by block);
  all moves +1, then all -1 (T = 2^13, b = 64, 128 blocks): offsets {0, 64},
    window length 65: ranges of 65 values with two of them used, and of one;
  all moves 0: every range is one value;
  one block wider than the rest (T = 2^12, b = 64): moves 0 but for one
    block of +1 / -1: ranges of 65 values against 64 blocks (by block) beside
    ranges of one value (by value) in the same proof.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import ORACLE, PKG, free_port

pytestmark = pytest.mark.gpu

TAU = 2


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("SEZKP_PW_BY_VALUE", "SEZKP_DEBUG_TRIP_GUARD", "SEZKP_FORCE_SHARDED"):
        monkeypatch.delenv(k, raising=False)


def _partition(product, mv, b, seed):
    t = mv.shape[0]
    rng = np.random.default_rng(seed)
    imv = rng.integers(-1, 2, t).astype(np.int8)
    hw = (rng.random((t, TAU)) < 0.4).astype(np.uint8)
    ws = (rng.integers(0, 16, (t, TAU)) * hw).astype(np.uint16)
    return product.partition(imv, mv.astype(np.int8), hw, ws, b)


def _up_down(product):
    t, b = 1 << 13, 64
    mv = np.ones((t, TAU), np.int64)
    mv[t // 2:] = -1
    mv[:, 1] = -mv[:, 1]  # the second tape the other way round
    return _partition(product, mv, b, 1)


def _still(product):
    return _partition(product, np.zeros((1 << 12, TAU), np.int64), 64, 2)


def _one_wide(product):
    t, b = 1 << 12, 64
    mv = np.zeros((t, TAU), np.int64)
    mv[5 * b:6 * b, 0] = 1
    mv[5 * b:6 * b, 1] = -1
    return _partition(product, mv, b, 3)


BUILDERS = {
    "gen_b64": lambda p: p.reference_blocks(1 << 12, 64, TAU, 42),
    "gen_b512": lambda p: p.reference_blocks(1 << 12, 512, TAU, 42),
    "up_down": _up_down,
    "still": _still,
    "one_wide": _one_wide,
    "gen13_b64": lambda p: p.reference_blocks(1 << 13, 64, TAU, 43),
}
_cases = {}


def _case(product, oracle, name):
    """(blocks, manifest root, the oracle's proof), computed once per trace."""
    if name not in _cases:
        blocks = BUILDERS[name](product)
        root = blocks.manifest_root()
        _cases[name] = (blocks, root, oracle.prove_v1(blocks, root))
    return _cases[name]


def _spans(blocks, lo=0, hi=None):
    """Per per-block column the number of values in its range over blocks
    [lo, hi), and the number of those blocks."""
    nb = blocks.n_blocks
    hi = nb if hi is None else hi
    wl = (blocks.win_right.astype(np.int64) - blocks.win_left.astype(np.int64) + 1).reshape(nb, TAU)
    cols = [wl, blocks.off_in.astype(np.int64).reshape(nb, TAU), blocks.off_out.astype(np.int64).reshape(nb, TAU)]
    return [int(c[lo:hi, r].max() - c[lo:hi, r].min()) + 1 for c in cols for r in range(TAU)], hi - lo


def _want_stats(blocks, lo=0, hi=None, by_value=True):
    """What the device must report for a device holding blocks [lo, hi): a
    column is keyed by value when its range has no more values than the device
    has blocks, and then builds one unit per value of the range."""
    spans, cnt = _spans(blocks, lo, hi)
    mine = [s for s in spans if by_value and s <= cnt]
    return {"cols_by_value": len(mine), "cols_by_block": len(spans) - len(mine), "units_built": sum(mine)}


def test_traces_reach_both_forms(product):
    """The designed ranges: which form each trace's columns take."""
    by_value = {}
    for name in list(BUILDERS)[:5]:
        spans, nb = _spans(BUILDERS[name](product))
        by_value[name] = [s <= nb for s in spans]
    assert all(by_value["gen_b64"]) and not any(by_value["gen_b512"])
    assert all(by_value["up_down"]) and all(by_value["still"])
    # 65 values against 64 blocks where the wide block's tape moves, one value elsewhere: both forms in one proof
    assert by_value["one_wide"] == [False, False, True, False, False, True]
    assert _spans(BUILDERS["still"](product))[0] == [1] * 6
    assert max(_spans(BUILDERS["up_down"](product))[0]) == 65


@pytest.mark.parametrize("by_value", [True, False])
@pytest.mark.parametrize("name", list(BUILDERS))
def test_prove_matches_oracle(gpu_ok, product, oracle, monkeypatch, name, by_value):
    """Default, and SEZKP_PW_BY_VALUE=0 (read per proof: one unit per block
    for every column, the earlier tables): the oracle's bytes."""
    if not by_value:
        monkeypatch.setenv("SEZKP_PW_BY_VALUE", "0")
    blocks, root, want = _case(product, oracle, name)
    ctx = product.ProverContext(0)
    try:
        ctx.upload(blocks)
        assert ctx.pw_table_stats() == {"cols_by_value": 0, "cols_by_block": 0, "units_built": 0}
        assert ctx.prove(root).proof_bytes == want
        assert ctx.pw_table_stats() == _want_stats(blocks, by_value=by_value)
    finally:
        ctx.close()


def test_forms_alternate_on_one_context(gpu_ok, product, oracle):
    """By value, by block, by value with another range, and the first again,
    staged on one context (T = 2^12 throughout): the range and the form are
    taken anew by every proof, nothing of the last one is read."""
    ctx = product.ProverContext(0)
    try:
        first = True
        for name in ("gen_b64", "one_wide", "still", "gen_b64"):
            blocks, root, want = _case(product, oracle, name)
            if first:
                ctx.upload(blocks)
                first = False
            else:
                ctx.stage(blocks)
            assert ctx.prove(root).proof_bytes == want, name
            assert ctx.pw_table_stats() == _want_stats(blocks), name
        blocks, root, want = _case(product, oracle, "gen_b512")
        ctx.upload(blocks)
        assert ctx.prove(root).proof_bytes == want
        assert ctx.pw_table_stats() == _want_stats(blocks)
    finally:
        ctx.close()


def test_refused_proof_in_between(gpu_ok, product, oracle, monkeypatch):
    """Good, refused, good on one context. SEZKP_DEBUG_TRIP_GUARD=0 (read per
    prove) sets the guard word behind the column commitment, so the proof is
    refused without a fault after its tables were built, and the context stays
    usable (SEZKP_DEBUG_FAIL_AT is read once per process and leaves a context
    unusable, so it cannot be followed by a good proof). The next trace has
    other ranges: its tables and forms are its own."""
    ctx = product.ProverContext(0)
    try:
        blocks, root, want = _case(product, oracle, "gen_b64")
        ctx.upload(blocks)
        assert ctx.prove(root).proof_bytes == want
        monkeypatch.setenv("SEZKP_DEBUG_TRIP_GUARD", "0")
        with pytest.raises(product.SezkpError):
            ctx.prove(root)
        monkeypatch.delenv("SEZKP_DEBUG_TRIP_GUARD")
        for name in ("one_wide", "gen_b64"):
            blocks, root, want = _case(product, oracle, name)
            ctx.stage(blocks)
            assert ctx.prove(root).proof_bytes == want, name
            assert ctx.pw_table_stats() == _want_stats(blocks), name
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["gen_b64", "gen_b512", "up_down"])
def test_forced_sharded_path(gpu_ok, product, oracle, monkeypatch, name):
    """SEZKP_FORCE_SHARDED=1: the sharded code path on one rank (its block
    range comes from the rank's rows)."""
    monkeypatch.setenv("SEZKP_FORCE_SHARDED", "1")
    blocks, root, want = _case(product, oracle, name)
    ctx = product.ProverContext(0)
    try:
        ctx.upload(blocks)
        assert ctx.prove(root).proof_bytes == want
        assert ctx.pw_table_stats() == _want_stats(blocks)
    finally:
        ctx.close()


SHARDED = ("gen13_b64", "up_down")


def _sharded_worker(rank, world, port, q):
    sys.path[:0] = [PKG, ORACLE, os.path.dirname(os.path.abspath(__file__))]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sezkp_amd
        ctx = sezkp_amd.ShardedProverContext(rank, world, device=0, comm="host")
        out = []
        for name in SHARDED:
            blocks = BUILDERS[name](sezkp_amd)
            ctx.upload(blocks)
            proof = ctx.prove(blocks.manifest_root()).proof_bytes
            out.append((hashlib.sha256(proof).hexdigest(), ctx.pw_table_stats()))
        ctx.close()
        q.put((rank, out))
    except Exception as e:
        q.put((rank, f"ERR {type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


def test_sharded_p2_host_collectives(gpu_ok, product, oracle):
    """P = 2 over host collectives (two ranks sharing the GPU), T = 2^13,
    b = 64. A rank holds the blocks that overlap its rows and the row after
    them (`shard_rows`: rank 0 blocks 0..64, rank 1 blocks 64..127, blk_lo =
    64), so rank 1's range is taken from block 64 on while its readers index
    the block values by the global block number. Each rank's ranges are its
    own blocks' (in `up_down` the two halves hold different values: rank 1
    sees one value per column, rank 0 both through block 64), every rank
    returns the oracle's bytes, and the form words are those of the rank's
    blocks."""
    import torch.multiprocessing as mp
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
        for name, (digest, stats) in zip(SHARDED, out):
            blocks, _, want = _case(product, oracle, name)
            assert blocks.n_blocks == 128
            assert digest == hashlib.sha256(want).hexdigest(), (rank, name)
            from sezkp_amd.blocks import shard_rows
            row0, nrows = shard_rows(blocks.step_start, rank, 2)
            lo, hi = row0 // 64, (row0 + nrows) // 64
            assert (lo > 0) == (rank == 1) and hi - lo < 128
            assert stats == _want_stats(blocks, lo, hi), (rank, name, lo, hi)
            assert stats["cols_by_value"] == 6, (rank, name)
