"""Proving from a raw trace on sharded contexts: P ranks share the one GPU and
exchange through `HostCollectives` (gloo), as tests/test_gpu_sharded.py does.
Each rank uploads the movement log (or only its rows), partitions the blocks
it reads on the device, and the ranks exchange the input-head offsets
(`trace_in_head`) and the manifest leaves (`manifest_leaves`) inside the first
proof. Yardsticks, none touched by this change: the numpy `partition`,
`BlockSoA.leaf_hashes()` / `manifest_root()` / `manifest_frontier_root()`,
`oracle.manifest_root` and `oracle_ctypes.prove_v1`.

Shapes (world, t, tau, b, moves):
  1 (2, 8192, 2, 512, random)   smallest legal shard, blocks aligned with the rank boundary
  2 (2, 8192, 3, 333, random)   a block straddles row 4096; 25 leaves (odd promotions)
  3 (2, 8192, 1, 8192, random)  one block: rank 1 owns nothing
  4 (2, 8192, 2, 5000, alt127)  two ragged blocks: rank 1 reads both, owns one
  5 (4, 16384, 3, 1, minus/plus) 4096 owned blocks per rank = four scan tiles, a tree of exactly
                                2^14 leaves, the rank prefix at -128 / +127 a row
  6 (8, 32768, 8, 512, random)  the headline's block shape at P = 8
"""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import ORACLE, PKG, free_port
from test_gpu_trace_upload import make_trace

pytestmark = pytest.mark.gpu

CASES = [
    (2, 8192, 2, 512, "random"),
    (2, 8192, 3, 333, "random"),
    (2, 8192, 1, 8192, "random"),
    (2, 8192, 2, 5000, "alt127"),
    (4, 16384, 3, 1, "minus"),
    (4, 16384, 3, 1, "plus"),
    (8, 32768, 8, 512, "random"),
]
FROM_BLOCKS_MSG = "manifest root from the trace: the active trace image was uploaded as blocks"
QUEUE_TIMEOUT = 300


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@functools.lru_cache(maxsize=None)
def want(t, tau, b, moves):
    """The yardsticks of one trace, computed once: (blocks, root, frontier root, leaves, proof digest)."""
    import oracle_ctypes
    import sezkp_amd
    blocks = sezkp_amd.partition(*make_trace(t, tau, b, moves), b)
    root = blocks.manifest_root()
    assert root == oracle_ctypes.manifest_root(blocks)
    return blocks, root, blocks.manifest_frontier_root(), blocks.leaf_hashes(), sha(oracle_ctypes.prove_v1(blocks, root))


def _err(e):
    return ("ERR", getattr(e, "code", None), f"{type(e).__name__}: {e}")


def _worker(rank, world, port, shape, mode, q):
    """One rank. mode: "whole" (upload_trace of the whole view), "rows" (only
    trace_shard_rows through upload_trace_rows), "short:<r>" (rank r's slice is
    one row short; nobody proves)."""
    sys.path[:0] = [PKG, ORACLE]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sezkp_amd
        t, tau, b, moves = shape
        tr = make_trace(t, tau, b, moves)
        ctx = sezkp_amd.ShardedProverContext(rank, world, device=0, comm="host")
        out = {"rank": rank}
        if mode == "whole":
            ctx.upload_trace(*tr, b)
        else:
            row0, nrows = sezkp_amd.trace_shard_rows(t, b, rank, world)
            if mode == f"short:{rank}":
                nrows -= 1
            try:
                ctx.upload_trace_rows(*(a[row0:row0 + nrows] for a in tr), b, t, row0)
                out["upload"] = ("ok", row0, nrows)
            except sezkp_amd.SezkpError as e:
                out["upload"] = _err(e)
        if mode.startswith("short"):
            calls = dict(ctx._coll.calls)
            out["collectives"] = sum(v for v in calls.values() if isinstance(v, int))
            ctx.close()
            q.put(out)
            return
        try:  # the reports need a completed proof; a report starts no collective
            ctx.manifest_root()
            out["early_root"] = ("ok", None, "")
        except sezkp_amd.SezkpError as e:
            out["early_root"] = _err(e)
        a1 = ctx.prove()
        out["stats1"] = ctx.comm_stats()
        a2 = ctx.prove()
        out["stats2"] = ctx.comm_stats()
        out.update(digest=sha(a1.proof_bytes), repeat=a1.proof_bytes == a2.proof_bytes, art_root=a1.manifest_root,
                   root=ctx.manifest_root(), frontier=ctx.manifest_root(frontier=True),
                   leaves=sha(ctx.manifest_leaves()), n_blocks=ctx.n_blocks)
        try:
            ctx.blocks()
            out["blocks"] = ("ok", None, "")
        except sezkp_amd.SezkpError as e:
            out["blocks"] = _err(e)
        ctx.close()
        q.put(out)
    except Exception as e:
        q.put({"rank": rank, "error": f"{type(e).__name__}: {e}"})
    finally:
        dist.destroy_process_group()


def _run(world, shape, mode):
    import torch.multiprocessing as mp
    assert world <= 8
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, shape, mode, q)) for r in range(world)]
    for p in ps:
        p.start()
    try:
        res = sorted((q.get(timeout=QUEUE_TIMEOUT) for _ in ps), key=lambda o: o["rank"])
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for o in res:
        assert "error" not in o, o
    return res


def _check_ranks(res, world, shape):
    t, tau, b, moves = shape
    blocks, root, frontier, leaves, digest = want(*shape)
    nblk = blocks.n_blocks
    for o in res:
        rank = o["rank"]
        assert o["digest"] == digest, f"rank {rank}: {o['digest']}"
        assert o["repeat"], rank
        assert o["art_root"] == root and o["root"] == root and o["frontier"] == frontier, rank
        assert o["leaves"] == sha(leaves) and o["n_blocks"] == nblk, rank
        assert o["early_root"][1] == -1 and "prove first" in o["early_root"][2], o["early_root"]
        assert o["blocks"][1] == -1 and "sharded" in o["blocks"][2], o["blocks"]
        # the first proof partitions: the two new collectives, in order, before the old ones
        names1 = [c["name"] for c in o["stats1"]]
        assert names1[:3] == ["trace_in_head", "manifest_leaves", "col_chunk_roots"], names1
        st1 = {c["name"]: c for c in o["stats1"]}
        assert st1["trace_in_head"]["bytes"] == (world - 1) * 8
        assert st1["manifest_leaves"]["bytes"] == 2 * (world - 1) * 32 * nblk // world
        assert st1["trace_in_head"]["ms"] >= 0 and st1["manifest_leaves"]["ms"] >= 0
        # later proofs of the image run neither, and are otherwise the same
        names2 = [c["name"] for c in o["stats2"]]
        assert names2 == names1[2:], (names1, names2)


@pytest.mark.parametrize("world,t,tau,b,moves", CASES)
def test_sharded_trace_matches_oracle(gpu_ok, product, oracle, world, t, tau, b, moves):
    shape = (t, tau, b, moves)
    owned = [product.trace_shard_blocks(t, b, r, world)["own_cnt"] for r in range(world)]
    assert sum(owned) == -(-t // b)
    if (t, b) == (8192, 8192):
        assert owned == [1, 0]
    if b == 1:
        assert owned == [4096] * 4  # four scan tiles per rank
    _check_ranks(_run(world, shape, "whole"), world, shape)


def test_sharded_trace_row_slices(gpu_ok, product, oracle):
    """Case 2 with each rank uploading only the rows it reads."""
    world, shape = 2, (8192, 3, 333, "random")
    res = _run(world, shape, "rows")
    for o in res:
        row0, nrows = product.trace_shard_rows(8192, 333, o["rank"], world)
        assert o["upload"] == ("ok", row0, nrows) and nrows < 8192
    _check_ranks(res, world, shape)


def test_sharded_trace_short_slice_is_refused_on_that_rank_alone(gpu_ok, product):
    world, shape = 2, (8192, 3, 333, "random")
    res = _run(world, shape, "short:1")
    row0, nrows = product.trace_shard_rows(8192, 333, 1, world)
    assert res[0]["upload"][0] == "ok"
    kind, code, msg = res[1]["upload"]
    assert (kind, code) == ("ERR", -1), res[1]
    assert f"step arrays hold rows [{row0}, {row0 + nrows - 1}) but this context needs rows [{row0}, {row0 + nrows})" \
        in msg, msg
    assert all(o["collectives"] == 0 for o in res)  # no upload performs a collective


# ------------------------------------------------------------ one rank
def _single_gpu_bytes(product, shape):
    t, tau, b, moves = shape
    c = product.ProverContext(0)
    try:
        c.upload_trace(*make_trace(*shape), b)
        return c.prove()
    finally:
        c.close()


@pytest.mark.parametrize("force", [False, True])
def test_world1_is_the_single_gpu_trace_path(gpu_ok, product, oracle, monkeypatch, force):
    """world = 1: the single-device schedule, or with SEZKP_FORCE_SHARDED the
    sharded algorithm over a one-rank RCCL communicator (every collective of
    the first proof runs on the device, the two new ones included)."""
    if force:
        monkeypatch.setenv("SEZKP_FORCE_SHARDED", "1")
    shape = (4096, 3, 333, "random")
    single = _single_gpu_bytes(product, shape)
    blocks, root, frontier, leaves, digest = want(*shape)
    assert sha(single.proof_bytes) == digest and single.manifest_root == root
    c = product.ShardedProverContext(0, 1, device=0, comm="rccl")
    try:
        c.upload_trace(*make_trace(*shape), 333)
        art = c.prove()
        names = [s["name"] for s in c.comm_stats()]
        assert names[:2] == (["trace_in_head", "manifest_leaves"] if force else []), names
        assert (art.proof_bytes, art.manifest_root) == (single.proof_bytes, root)
        assert c.prove().proof_bytes == single.proof_bytes
        assert "trace_in_head" not in [s["name"] for s in c.comm_stats()]
        assert c.manifest_root() == root and c.manifest_root(frontier=True) == frontier
        assert c.manifest_leaves() == leaves
        # a given root is used as given
        other = bytes(range(32))
        assert sha(c.prove(other).proof_bytes) == sha(oracle.prove_v1(blocks, other))
        # row slices on one rank: the whole trace or nothing
        tr = make_trace(*shape)
        with pytest.raises(product.SezkpError, match=r"needs rows \[0, 4096\)") as e:
            c.upload_trace_rows(*(a[:4095] for a in tr), 333, 4096, 0)
        assert e.value.code == -1
        c.upload_trace_rows(*tr, 333, 4096, 0)
        assert c.prove().proof_bytes == single.proof_bytes
        # the step arrays as device tensors; the borrowed and the asynchronous proof, without a root
        torch = gpu_ok
        dev = [torch.from_numpy(np.array(a)).cuda() for a in (tr[0], tr[1], tr[2], tr[3].view(np.int16))]
        c.upload_trace_rows(*dev, 333, 4096, 0)
        assert bytes(c.prove_view()) == single.proof_bytes  # the first proof of this image
        c.prove_async()
        assert bytes(c.wait_view()) == single.proof_bytes
        assert c.manifest_root() == root
    finally:
        c.close()


@pytest.mark.parametrize("rank", [0, 1])
def test_rank_alone_at_p2_measures_its_own_part(gpu_ok, product, rank):
    """A rank of 2 alone (sezkp_ctx_create_sharded_solo) takes a trace like any
    sharded context: the proof runs with the rank's own blocks (bytes
    meaningless), and the collectives report what they would put on the
    links. (A rank-alone context of ONE rank stands for no rank of a sharded
    proof and keeps its refusal: tests/test_gpu_trace_upload.py pins it.)"""
    t, tau, b = 8192, 2, 512
    tr = make_trace(t, tau, b, "random")
    c = product.ShardedProverContext(rank, 2, 0, comm="solo")
    try:
        c.upload_trace(*tr, b)
        assert len(c.prove().proof_bytes) > 0
        st = {s["name"]: s for s in c.comm_stats()}
        assert st["trace_in_head"]["bytes"] == 8 and st["manifest_leaves"]["bytes"] == 32 * 16
        c.prove()
        assert "manifest_leaves" not in [s["name"] for s in c.comm_stats()]
        # the rank's slice goes through upload_trace_rows as well
        row0, nrows = product.trace_shard_rows(t, b, rank, 2)
        c.upload_trace_rows(*(a[row0:row0 + nrows] for a in tr), b, t, row0)
        c.prove()
        assert [s["name"] for s in c.comm_stats()][:2] == ["trace_in_head", "manifest_leaves"]
    finally:
        c.close()


# ------------------------------------------------------------ reports and refusals
def test_reports_and_refusals_before_the_first_proof(gpu_ok, product):
    t, tau, b = 8192, 2, 512
    tr = make_trace(t, tau, b, "random")
    c = product.ShardedProverContext(0, 2, 0, comm="solo")
    try:
        c.upload_trace(*tr, b)
        for call in (c.manifest_root, c.manifest_leaves, lambda: c.manifest_root(frontier=True)):
            with pytest.raises(product.SezkpError, match="prove first") as e:
                call()
            assert e.value.code == -1
        with pytest.raises(product.SezkpError, match="sharded") as e:
            c.blocks()
        assert e.value.code == -1
        with pytest.raises(product.SezkpError, match="sharded") as e:
            c.stage_trace(*tr, b)
        assert e.value.code == -1
        # 41 tapes: refused at upload, naming the limit
        with pytest.raises(product.SezkpError, match="at most 40 tapes") as e:
            c.upload_trace(*make_trace(8192, 41, 512, "random"), 512)
        assert e.value.code == -1
        # too few rows for two ranks: the planner's message, as for blocks
        with pytest.raises(product.SezkpError, match=r"n >= 4096 \* P") as e:
            c.upload_trace(*make_trace(4096, 2, 512, "random"), 512)
        assert e.value.code == -1
        # the refusals left the uploaded image alone
        with pytest.raises(product.SezkpError, match="prove first"):
            c.manifest_root()
        # an image uploaded as blocks keeps its error
        c.upload(product.partition(*tr, b))
        for call in (c.prove, c.prove_view, c.prove_async):
            with pytest.raises(product.SezkpError) as e:
                call()
            assert e.value.code == -1 and FROM_BLOCKS_MSG in str(e.value)
        with pytest.raises(product.SezkpError, match="uploaded as blocks"):
            c.manifest_root()
    finally:
        c.close()


# ------------------------------------------------------------ launcher
def test_launcher_proves_from_a_trace_file(gpu_ok, product, oracle, tmp_path):
    import subprocess

    import cbor_min
    t, tau, b = 8192, 3, 333
    shape = (t, tau, b, "random")
    blocks, root, _, _, digest = want(*shape)
    (tmp_path / "t.cbor").write_bytes(product.Trace(*make_trace(*shape)).to_cbor())
    (tmp_path / "b.cbor").write_bytes(blocks.to_cbor())
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    r = subprocess.run([cli, "commit", "--blocks", str(tmp_path / "b.cbor"), "--out", str(tmp_path / "want.cbor")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    cmd = [sys.executable, "-m", "sezkp_amd.launch", "prove", "--trace", str(tmp_path / "t.cbor"), "--b", str(b),
           "--out", str(tmp_path / "p.cbor"), "--out-manifest", str(tmp_path / "m.cbor"), "--manifest",
           str(tmp_path / "want.cbor"), "--gpus", "2", "--comm", "host", "--timeout", "300"]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    art = cbor_min.loads((tmp_path / "p.cbor").read_bytes())
    assert art["backend"] == "stark" and bytes(art["manifest_root"]) == root
    assert sha(bytes(art["proof_bytes"])) == digest
    assert art["meta"] == {"proto": "stark-v1", "domain_n": 8 * t, "tau": tau}
    assert (tmp_path / "m.cbor").read_bytes() == (tmp_path / "want.cbor").read_bytes()
    # a manifest of another root: non-zero exit, nothing written
    (tmp_path / "bad.cbor").write_bytes(cbor_min.dumps({"root": [7] * 32, "n_leaves": blocks.n_blocks}))
    bad = cmd[:]
    bad[bad.index(str(tmp_path / "want.cbor"))] = str(tmp_path / "bad.cbor")
    bad[bad.index(str(tmp_path / "p.cbor"))] = str(tmp_path / "p2.cbor")
    bad[bad.index(str(tmp_path / "m.cbor"))] = str(tmp_path / "m2.cbor")
    r = subprocess.run(bad, cwd=PKG, capture_output=True, text=True, timeout=400)
    assert r.returncode != 0 and "manifest root mismatch" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "p2.cbor").exists() and not (tmp_path / "m2.cbor").exists()
