"""A raw trace on sharded contexts, the host plan (CPU only, no device call):
sezkp_trace_shard_rows / sezkp_trace_shard_blocks (csrc/trace_plan.h) against
sezkp_shard_rows on the explicit uniform block boundaries.

Ownership: rank g owns block k exactly when the block's first row lies in the
rank's own rows [g n/P, (g + 1) n/P). Every block has one owner, the owner
reads the whole block, and a rank may own none."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

TS = [1 << v for v in range(12, 17)]
WORLDS = [1, 2, 4, 8]


def bs_of(t):
    return [1, 7, 100, 333, 512, 1024, 5000, t]


GRID = [(t, b, w) for t in TS for b in bs_of(t) for w in WORLDS if t >= 4096 * w]


def uniform_step_start(t, b):
    nblk = -(-t // b)
    return np.minimum(np.arange(nblk + 1, dtype=np.uint64) * np.uint64(b), np.uint64(t))


def shard_rows(lib, ss, rank, world):
    row0, nrows = C.c_uint64(), C.c_uint64()
    rc = lib.sezkp_shard_rows(ss.ctypes.data, len(ss) - 1, rank, world, C.byref(row0), C.byref(nrows))
    assert rc == 0
    return row0.value, nrows.value


def test_symbols_exported_and_declared(product):
    lib = C.CDLL(product.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "sezkp_stark.h")).read()
    for s in ("sezkp_trace_shard_rows", "sezkp_trace_shard_blocks", "sezkp_ctx_upload_trace_rows"):
        assert hasattr(lib, s) and s in product._lib.EXPORTS and s + "(" in hdr, s
    assert lib.sezkp_abi_version() == 4
    assert "sezkp_shard_rows" in hdr.split("int32_t sezkp_trace_shard_rows(")[0][-400:]


@pytest.mark.parametrize("t,b,world", GRID)
def test_trace_shard_rows_equals_shard_rows(product, t, b, world):
    ss = uniform_step_start(t, b)
    for rank in range(world):
        assert product.trace_shard_rows(t, b, rank, world) == shard_rows(product.lib, ss, rank, world), rank


@pytest.mark.parametrize("t,b,world", GRID)
def test_trace_shard_blocks_ownership(product, t, b, world):
    ss = uniform_step_start(t, b)
    nblk = len(ss) - 1
    nxt = 0
    for rank in range(world):
        s = product.trace_shard_blocks(t, b, rank, world)
        # owned ranges: disjoint, in rank order, covering [0, nblk) exactly
        if s["own_cnt"]:
            assert s["own_lo"] == nxt, (rank, s)
            nxt = s["own_lo"] + s["own_cnt"]
            # inside the read range
            assert s["blk_lo"] <= s["own_lo"] and nxt <= s["blk_lo"] + s["blk_cnt"], (rank, s)
        # ownership as defined: the blocks whose first row lies in the rank's own rows
        lo, hi = rank * (t // world), (rank + 1) * (t // world)
        first, last = ss[:-1].astype(np.int64), ss[1:].astype(np.int64)
        own = np.flatnonzero((first >= lo) & (first < hi))
        assert s["own_cnt"] == len(own) and (len(own) == 0 or s["own_lo"] == own[0]), (rank, s)
        assert len(own) == 0 or own[-1] - own[0] + 1 == len(own)
        # the read range: the blocks overlapping the rows of sezkp_shard_rows
        row0, nrows = shard_rows(product.lib, ss, rank, world)
        over = np.flatnonzero((first < row0 + nrows) & (last > row0))
        assert (s["blk_lo"], s["blk_cnt"]) == (over[0], len(over)), (rank, s)
        assert int(ss[s["blk_lo"]]) == row0 and int(ss[s["blk_lo"] + s["blk_cnt"]]) == row0 + nrows
    assert nxt == nblk


def test_a_rank_may_own_nothing(product):
    assert product.trace_shard_blocks(8192, 8192, 0, 2) == {"blk_lo": 0, "blk_cnt": 1, "own_lo": 0, "own_cnt": 1}
    s = product.trace_shard_blocks(8192, 8192, 1, 2)
    assert (s["blk_lo"], s["blk_cnt"], s["own_cnt"]) == (0, 1, 0)
    assert product.trace_shard_rows(8192, 8192, 1, 2) == (0, 8192)


@pytest.mark.parametrize("t,b,rank,world", [
    (8192, 0, 0, 2),       # b = 0
    (8192 + 1, 512, 0, 2),  # t no power of two
    (3000, 512, 0, 1),
    (0, 512, 0, 1),
    (8192, 512, 0, 3),     # world not in {1, 2, 4, 8}
    (1 << 16, 512, 0, 16),
    (8192, 512, 0, 0),
    (8192, 512, 2, 2),     # rank out of range
    (8192, 512, -1, 2),
    (4096, 512, 0, 2),     # t < 4096 * world
    (1 << 14, 512, 0, 8),
])
def test_errors(product, t, b, rank, world):
    lib = product.lib
    r0, nr = C.c_uint64(7), C.c_uint64(7)
    w = [C.c_uint32(7) for _ in range(4)]
    assert lib.sezkp_trace_shard_rows(t, b, rank, world, C.byref(r0), C.byref(nr)) == product._lib.SEZKP_E_INVALID
    assert lib.sezkp_trace_shard_blocks(t, b, rank, world, *[C.byref(x) for x in w]) == product._lib.SEZKP_E_INVALID
    assert (r0.value, nr.value) == (7, 7) and all(x.value == 7 for x in w)  # nothing written
    with pytest.raises(product.SezkpError):
        product.trace_shard_rows(t, b, rank, world)
    with pytest.raises(product.SezkpError):
        product.trace_shard_blocks(t, b, rank, world)


def test_null_outputs(product):
    lib = product.lib
    x = C.c_uint64()
    assert lib.sezkp_trace_shard_rows(8192, 512, 0, 2, None, C.byref(x)) == product._lib.SEZKP_E_INVALID
    assert lib.sezkp_trace_shard_rows(8192, 512, 0, 2, C.byref(x), None) == product._lib.SEZKP_E_INVALID
    w = [C.c_uint32() for _ in range(4)]
    for i in range(4):
        args = [C.byref(y) for y in w]
        args[i] = None
        assert lib.sezkp_trace_shard_blocks(8192, 512, 0, 2, *args) == product._lib.SEZKP_E_INVALID


def test_launcher_trace_usage_and_manifest_file(product, tmp_path, capsys):
    """`launch prove --trace`: usage errors before any process is started, and
    the manifest it writes is the file `sezkp-cli commit` writes."""
    import subprocess

    from conftest import PKG
    from sezkp_amd import launch
    out = str(tmp_path / "p.cbor")
    assert launch.main(["prove", "--trace", "t.cbor", "--out", out]) == 2                     # no --b
    assert launch.main(["prove", "--trace", "t.cbor", "--b", "0", "--out", out]) == 2
    assert launch.main(["prove", "--trace", "t.cbor", "--b", "4", "--blocks", "b.cbor", "--out", out]) == 2
    assert launch.main(["prove", "--trace", "t.cbor", "--b", "4", "--out-manifest", "m.json", "--out", out]) == 2
    assert launch.main(["prove", "--out", out]) == 2                                          # neither input
    assert launch.main(["prove", "--blocks", "b.cbor", "--out", out]) == 2                    # no --manifest
    capsys.readouterr()
    blocks = product.partition(*product.simulate(64, 2, 3), 8)
    (tmp_path / "b.cbor").write_bytes(blocks.to_cbor())
    r = subprocess.run([os.path.join(PKG, "bin", "sezkp-cli"), "commit", "--blocks", str(tmp_path / "b.cbor"), "--out",
                        str(tmp_path / "m.cbor")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    mine = launch._manifest_cbor(blocks.manifest_root(), blocks.n_blocks)
    assert mine == (tmp_path / "m.cbor").read_bytes()
    (tmp_path / "mine.cbor").write_bytes(mine)
    assert launch._read_manifest(str(tmp_path / "mine.cbor")) == (blocks.manifest_root(), blocks.n_blocks)


def test_trace_view_of_a_row_slice(product):
    tr = product.simulate(64, 2, 3)
    v, keep = product.trace.trace_view(*(a[8:24] for a in tr), b=8, t=64)
    assert (v.t, v.tau, v.b, len(keep[0])) == (64, 2, 8, 16)
    with pytest.raises(product.SezkpError):
        product.trace.trace_view(*(a[8:24] for a in tr), b=8, t=15)  # fewer steps than rows held


def test_world1_small_traces(product):
    """One rank reads and owns everything, also below one chunk of rows."""
    for t, b in ((1, 1), (32, 4), (512, 100), (1024, 1024), (2048, 7)):
        nblk = -(-t // b)
        assert product.trace_shard_rows(t, b, 0, 1) == (0, t)
        assert product.trace_shard_blocks(t, b, 0, 1) == {"blk_lo": 0, "blk_cnt": nblk, "own_lo": 0, "own_cnt": nblk}
