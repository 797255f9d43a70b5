"""Block files and TraceFiles written as CBOR on the device
(sezkp_ctx_encode_trace_blocks_cbor, sezkp_ctx_encode_blocks_cbor,
sezkp_ctx_encode_trace_cbor): byte for byte the host encoders' files.

Yardsticks, none touched by this change: `BlockSoA.to_cbor()`
(sezkp_blocks_encode_cbor) and `Trace.to_cbor()` (sezkp_trace_encode_cbor),
which the reference fixtures pin (tests/test_host_abi.py,
tests/test_trace_upload_host.py), and the fixtures themselves. The views are
those of tests/cbor_encode_corpus.py; tests/test_cbor_encode_host.py runs the
same views through the shared header on the CPU under the sanitizers.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cbor_encode_corpus as K
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
CLI = os.path.join(PKG, "bin", "sezkp-cli")


def golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


@pytest.fixture(scope="module")
def ctx(gpu_ok, product):
    c = product.ProverContext(0)
    yield c
    c.close()


def on_device(ctx, kind):
    st = ctx.encode_stats()
    assert (st["path"], st["reason"]) == ("device", "none") and st["ms_host"] == 0.0, (kind, st)
    return st


def check_view(product, ctx, name, v):
    blocks = K.to_blocks(product, v)
    want = blocks.to_cbor()
    got = ctx.encode_blocks_cbor(blocks)
    assert len(got) == len(want), (name, len(got), len(want))
    assert got == want, (name, next(i for i in range(len(want)) if got[i] != want[i]))
    st = on_device(ctx, name)
    assert (st["bytes"], st["n_blocks"], st["tau"], st["t"]) == (len(want), blocks.n_blocks, blocks.tau,
                                                                  int(blocks.step_start[-1])), (name, st)


# ------------------------------------------------------------ the fixtures
def test_golden_block_files_round_trip(ctx, product):
    for f in ("ref_blocks.cbor", "riscv_blocks.cbor"):
        raw = golden(f)
        assert ctx.encode_blocks_cbor(product.BlockSoA.from_cbor(raw)) == raw, f
        on_device(ctx, f)


def test_golden_trace_file_round_trips_and_partitions_into_the_golden_blocks(ctx, product):
    raw = golden("riscv_trace.cbor")
    assert ctx.trace_cbor(product.Trace.from_cbor(raw)) == raw
    on_device(ctx, "trace")
    ctx.upload_trace_cbor(raw, b=4)
    assert ctx.blocks_cbor() == golden("riscv_blocks.cbor")
    st = on_device(ctx, "image")
    assert (st["n_blocks"], st["tau"]) == (ctx.n_blocks, ctx.tau)
    assert ctx.trace_cbor() == raw  # the image's own TraceFile
    on_device(ctx, "image trace")


# ------------------------------------------------------------ the corpus
CASES = K.block_views()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_block_view_is_written_as_the_host_encoder_writes_it(ctx, product, name):
    check_view(product, ctx, name, dict(CASES)[name])


def test_the_corpus_covers_what_it_must():
    names = [n for n, _ in CASES]
    for tau in K.TAUS:
        assert f"tau{tau}" in names
    for tau in range(1, 256):  # both sides of every change of the steps per tile
        if K.tile_steps(tau) != K.tile_steps(tau - 1):
            assert tau in K.TAUS and tau - 1 in K.TAUS, tau
    w = K.widths_view()
    for ws in K.WSYM:
        for hw in (0, 1):
            assert ((w["wsym"] == ws) & (w["has_write"] == hw)).any(), (ws, hw)
    for m in K.MOVES:
        assert (w["mv"] == m).any() and (w["input_mv"] == m).any(), m
    h = K.heads_view()
    for f in ("in_head_in", "in_head_out", "win_left", "win_right"):
        assert set(K.I64) <= set(int(x) for x in h[f]), f
    for f in ("step_lo", "step_hi"):
        assert set(K.U64) <= set(int(x) for x in h[f]), f
    e = dict(CASES)["empties"]["step_start"]
    n = np.diff(e.astype(np.int64))
    assert n[0] == 0 and n[-1] == 0 and (n[1:-1] == 0).any() and set(n) >= {0, 1, 23, 24, 255, 256, 257}


def test_more_tiles_than_one_pass_of_the_scan(ctx, product):
    v = K.scan_pass_view()
    assert -(-int(v["step_start"][-1]) // K.tile_steps(1)) > 1024
    check_view(product, ctx, "scan_pass", v)


@pytest.mark.parametrize("name", [n for n, _, _ in K.trace_cases()])
def test_trace_is_written_as_the_host_encoder_writes_it(ctx, product, name):
    s, tau = {n: (s, tau) for n, s, tau in K.trace_cases()}[name]
    tr = product.Trace(s["input_mv"], s["mv"], s["has_write"], s["wsym"])
    want = tr.to_cbor()
    assert ctx.trace_cbor(tr) == want
    st = on_device(ctx, name)
    assert (st["bytes"], st["t"], st["tau"], st["n_blocks"]) == (len(want), tr.t, tau, 0)


@pytest.mark.parametrize("t,b,tau", [(4096, 512, 8), (4096, 8, 2), (256, 1, 2), (512, 1024, 3), (1024, 200, 1)])
def test_image_of_a_partitioned_trace(gpu_ok, product, t, b, tau):
    tr = product.simulate(t, tau, 7)
    c = product.ProverContext(0)
    try:
        c.upload_trace(*tr, b)
        want = c.blocks().to_cbor()
        assert c.blocks_cbor() == want == product.partition(*tr, b).to_cbor()
        on_device(c, "image")
        assert c.trace_cbor() == product.Trace(*tr).to_cbor()
    finally:
        c.close()


# ------------------------------------------------------------ device inputs
def test_torch_tensors_on_the_gpu_give_the_bytes_of_their_host_copies(ctx, product, gpu_ok):
    torch = gpu_ok
    v = K.view([255, 1, 1, 254, 2, 100], 8, seed=31)
    blocks = K.to_blocks(product, v)
    host = (v["input_mv"], v["mv"], v["has_write"], v["wsym"])
    dev = tuple(torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to("cuda:0").contiguous() for a in host)
    want = blocks.to_cbor()
    assert ctx.encode_blocks_cbor(blocks, steps=dev) == want
    on_device(ctx, "device steps")
    assert ctx.encode_blocks_cbor(blocks.meta_only(), steps=dev) == want
    # some arrays on the device, some on the host
    assert ctx.encode_blocks_cbor(blocks, steps=(dev[0], host[1], dev[2], host[3])) == want
    tw = product.Trace(*host).to_cbor()
    assert ctx.trace_cbor(dev) == tw and ctx.trace_cbor(host) == tw
    on_device(ctx, "device trace")


# ------------------------------------------------------------ state
def test_an_encode_leaves_proofs_and_a_pending_ingest_alone(gpu_ok, product, monkeypatch):
    t, tau, b = 4096, 2, 512
    tr = product.simulate(t, tau, 3)
    other = K.to_blocks(product, K.view([3, 0, 70], 2, seed=41))
    c = product.ProverContext(0)
    try:
        c.upload_trace(*tr, b)
        before = c.prove().proof_bytes
        assert c.prove().proof_bytes == before
        repeat = c.dict_cache_stats()  # of a proof that follows a proof
        files = {}
        for kind, call in (("image", c.blocks_cbor), ("view", lambda: c.encode_blocks_cbor(other)),
                           ("image trace", c.trace_cbor), ("trace", lambda: c.trace_cbor(product.Trace(*tr)))):
            files[kind] = call()
            on_device(c, kind)
            assert c.prove().proof_bytes == before, kind
            assert c.dict_cache_stats() == repeat, kind  # no table rebuilt because of an encode
        # the host path: the same bytes, reported as such; read per call
        monkeypatch.setenv("SEZKP_CBOR_ENCODE_HOST", "1")
        for kind, call in (("image", c.blocks_cbor), ("view", lambda: c.encode_blocks_cbor(other)),
                           ("image trace", c.trace_cbor), ("trace", lambda: c.trace_cbor(product.Trace(*tr)))):
            assert call() == files[kind], kind
            st = c.encode_stats()
            assert (st["path"], st["reason"]) == ("host", "forced") and st["ms_host"] > 0 and st["ms_kernels"] == 0, st
            assert st["bytes"] == len(files[kind])
        monkeypatch.setenv("SEZKP_CBOR_ENCODE_HOST", "0")
        assert c.blocks_cbor() == files["image"]
        on_device(c, "image again")
        # a pending ingest survives every kind of encode
        blocks = product.partition(*tr, b)
        root = blocks.manifest_root()
        c.ingest_blocks_cbor(blocks.to_cbor())
        assert c.blocks_ingest_stats()["path"] == "device"
        assert c.blocks_cbor() == files["image"] and c.encode_blocks_cbor(other) == files["view"]
        assert c.trace_cbor(product.Trace(*tr)) == files["trace"]
        c.upload_ingested()
        assert c.prove(root).proof_bytes == before
    finally:
        c.close()


# ------------------------------------------------------------ errors
def raw_encode_blocks(product, c, view):
    buf, err = product._lib.Buf(), C.create_string_buffer(512)
    rc = product.lib.sezkp_ctx_encode_blocks_cbor(c._h, C.byref(view), C.byref(buf), err, 512)
    assert rc != 0 and buf.len == 0 and not buf.data
    return rc, err.value.decode()


def test_errors_leave_the_context_usable(gpu_ok, product):
    t, tau, b = 4096, 2, 512
    tr = product.simulate(t, tau, 5)
    blocks = product.partition(*tr, b)
    root = blocks.manifest_root()
    c = product.ProverContext(0)
    try:
        # nothing uploaded, then an image uploaded as blocks
        with pytest.raises(product.SezkpError, match="no trace uploaded") as e:
            c.blocks_cbor()
        assert e.value.code == -1
        c.upload(blocks)
        want = c.prove(root).proof_bytes
        for call in (c.blocks_cbor, c.trace_cbor):
            with pytest.raises(product.SezkpError, match="uploaded as blocks") as e:
                call()
            assert e.value.code == -1
        # tau > 255 and null arrays, before any device call
        small = K.to_blocks(product, K.view([2, 1], 2))
        v = small.view()
        v.tau = 256
        assert raw_encode_blocks(product, c, v) == (-1, "block view: tau must be at most 255 (got 256)")
        for f in ("version", "step_start", "win_left", "off_out"):
            v = small.view()
            setattr(v, f, None)
            assert raw_encode_blocks(product, c, v) == (-1, "block view: null block table"), f
        for f in ("input_mv", "mv", "has_write", "wsym"):
            v = small.view()
            setattr(v, f, None)
            assert raw_encode_blocks(product, c, v) == (-1, "block view: null step array"), f
        bad = K.view([2, 1], 2)
        bad["step_start"] = np.array([0, 3, 2], np.uint64)
        v = K.to_blocks(product, bad).view()
        assert raw_encode_blocks(product, c, v) == (-1, "block view: step_start decreases at block 1")
        buf, err = product._lib.Buf(), C.create_string_buffer(512)
        assert product.lib.sezkp_ctx_encode_blocks_cbor(c._h, None, C.byref(buf), err, 512) == -1
        assert product.lib.sezkp_ctx_encode_blocks_cbor(c._h, C.byref(small.view()), None, err, 512) == -1
        tv = product._lib.TraceView()
        tv.t, tv.tau = 4, 256
        assert product.lib.sezkp_ctx_encode_trace_cbor(c._h, C.byref(tv), C.byref(buf), err, 512) == -1
        assert err.value == b"trace view: tau must be at most 255 (got 256)"
        tv.tau = 2
        assert product.lib.sezkp_ctx_encode_trace_cbor(c._h, C.byref(tv), C.byref(buf), err, 512) == -1
        assert err.value == b"trace view: null step array" and buf.len == 0
        assert c.prove(root).proof_bytes == want
        assert c.encode_blocks_cbor(small) == small.to_cbor()
    finally:
        c.close()


def test_a_sharded_context_refuses_and_proves_afterwards(gpu_ok, product):
    t, tau, b = 8192, 2, 512
    tr = product.simulate(t, tau, 9)
    c = product.ShardedProverContext(0, 2, 0, comm="solo")
    try:
        c.upload_trace(*tr, b)
        for call in (c.blocks_cbor, c.trace_cbor):
            with pytest.raises(product.SezkpError, match="not on a sharded context") as e:
                call()
            assert e.value.code == -1
        assert len(c.prove().proof_bytes) > 0
    finally:
        c.close()


# ------------------------------------------------------------ CLI
def test_cli_prove_from_a_trace_writes_the_same_blocks_on_both_paths(gpu_ok, tmp_path):
    outs = {}
    for tag, extra in (("dev", []), ("host", ["--host-decode"])):
        proof, blocks = str(tmp_path / f"{tag}_proof.cbor"), str(tmp_path / f"{tag}_blocks.cbor")
        r = subprocess.run([CLI, "prove", "--backend", "stark", "--trace", os.path.join(GOLDEN, "riscv_trace.cbor"),
                            "--b", "4", "--out", proof, "--out-blocks", blocks] + extra, capture_output=True, text=True)
        assert r.returncode == 0, (tag, r.stderr)
        outs[tag] = (open(proof, "rb").read(), open(blocks, "rb").read())
    assert outs["dev"] == outs["host"] and outs["dev"][1] == golden("riscv_blocks.cbor")
