"""TraceFile CBOR decoded on the device (sezkp_ctx_upload_trace_cbor,
sezkp_ctx_decode_trace_cbor): for every input the result is what
sezkp_trace_decode_cbor followed by sezkp_ctx_upload_trace gives.

Yardsticks, none touched by this change: the host decoder
(`Trace.from_cbor`), `upload_trace` of its arrays, the numpy `partition`,
`oracle.manifest_root` and `oracle_ctypes.prove_v1`. The corpora are in
tests/trace_cbor_corpus.py (A canonical, B declined but decodable, C refused);
tests/test_trace_cbor_host.py runs the same files through the shared header on
the CPU under the sanitizers.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import trace_cbor_corpus as K
from conftest import GOLDEN, ORACLE, PKG, free_port
from test_gpu_sharded_trace import QUEUE_TIMEOUT, sha, want as sharded_want
from test_gpu_trace_upload import assert_blocks_equal, make_trace

pytestmark = pytest.mark.gpu
FIXTURE = open(os.path.join(GOLDEN, "riscv_trace.cbor"), "rb").read()
NAMES = ("input_mv", "mv", "has_write", "wsym")


@pytest.fixture(scope="module")
def ctx(gpu_ok, product, oracle):
    c = product.ProverContext(0)
    yield c
    c.close()


def device_decode(product, ctx, raw):
    try:
        return ("ok", ctx.decode_trace_cbor(raw).arrays())
    except product.SezkpError as e:
        return ("err", e.code, str(e))


def assert_same_as_host(product, ctx, name, raw, path=None):
    """Code, message and arrays of the decode-only entry point equal the host
    decoder's; path: the pinned path, or None."""
    want, got = K.host_decode(product, raw), device_decode(product, ctx, raw)
    st = ctx.trace_ingest_stats()
    assert got[0] == want[0], (name, got[1:] if got[0] == "err" else "decoded", want[1:] if want[0] == "err" else "")
    if want[0] == "err":
        assert got[1:] == want[1:], name
        assert st["path"] == "host", (name, st)  # every error message is the host decoder's
    else:
        for g, w, arr in zip(got[1], want[1], NAMES):
            assert g.dtype == w.dtype and g.shape == w.shape, (name, arr)
            np.testing.assert_array_equal(g, w, err_msg=f"{name}: {arr}")
    assert st["bytes"] == len(raw)
    if path is not None:
        assert st["path"] == path, (name, st)
    if st["path"] == "device":
        assert st["reason"] == "none" and st["candidates"] >= st["t"] == len(want[1][0]), (name, st)
        assert st["tau"] == want[1][1].shape[1] and st["ms_host"] == 0.0, (name, st)
    else:
        assert st["reason"] != "none", (name, st)
        if want[0] == "ok":  # the shape of what the host decoder gave, whatever the head said
            assert (st["t"], st["tau"]) == (len(want[1][0]), want[1][1].shape[1]), (name, st)
    return st


# ------------------------------------------------------------ corpus A
def test_corpus_a_grid_of_head_length_thresholds(ctx, product):
    for name, raw in K.corpus_a_small():
        assert_same_as_host(product, ctx, name, raw, path="device")


def test_corpus_a_fixture_and_extreme_step_lengths(ctx, product):
    for name, raw in K.corpus_a_extremes():
        assert_same_as_host(product, ctx, name, raw, path="device")
    tr = ctx.decode_trace_cbor(FIXTURE)
    for got, ref in zip(tr.arrays(), product.reference_trace(32, 2)):
        np.testing.assert_array_equal(got, ref)
    assert tr.to_cbor() == FIXTURE


def test_corpus_a_encoded_files_around_2_16_steps_and_the_tile(ctx, product):
    for name, raw in K.corpus_a_encoded(product):
        assert product.trace_cbor_head(raw) is not None, name
        assert_same_as_host(product, ctx, name, raw, path="device")


def test_corpus_a_steps_that_straddle_the_mark_tiles(ctx, product):
    raw, offs = K.straddle_file()
    tile = K.tiling()["tile"]
    crossing, rel = K.straddle_facts(offs, tile)
    # asserted here, on the CPU: a signature crosses a boundary of the marking
    # kernel's per-workgroup byte tile, and steps start at tile offsets 0 and tile - 1
    assert crossing and all(o // tile != (o + len(K.SIG) - 1) // tile for o in crossing)
    assert 0 in rel and tile - 1 in rel
    st = assert_same_as_host(product, ctx, "straddle", raw, path="device")
    assert st["t"] == st["candidates"] == K.STRADDLE_T


def test_pageable_numpy_and_pinned_tensor_bytes_decode_alike(ctx, product, gpu_ok):
    raw = K.np_trace(product, 5000, 3, 77).to_cbor()
    want = K.host_decode(product, raw)[1]
    pinned = gpu_ok.frombuffer(bytearray(raw), dtype=gpu_ok.uint8).pin_memory()
    for data in (raw, np.frombuffer(raw, np.uint8), pinned):
        got = ctx.decode_trace_cbor(data).arrays()
        assert ctx.trace_ingest_stats()["path"] == "device"
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


# ------------------------------------------------------------ corpus B, C
def test_corpus_b_declined_files_decode_as_on_the_host(ctx, product):
    reasons = {}
    for name, raw, pinned in K.corpus_b():
        assert K.host_decode(product, raw)[0] == "ok", name
        st = assert_same_as_host(product, ctx, name, raw, path="host" if pinned else None)
        reasons[name] = (st["reason"], st["index"])
    assert reasons["tapes_before_input_mv"][0] in ("candidates", "step", "chain")
    assert reasons["non_minimal_int"] == ("step", 7)
    assert reasons["unknown_tape_key"] == ("step", 9)
    assert reasons["indefinite_steps"][0] == reasons["top_level_key_order"][0] == "head"
    assert reasons["meta_map"][0] == "tail"


def test_corpus_c_refused_files_give_the_host_decoders_error(ctx, product):
    for name, raw in K.corpus_c():
        assert K.host_decode(product, raw)[0] == "err", name
        assert_same_as_host(product, ctx, name, raw, path="host")


def test_corpus_c_one_changed_byte(ctx, product):
    for name, raw in K.corpus_flips():
        assert_same_as_host(product, ctx, name, raw)


def test_upload_of_a_refused_file_leaves_the_trace_image_alone(ctx, product):
    ctx.upload_trace_cbor(FIXTURE, 4)
    root = ctx.manifest_root()
    bad = dict(K.corpus_c())["mv_128"]
    with pytest.raises(product.SezkpError) as e:
        ctx.upload_trace_cbor(bad, 4)
    assert (e.value.code, str(e.value)) == K.host_decode(product, bad)[1:]
    assert e.value.code == -4
    assert ctx.manifest_root() == root and (ctx.n_rows, ctx.tau) == (32, 2)
    with pytest.raises(product.SezkpError) as e:
        ctx.upload_trace_cbor(FIXTURE, 0)
    assert e.value.code == -1
    # upload errors are upload_trace's: 300 rows are no power of two
    with pytest.raises(product.SezkpError) as e:
        ctx.upload_trace_cbor(K.designed_file(300, 2), 4)
    assert (e.value.code, str(e.value)) == (-1, "[-1] n_base must be a power of two (got 300)")


# ------------------------------------------------------------ end to end
@pytest.mark.parametrize("name,t,tau,b", [("fixture", 32, 2, 4), ("t8192", 8192, 3, 333)])
def test_upload_by_cbor_proves_as_upload_of_the_decoded_arrays(ctx, product, oracle, name, t, tau, b):
    if name == "fixture":
        raw, arrays = FIXTURE, product.reference_trace(32, 2)
    else:
        arrays = make_trace(t, tau, b, "random")
        raw = product.Trace(*arrays).to_cbor()
    ctx.upload_trace_cbor(raw, b)
    assert ctx.trace_ingest_stats()["path"] == "device"
    assert (ctx.tau, ctx.n_rows, ctx.n_blocks) == (tau, t, -(-t // b))
    art = ctx.prove()
    # yardstick 1: upload_trace of the host-decoded arrays on a second context
    other = product.ProverContext(0)
    try:
        other.upload_trace(*product.Trace.from_cbor(raw).arrays(), b)
        ref = other.prove()
        assert art.proof_bytes == ref.proof_bytes and art.manifest_root == ref.manifest_root
        assert ctx.manifest_root() == other.manifest_root()
        assert_blocks_equal(product, ctx.blocks(), other.blocks())
    finally:
        other.close()
    # yardstick 2: the oracle's proof of the numpy partition
    blocks = product.partition(*arrays, b)
    root = blocks.manifest_root()
    assert root == oracle.manifest_root(blocks) == ctx.manifest_root() == art.manifest_root
    assert sha(art.proof_bytes) == sha(oracle.prove_v1(blocks, root))
    assert_blocks_equal(product, ctx.blocks(), blocks)
    assert art.meta == {"proto": "stark-v1", "domain_n": 8 * t, "tau": tau}


def test_stateless_prove_trace_cbor(gpu_ok, product, oracle):
    art = product.StarkV1.prove_trace_cbor(FIXTURE, 4)
    blocks = product.partition(*product.reference_trace(32, 2), 4)
    assert art.manifest_root == blocks.manifest_root()
    assert art.proof_bytes == oracle.prove_v1(blocks, art.manifest_root)
    assert art.meta == {"proto": "stark-v1", "domain_n": 256, "tau": 2}
    assert product.StarkV1.prove_trace_cbor(FIXTURE, 4, streaming=True).meta["mode"] == "streaming"


def test_context_reuse_across_upload_kinds_and_growing_files(gpu_ok, product, oracle):
    c = product.ProverContext(0)
    try:
        c.upload_trace_cbor(FIXTURE, 4)
        small = c.prove().proof_bytes
        blocks = product.synthetic_blocks(1 << 12, 512, 8, 42)
        c.upload(blocks)
        assert c.prove(blocks.manifest_root()).proof_bytes == oracle.prove_v1(blocks, blocks.manifest_root())
        t, tau, b = 16384, 5, 1000  # a larger file and trace: every buffer grows
        tr = K.np_trace(product, t, tau, 3)
        c.upload_trace_cbor(tr.to_cbor(), b)
        assert c.trace_ingest_stats()["path"] == "device"
        want = product.partition(*tr.arrays(), b)
        assert c.manifest_root() == want.manifest_root()
        assert_blocks_equal(product, c.blocks(), want)
        c.upload_trace_cbor(FIXTURE, 4)  # and back to the small one, in the kept buffers
        assert c.prove().proof_bytes == small
    finally:
        c.close()


def test_forced_host_path_gives_the_same_bytes(gpu_ok, product, monkeypatch):
    c = product.ProverContext(0)
    try:
        c.upload_trace_cbor(FIXTURE, 4)
        dev = (c.prove().proof_bytes, c.manifest_root(), c.blocks().to_cbor())
        assert c.trace_ingest_stats()["path"] == "device"
        shape, meta, leaves = (c.tau, c.n_rows, c.n_blocks), c.prove().meta, c.manifest_leaves()
        assert shape == (2, 32, 8) and meta == {"proto": "stark-v1", "domain_n": 256, "tau": 2} and len(leaves) == 256
        monkeypatch.setenv("SEZKP_TRACE_CBOR_HOST", "1")  # read per call
        c.tau = c.n_rows = c.n_blocks = -1
        c.upload_trace_cbor(FIXTURE, 4)
        st = c.trace_ingest_stats()
        assert (st["path"], st["reason"]) == ("host", "forced") and st["ms_host"] > 0 and st["ms_decode"] == 0
        assert (st["t"], st["tau"], st["bytes"]) == (32, 2, len(FIXTURE))
        assert (c.tau, c.n_rows, c.n_blocks) == shape
        art = c.prove()
        assert art.meta == meta and c.manifest_leaves() == leaves
        assert (art.proof_bytes, c.manifest_root(), c.blocks().to_cbor()) == dev
        audit = c.air_audit(bitmaps=True)
        assert audit.n_rows == 32
        monkeypatch.setenv("SEZKP_TRACE_CBOR_HOST", "0")
        c.decode_trace_cbor(FIXTURE)
        assert c.trace_ingest_stats()["path"] == "device"
    finally:
        c.close()


@pytest.mark.parametrize("kind", ["indefinite_steps", "top_level_key_order", "meta_map"])
def test_upload_of_a_declined_file_is_upload_of_its_decoded_arrays(gpu_ok, product, kind):
    """Files the device path declines (two at the head, one at the tail) and
    the host decoder accepts, of a shape that can be proved: everything the
    context reports is what upload_trace of the decoded arrays gives."""
    t, tau, b = 64, 2, 8
    body = b"".join(K.enc_step(m, tp) for m, tp in K.designed_steps(t, tau, 5))
    pre = b"\xa4" + K.text("version") + K.head(0, 1) + K.text("tau") + K.head(0, tau) + K.text("steps")
    raw = {"indefinite_steps": pre + b"\x9f" + body + b"\xff" + K.text("meta") + b"\xf6",
           "top_level_key_order": b"\xa4" + K.text("tau") + K.head(0, tau) + K.text("version") + K.head(0, 1) +
           K.text("steps") + K.head(4, t) + body + K.text("meta") + b"\xf6",
           "meta_map": pre + K.head(4, t) + body + K.text("meta") + b"\xa1" + K.text("k") + K.head(0, 1)}[kind]
    tr = product.Trace.from_cbor(raw)
    c, ref = product.ProverContext(0), product.ProverContext(0)
    try:
        ref.upload_trace(*tr.arrays(), b)
        c.upload_trace_cbor(raw, b)
        st = c.trace_ingest_stats()
        assert (st["path"], st["reason"]) == ("host", "tail" if kind == "meta_map" else "head")
        assert (st["t"], st["tau"]) == (t, tau)
        assert (c.tau, c.n_rows, c.n_blocks) == (ref.tau, ref.n_rows, ref.n_blocks) == (tau, t, t // b)
        got, want = c.prove(), ref.prove()
        assert got.meta == want.meta == {"proto": "stark-v1", "domain_n": 8 * t, "tau": tau}
        assert got.proof_bytes == want.proof_bytes and got.to_cbor() == want.to_cbor()
        assert c.manifest_leaves() == ref.manifest_leaves() and len(c.manifest_leaves()) == 32 * (t // b)
        assert c.manifest_root() == ref.manifest_root()
        # the stateless form decodes such a file once, on the host, and uploads its arrays
        art = product.StarkV1.prove_trace_cbor(raw, b)
        assert (art.proof_bytes, art.manifest_root, art.meta) == (want.proof_bytes, want.manifest_root, want.meta)
    finally:
        c.close()
        ref.close()


def test_launcher_writes_the_shape_of_a_file_the_device_declines(gpu_ok, product, tmp_path):
    """`launch prove --trace` on a file with an indefinite `steps` array: the
    manifest's leaf count and the artifact's tau are the decoded trace's."""
    import cbor_min
    t, tau, b = 64, 2, 8
    body = b"".join(K.enc_step(m, tp) for m, tp in K.designed_steps(t, tau, 5))
    raw = (b"\xa4" + K.text("version") + K.head(0, 1) + K.text("tau") + K.head(0, tau) + K.text("steps") + b"\x9f" +
           body + b"\xff" + K.text("meta") + b"\xf6")
    (tmp_path / "t.cbor").write_bytes(raw)
    want = product.partition(*product.Trace.from_cbor(raw).arrays(), b)
    r = subprocess.run([sys.executable, "-m", "sezkp_amd.launch", "prove", "--trace", str(tmp_path / "t.cbor"), "--b",
                        str(b), "--out", str(tmp_path / "p.cbor"), "--out-manifest", str(tmp_path / "m.cbor"),
                        "--gpus", "1"], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    man = cbor_min.loads((tmp_path / "m.cbor").read_bytes())
    assert man["n_leaves"] == want.n_blocks == 8 and bytes(man["root"]) == want.manifest_root()
    art = cbor_min.loads((tmp_path / "p.cbor").read_bytes())
    assert art["meta"] == {"proto": "stark-v1", "domain_n": 8 * t, "tau": tau}
    assert bytes(art["manifest_root"]) == want.manifest_root()


def test_cli_with_and_without_host_decode_writes_the_same_files(gpu_ok, product, tmp_path):
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    tr = K.np_trace(product, 4096, 3, 5)
    trace = str(tmp_path / "trace.cbor")
    open(trace, "wb").write(tr.to_cbor())
    outs = {}
    for tag, extra in (("dev", []), ("host", ["--host-decode"])):
        files = {k: str(tmp_path / f"{tag}_{k}") for k in ("proof.cbor", "blocks.cbor", "manifest.cbor")}
        r = subprocess.run([cli, "prove", "--backend", "stark", "--trace", trace, "--b", "100", "--out",
                            files["proof.cbor"], "--out-blocks", files["blocks.cbor"], "--out-manifest",
                            files["manifest.cbor"]] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs[tag] = {k: open(f, "rb").read() for k, f in files.items()}
    assert outs["dev"] == outs["host"]
    assert outs["dev"]["blocks.cbor"] == product.partition(*tr.arrays(), 100).to_cbor()
    # a canonical head and a bad body: the same line and exit code
    bad = str(tmp_path / "bad.cbor")
    open(bad, "wb").write(dict(K.corpus_c())["mv_128"])
    msgs = []
    for extra in ([], ["--host-decode"]):
        r = subprocess.run([cli, "prove", "--backend", "stark", "--trace", bad, "--b", "4", "--out",
                            str(tmp_path / "none.cbor")] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and not os.path.exists(str(tmp_path / "none.cbor"))
        msgs.append(r.stderr)
    assert msgs[0] == msgs[1] == "Error: reading trace: deserialize CBOR trace: mv out of i8 range\n"


# ------------------------------------------------------------ sharded
def _worker(rank, world, port, shape, q):
    sys.path[:0] = [PKG, ORACLE]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sezkp_amd
        t, tau, b, moves = shape
        raw = sezkp_amd.Trace(*make_trace(t, tau, b, moves)).to_cbor()
        c = sezkp_amd.ShardedProverContext(rank, world, device=0, comm="host")
        c.upload_trace_cbor(raw, b)
        st = c.trace_ingest_stats()
        art = c.prove()
        q.put({"rank": rank, "path": st["path"], "t": st["t"], "digest": sha(art.proof_bytes),
               "art_root": art.manifest_root, "root": c.manifest_root(), "n_blocks": c.n_blocks})
        c.close()
    except Exception as e:
        q.put({"rank": rank, "error": f"{type(e).__name__}: {e}"})
    finally:
        dist.destroy_process_group()


def test_sharded_ranks_upload_by_cbor(gpu_ok):
    """Shape 2 of tests/test_gpu_sharded_trace.py: a block straddles the rank boundary."""
    import torch.multiprocessing as mp
    world, shape = 2, (8192, 3, 333, "random")
    blocks, root, _frontier, _leaves, digest = sharded_want(*shape)
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = free_port()
    ps = [mpc.Process(target=_worker, args=(r, world, port, shape, q)) for r in range(world)]
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
        assert (o["path"], o["t"], o["n_blocks"]) == ("device", 8192, blocks.n_blocks)
        assert o["digest"] == digest and o["art_root"] == o["root"] == root


def test_rank_alone_context_of_one_rank_refuses(gpu_ok, product):
    err = __import__("ctypes").create_string_buffer(1024)
    h = product.lib.sezkp_ctx_create_sharded_solo(0, 0, 1, err, 1024)
    assert h
    try:
        buf = np.frombuffer(FIXTURE, np.uint8)
        rc = product.lib.sezkp_ctx_upload_trace_cbor(h, buf.ctypes.data, len(FIXTURE), 4, err, 1024)
        assert rc == -1 and err.value.startswith(b"upload_trace: not on a rank-alone sharded context of one rank")
    finally:
        product.lib.sezkp_ctx_destroy(h)
