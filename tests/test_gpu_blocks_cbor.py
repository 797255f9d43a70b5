"""Block-file CBOR decoded on the device (sezkp_ctx_ingest_blocks_cbor,
sezkp_ctx_upload_blocks_cbor, sezkp_ctx_decode_blocks_cbor): for every input
the result is what sezkp_blocks_decode_cbor followed by sezkp_ctx_upload gives:
the code, the message, the arrays and the proof bytes.

Yardsticks, none touched by this change: the host decoder
(`BlockSoA.from_cbor`), `ProverContext.upload` + `prove` of its blocks, and
`oracle_ctypes.prove_v1`. The corpora are in tests/blocks_cbor_corpus.py (A
canonical, B declined but decodable, C refused); tests/test_blocks_cbor_host.py
runs the same files through the shared header on the CPU under the sanitizers.

The host decoder keeps no tags (BlockSoA has none and to_cbor writes zero
tags), so "to_cbor() of the result is the input file" is asserted for every
file of A whose tags are zero, which is all of them but `tag_bytes`; for that
one to_cbor() equals the host decoder's.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import blocks_cbor_corpus as K
from conftest import GOLDEN, ORACLE, PKG, free_port
from test_gpu_sharded_trace import QUEUE_TIMEOUT, sha

pytestmark = pytest.mark.gpu
REF = open(os.path.join(GOLDEN, "ref_blocks.cbor"), "rb").read()
RISCV = open(os.path.join(GOLDEN, "riscv_blocks.cbor"), "rb").read()
CLI = os.path.join(PKG, "bin", "sezkp-cli")


@pytest.fixture(scope="module")
def ctx(gpu_ok, product, oracle):
    c = product.ProverContext(0)
    yield c
    c.close()


def device_decode(product, ctx, raw):
    try:
        return ("ok", ctx.decode_blocks_cbor(raw))
    except product.SezkpError as e:
        return ("err", e.code, str(e))


def assert_blocks_equal(name, got, want):
    assert (got.tau, got.n_blocks) == (want.tau, want.n_blocks), name
    for f in K.ARRAYS:
        g, w = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        assert g.dtype == w.dtype and g.shape == w.shape, (name, f, g.dtype, g.shape, w.dtype, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {f}")


def assert_same_as_host(product, ctx, name, raw, path=None):
    """Code, message and arrays of the decode-only entry point equal the host
    decoder's; path: the pinned path, or None."""
    want, got = K.host_decode(product, raw), device_decode(product, ctx, raw)
    st = ctx.blocks_ingest_stats()
    assert got[0] == want[0], (name, got[1:] if got[0] == "err" else "decoded", want[1:] if want[0] == "err" else "")
    if want[0] == "err":
        assert got[1:] == want[1:], name
        assert st["path"] == "host", (name, st)  # every error message is the host decoder's
    else:
        assert_blocks_equal(name, got[1], want[1])
    assert st["bytes"] == len(raw)
    if path is not None:
        assert st["path"] == path, (name, st)
    if st["path"] == "device":
        w = want[1]
        assert st["reason"] == "none" and st["ms_host"] == 0.0, (name, st)
        assert st["block_candidates"] >= st["n_blocks"] == w.n_blocks and st["tau"] == w.tau, (name, st)
        assert st["step_candidates"] >= st["t"] == int(w.step_start[-1]), (name, st)
    else:
        assert st["reason"] != "none", (name, st)
        if want[0] == "ok":  # the shape of what the host decoder gave, whatever the head said
            w = want[1]
            assert (st["n_blocks"], st["t"], st["tau"]) == (w.n_blocks, int(w.step_start[-1]), w.tau), (name, st)
    return st, got


# ------------------------------------------------------------ corpus A
@pytest.mark.parametrize("tau", [0, 1, 23, 24, 255])
def test_corpus_a_grid_of_head_length_thresholds(ctx, product, tau):
    for name, raw in K.corpus_a_grid():
        if name.startswith(f"grid_tau{tau}_"):
            _st, got = assert_same_as_host(product, ctx, name, raw, path="device")
            assert got[1].to_cbor() == raw, name


def test_corpus_a_fixtures_field_walk_tags_and_sizes(ctx, product):
    for name, raw in K.corpus_a_extremes():
        assert product.blocks_cbor_head(raw) is not None, name
        _st, got = assert_same_as_host(product, ctx, name, raw, path="device")
        if name == "tag_bytes":  # the decoder keeps no tags
            assert got[1].to_cbor() == product.BlockSoA.from_cbor(raw).to_cbor() != raw
        else:
            assert got[1].to_cbor() == raw, name
    assert_blocks_equal("ref", ctx.decode_blocks_cbor(REF), product.reference_blocks(64, 8, 2))


def test_corpus_a_signatures_that_straddle_the_mark_tiles(ctx, product):
    raw, offs, soffs = K.straddle_file()
    tile = K.tiling()["tile"]
    bcross, scross, rel = K.straddle_facts(offs, soffs, tile)
    # asserted here, on the CPU: a block signature and a step signature cross a
    # boundary of the marking kernel's per-workgroup byte tile, and blocks
    # start at tile offsets 0 and tile - 1
    assert bcross and all(o // tile != (o + len(K.BLOCK_SIG) - 1) // tile for o in bcross)
    assert scross and all(o // tile != (o + len(K.STEP_SIG) - 1) // tile for o in scross)
    assert 0 in rel and tile - 1 in rel
    st, got = assert_same_as_host(product, ctx, "straddle", raw, path="device")
    assert st["n_blocks"] == st["block_candidates"] == K.STRADDLE_B and st["t"] == st["step_candidates"] == len(soffs)
    assert got[1].to_cbor() == raw


def test_pageable_numpy_and_pinned_tensor_bytes_decode_alike(ctx, product, gpu_ok):
    raw = K.designed_file([7, 300, 1, 64] * 12, 3, 6)
    want = product.BlockSoA.from_cbor(raw)
    pinned = gpu_ok.frombuffer(bytearray(raw), dtype=gpu_ok.uint8).pin_memory()
    for data in (raw, np.frombuffer(raw, np.uint8), pinned):
        got = ctx.decode_blocks_cbor(data)
        assert ctx.blocks_ingest_stats()["path"] == "device"
        assert_blocks_equal("input kinds", got, want)


# ------------------------------------------------------------ corpus B, C
def test_corpus_b_declined_files_decode_as_on_the_host(ctx, product):
    for name, raw, pin in K.corpus_b():
        assert K.host_decode(product, raw)[0] == "ok", name
        st, _got = assert_same_as_host(product, ctx, name, raw, path=None if pin is None else "host")
        if pin is not None:
            reason, index = pin
            assert st["reason"] == reason and (index is None or st["index"] == index), (name, st)


def test_corpus_c_refused_files_give_the_host_decoders_error(ctx, product):
    for name, raw in K.corpus_c():
        assert K.host_decode(product, raw)[0] == "err", name
        assert_same_as_host(product, ctx, name, raw, path="host")


def test_corpus_c_one_changed_byte(ctx, product):
    for name, raw in K.corpus_flips():
        assert_same_as_host(product, ctx, name, raw)


# ------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def t4096(product):
    blocks = product.reference_blocks(4096, 512, 2)
    return blocks, blocks.to_cbor()


def proof_cases(product, t4096):
    return [("ref", REF), ("riscv", RISCV), ("t4096", t4096[1])]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_upload_by_cbor_proves_as_upload_of_the_decoded_blocks(ctx, product, oracle, t4096, which):
    name, raw = proof_cases(product, t4096)[which]
    want = product.BlockSoA.from_cbor(raw)
    root = want.manifest_root()
    ctx.upload_blocks_cbor(raw)
    st = ctx.blocks_ingest_stats()
    assert st["path"] == "device", (name, st)
    assert (ctx.tau, ctx.n_rows, ctx.n_blocks) == (want.tau, int(want.step_start[-1]), want.n_blocks)
    art = ctx.prove(root)
    other = product.ProverContext(0)
    try:
        other.upload(want)
        ref = other.prove(root)
    finally:
        other.close()
    assert art.proof_bytes == ref.proof_bytes and art.meta == ref.meta
    assert sha(art.proof_bytes) == sha(oracle.prove_v1(want, root))


def test_ingest_meta_gives_the_manifest_root_and_upload_ingested_the_proof(ctx, product, oracle, t4096):
    blocks, raw = t4096
    meta = ctx.ingest_blocks_cbor(raw)
    assert ctx.blocks_ingest_stats()["path"] == "device"
    assert meta.input_mv.size == meta.mv.size == meta.has_write.size == meta.wsym.size == 0
    for f in K.ARRAYS[:13]:
        np.testing.assert_array_equal(getattr(meta, f), getattr(blocks, f), err_msg=f)
    root = meta.manifest_root()
    assert root == blocks.manifest_root() == oracle.manifest_root(blocks)
    ctx.upload_ingested()
    assert ctx.prove(root).proof_bytes == oracle.prove_v1(blocks, root)
    # consumed: nothing is pending any more
    with pytest.raises(product.SezkpError) as e:
        ctx.upload_ingested()
    assert e.value.code == -1 and "no ingest is pending" in str(e.value)
    # and the next ingest drops the one before it
    ctx.ingest_blocks_cbor(raw)
    small = ctx.ingest_blocks_cbor(REF)
    assert small.n_blocks == 8
    ctx.upload_ingested()
    want = product.BlockSoA.from_cbor(REF)
    assert ctx.prove(want.manifest_root()).proof_bytes == oracle.prove_v1(want, want.manifest_root())


def test_upload_ingested_with_nothing_pending_is_invalid(gpu_ok, product):
    c = product.ProverContext(0)
    try:
        with pytest.raises(product.SezkpError) as e:
            c.upload_ingested()
        assert e.value.code == -1
        c.decode_blocks_cbor(REF)  # the parity entry leaves nothing pending either
        with pytest.raises(product.SezkpError) as e:
            c.upload_ingested()
        assert e.value.code == -1
    finally:
        c.close()


def test_forced_host_path_gives_the_same_proof(gpu_ok, product, monkeypatch, t4096):
    blocks, raw = t4096
    root = blocks.manifest_root()
    c = product.ProverContext(0)
    try:
        c.upload_blocks_cbor(raw)
        assert c.blocks_ingest_stats()["path"] == "device"
        dev = c.prove(root).proof_bytes
        monkeypatch.setenv("SEZKP_BLOCKS_CBOR_HOST", "1")  # read per call
        c.upload_blocks_cbor(raw)
        st = c.blocks_ingest_stats()
        assert (st["path"], st["reason"]) == ("host", "forced") and st["ms_host"] > 0 and st["ms_decode"] == 0
        assert (st["n_blocks"], st["t"], st["tau"], st["bytes"]) == (8, 4096, 2, len(raw))
        assert c.prove(root).proof_bytes == dev
        monkeypatch.setenv("SEZKP_BLOCKS_CBOR_HOST", "0")
        c.decode_blocks_cbor(raw)
        assert c.blocks_ingest_stats()["path"] == "device"
    finally:
        c.close()


def test_a_refused_file_leaves_the_uploaded_image_and_its_proofs_alone(ctx, product, t4096):
    blocks, raw = t4096
    root = blocks.manifest_root()
    ctx.upload_blocks_cbor(raw)
    before = ctx.prove(root).proof_bytes
    bad = dict(K.corpus_c())["mv_128"]
    for call in (ctx.upload_blocks_cbor, ctx.ingest_blocks_cbor, ctx.decode_blocks_cbor):
        with pytest.raises(product.SezkpError) as e:
            call(bad)
        assert (e.value.code, str(e.value)) == K.host_decode(product, bad)[1:] and e.value.code == -4
        assert ctx.blocks_ingest_stats()["path"] == "host"
    with pytest.raises(product.SezkpError) as e:
        ctx.upload_blocks_cbor(b"")
    assert (e.value.code, str(e.value)) == K.host_decode(product, b"")[1:]
    assert (ctx.tau, ctx.n_rows, ctx.n_blocks) == (2, 4096, 8)
    assert ctx.prove(root).proof_bytes == before


def test_blocks_that_upload_refuses_get_uploads_message(ctx, product):
    blocks = K.designed_blocks([512] * 8, 2, 1)
    blocks[3]["step_hi"] += 1
    raw = K.enc_blocks_file([K.enc_block(b) for b in blocks])[0]
    want = product.BlockSoA.from_cbor(raw)
    other = product.ProverContext(0)
    try:
        with pytest.raises(product.SezkpError) as ref:
            other.upload(want)
    finally:
        other.close()
    with pytest.raises(product.SezkpError) as e:
        ctx.upload_blocks_cbor(raw)
    assert ctx.blocks_ingest_stats()["path"] == "device"
    assert (e.value.code, str(e.value)) == (ref.value.code, str(ref.value))
    assert e.value.code == -1 and "block 3: step_hi-step_lo+1=513 but movement_log has 512 steps" in str(e.value)


def test_stateless_prove_blocks_cbor(gpu_ok, product, oracle):
    want = product.BlockSoA.from_cbor(REF)
    root = want.manifest_root()
    art = product.StarkV1.prove_blocks_cbor(REF, root)
    assert art.proof_bytes == oracle.prove_v1(want, root) and art.manifest_root == root
    assert art.meta == {"proto": "stark-v1", "domain_n": 512, "tau": 2}
    # a file the device path declines at the head is decoded once, on the host
    ind = b"\x9f" + REF[1:] + b"\xff"  # the same blocks in an indefinite-length array
    assert product.blocks_cbor_head(ind) is None
    assert product.StarkV1.prove_blocks_cbor(ind, root).proof_bytes == art.proof_bytes


# ------------------------------------------------------------ CLI
def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_prove_with_and_without_host_decode_writes_the_same_files(gpu_ok, product, tmp_path, t4096):
    blocks, raw = t4096
    bpath, mpath = str(tmp_path / "blocks.cbor"), str(tmp_path / "manifest.cbor")
    open(bpath, "wb").write(raw)
    r = run_cli("commit", "--blocks", bpath, "--out", mpath)
    assert r.returncode == 0, r.stderr
    outs, lines = {}, {}
    for tag, extra in (("dev", []), ("host", ["--host-decode"]), ("dev_assume", ["--assume-committed"])):
        out = str(tmp_path / f"{tag}.cbor")
        r = run_cli("prove", "--backend", "stark", "--blocks", bpath, "--manifest", mpath, "--out", out, *extra)
        assert r.returncode == 0, (tag, r.stderr)
        outs[tag], lines[tag] = open(out, "rb").read(), r.stdout.replace(out, "OUT")
    assert outs["dev"] == outs["host"] == outs["dev_assume"] and lines["dev"] == lines["host"]
    # a wrong manifest, a file that does not decode, a missing file: today's lines and exit codes
    other = str(tmp_path / "other.cbor")
    open(other, "wb").write(REF)
    wrong = str(tmp_path / "wrong_manifest.cbor")
    assert run_cli("commit", "--blocks", other, "--out", wrong).returncode == 0
    bad = str(tmp_path / "bad.cbor")
    open(bad, "wb").write(dict(K.corpus_c())["mv_128"])
    for blocks_arg, manifest_arg, extra, head in (
            (bpath, wrong, [], "Error: blocks/manifest mismatch: root mismatch: manifest="),
            (bad, mpath, [], f"Error: blocks/manifest mismatch: read blocks {bad}: deserialize CBOR block summaries: "),
            (bad, mpath, ["--assume-committed"], "Error: reading blocks: deserialize CBOR block summaries: "),
            (str(tmp_path / "none.cbor"), mpath, [], "Error: blocks/manifest mismatch: read blocks "),
            (bpath, str(tmp_path / "none_m.cbor"), [], "Error: blocks/manifest mismatch: ")):
        got = []
        for more in ([], ["--host-decode"]):
            out = str(tmp_path / "never.cbor")
            r = run_cli("prove", "--backend", "stark", "--blocks", blocks_arg, "--manifest", manifest_arg, "--out", out,
                        *extra, *more)
            assert r.returncode == 1 and not os.path.exists(out), (blocks_arg, r.stderr)
            got.append(r.stderr)
        assert got[0] == got[1] and got[0].startswith(head), got


def test_cli_audit_prints_the_same_on_both_paths(gpu_ok, product, tmp_path, t4096):
    bpath = str(tmp_path / "blocks.cbor")
    open(bpath, "wb").write(t4096[1])
    for fmt in ([], ["--json"]):
        a, b = run_cli("audit", "--blocks", bpath, *fmt), run_cli("audit", "--blocks", bpath, "--host-decode", *fmt)
        # 3: rows of the generator's trace violate the AIR, on either path
        assert a.returncode == b.returncode and a.returncode in (0, 3), (a.stderr, b.stderr)
        assert a.stdout == b.stdout and a.stdout and a.stderr == b.stderr == ""
    bad = str(tmp_path / "bad.cbor")
    open(bad, "wb").write(dict(K.corpus_c())["mv_128"])
    a, b = run_cli("audit", "--blocks", bad), run_cli("audit", "--blocks", bad, "--host-decode")
    assert a.returncode == b.returncode == 1 and a.stderr == b.stderr and a.stderr.startswith("Error: read blocks ")


# ------------------------------------------------------------ sharded
def _worker(rank, world, port, q):
    sys.path[:0] = [PKG, ORACLE]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sezkp_amd
        blocks = sezkp_amd.reference_blocks(8192, 512, 2)
        c = sezkp_amd.ShardedProverContext(rank, world, device=0, comm="host")
        c.upload_blocks_cbor(blocks.to_cbor())
        st = c.blocks_ingest_stats()
        art = c.prove(blocks.manifest_root())
        q.put({"rank": rank, "path": st["path"], "t": st["t"], "digest": sha(art.proof_bytes), "n_blocks": c.n_blocks})
        c.close()
    except Exception as e:
        q.put({"rank": rank, "error": f"{type(e).__name__}: {e}"})
    finally:
        dist.destroy_process_group()


def test_sharded_ranks_upload_by_cbor(gpu_ok, product):
    import torch.multiprocessing as mp
    world = 2
    blocks = product.reference_blocks(8192, 512, 2)
    root = blocks.manifest_root()
    single = product.ProverContext(0)
    try:
        single.upload(blocks)
        digest = sha(single.prove(root).proof_bytes)
    finally:
        single.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = free_port()
    ps = [mpc.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
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
        assert (o["path"], o["t"], o["n_blocks"]) == ("device", 8192, 16)
        assert o["digest"] == digest
