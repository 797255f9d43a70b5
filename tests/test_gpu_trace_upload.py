"""Proving from a raw trace on the GPU: partition_trace and the manifest root
computed by the device (sezkp_ctx_upload_trace / stage_trace) against the
yardsticks this change does not touch: the numpy `partition`, the native
`sezkp_simulate_blocks`, `oracle.manifest_root` and `oracle.prove_v1`.

Shapes (t, tau, b): the fixtures' own, the headline's block shape, one block
per row (4096 blocks: more than one scan tile, a 4096-leaf tree, the
lane-per-block sum form), a ragged last block with 13 leaves (odd promotions,
and a count at which the Frontier root differs), 293 blocks, a single block,
both sides of the one-chunk leaf condition (40 / 41 tapes), and 2^15 blocks
(above what one workgroup reduces: the tree starts with level launches).
Moves are designed, not only random: all zero, all -1 / +1, +-127 alternating
per block, and an input head moving by -128 or +127 per row."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPES = [(32, 2, 4), (64, 2, 8), (4096, 8, 512), (4096, 8, 1), (4096, 3, 333), (2048, 8, 7), (1024, 1, 1024),
          (1024, 40, 256), (1024, 41, 256)]
BIG_TREE = (1 << 15, 1, 1)  # blocks, leaves and roots only
MOVES = ["random", "zero", "minus", "plus", "alt127"]
FROM_BLOCKS_MSG = "manifest root from the trace: the active trace image was uploaded as blocks"


@functools.lru_cache(maxsize=None)
def make_trace(t, tau, b, moves, seed=5):
    """(input_mv, mv, has_write, wsym), read-only: shared between the tests."""
    rng = np.random.Generator(np.random.PCG64(seed + 31 * t + 7 * tau + b))
    hw = (rng.random((t, tau)) < 0.4).astype(np.uint8)
    ws = (rng.integers(0, 16, size=(t, tau), dtype=np.uint16) * hw).astype(np.uint16)
    imv = rng.integers(-1, 2, size=t, dtype=np.int8)
    if moves == "random":
        mv = rng.integers(-1, 2, size=(t, tau), dtype=np.int8)
    elif moves == "clean":  # heads never below 0, symbols below 16: the AIR holds on every row
        mv = rng.integers(0, 2, size=(t, tau), dtype=np.int8)
    elif moves == "zero":  # windows [0, 0]
        mv = np.zeros((t, tau), np.int8)
    elif moves == "minus":  # right end pinned at 0; the input head falls by 128 a row
        mv = np.full((t, tau), -1, np.int8)
        imv = np.full(t, -128, np.int8)
    elif moves == "plus":  # left end pinned at 0; the input head rises by 127 a row
        mv = np.full((t, tau), 1, np.int8)
        imv = np.full(t, 127, np.int8)
    elif moves == "alt127":  # +127 on even blocks, -127 on odd ones
        sign = 1 - 2 * ((np.arange(t) // b) & 1)
        mv = np.repeat((127 * sign).astype(np.int8)[:, None], tau, axis=1)
    else:
        raise ValueError(moves)
    out = (imv, np.ascontiguousarray(mv), hw, ws)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_blocks(t, tau, b, moves):
    import sezkp_amd
    return sezkp_amd.partition(*make_trace(t, tau, b, moves), b)


@functools.lru_cache(maxsize=None)
def want_proof(t, tau, b, moves, root):
    import oracle_ctypes
    return oracle_ctypes.prove_v1(want_blocks(t, tau, b, moves), root)


@pytest.fixture(scope="module")
def ctx(gpu_ok, product, oracle):
    c = product.ProverContext(0)
    yield c
    c.close()


def assert_blocks_equal(product, got, want):
    assert (got.tau, got.n_blocks) == (want.tau, want.n_blocks)
    for name, _ in product._lib.VIEW_FIELDS:
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg=name)


# ------------------------------------------------------------ blocks, leaves, both roots
@pytest.mark.parametrize("t,tau,b,moves", [s + (m,) for s in SHAPES for m in MOVES] +
                         [BIG_TREE + ("random",), BIG_TREE + ("minus",)])
def test_blocks_leaves_and_roots(ctx, product, oracle, t, tau, b, moves):
    tr = make_trace(t, tau, b, moves)
    want = want_blocks(t, tau, b, moves)
    ctx.upload_trace(*tr, b)
    assert (ctx.tau, ctx.n_rows, ctx.n_blocks) == (tau, t, want.n_blocks)
    assert_blocks_equal(product, ctx.blocks(), want)
    leaves = want.leaf_hashes()
    assert ctx.manifest_leaves() == leaves
    assert ctx.manifest_root() == oracle.manifest_root(want) == want.manifest_root()
    assert ctx.manifest_root(frontier=True) == want.manifest_frontier_root()
    if want.n_blocks == 13:
        assert ctx.manifest_root(frontier=True) != ctx.manifest_root()


def test_in_head_scan_is_exact_on_both_signs(ctx, product):
    """-128 and +127 a row over 4096 one-row blocks: four scan tiles, sums far
    outside what 16 or 32 bits hold per tile."""
    for moves, per_row in (("minus", -128), ("plus", 127)):
        ctx.upload_trace(*make_trace(4096, 8, 1, moves), 1)
        got = ctx.blocks()
        np.testing.assert_array_equal(got.in_head_in, per_row * np.arange(4096, dtype=np.int64))
        np.testing.assert_array_equal(got.in_head_out, per_row * np.arange(1, 4097, dtype=np.int64))


# ------------------------------------------------------------ reference pins
@pytest.mark.parametrize("name,t,b,blocks_file,manifest_file", [
    ("root_blocks", 64, 8, "ref_blocks.cbor", "ref_manifest.cbor"),
    ("minimal_riscv", 32, 4, "riscv_blocks.cbor", "riscv_manifest.cbor"),
])
def test_reference_fixtures_from_the_trace(ctx, product, name, t, b, blocks_file, manifest_file):
    import cbor_min
    tr = product.reference_trace(t, 2)
    ctx.upload_trace(*tr, b)
    assert ctx.blocks().to_cbor() == open(os.path.join(GOLDEN, blocks_file), "rb").read()
    man = cbor_min.loads(open(os.path.join(GOLDEN, manifest_file), "rb").read())
    assert ctx.manifest_root() == bytes(man["root"]) and man["n_leaves"] == ctx.n_blocks
    art = ctx.prove()
    assert art.manifest_root == bytes(man["root"])
    gold = json.load(open(os.path.join(GOLDEN, "v1_proofs.json")))[name]
    assert hashlib.sha256(art.proof_bytes).hexdigest() == gold["proof_sha256"]
    assert art.meta == {"proto": "stark-v1", "domain_n": 8 * t, "tau": 2}


def test_riscv_trace_file_from_cbor(ctx, product):
    raw = open(os.path.join(GOLDEN, "riscv_trace.cbor"), "rb").read()
    ctx.upload_trace(*product.Trace.from_cbor(raw).arrays(), 4)
    assert ctx.blocks().to_cbor() == open(os.path.join(GOLDEN, "riscv_blocks.cbor"), "rb").read()


def test_cli_prove_from_the_trace_file(gpu_ok, tmp_path):
    """`sezkp-cli prove --trace`: the proof, the blocks and the manifest are the
    reference's committed ones; a manifest of another root is refused."""
    import subprocess

    import cbor_min
    from conftest import PKG
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    g = lambda f: os.path.join(GOLDEN, f)
    out = {k: str(tmp_path / k) for k in ("proof.cbor", "blocks.cbor", "manifest.cbor", "blocks.jsonl", "m2.cbor")}
    base = [cli, "prove", "--backend", "stark", "--trace", g("riscv_trace.cbor"), "--b", "4"]
    r = subprocess.run(base + ["--out", out["proof.cbor"], "--out-blocks", out["blocks.cbor"], "--out-manifest",
                               out["manifest.cbor"], "--manifest", g("riscv_manifest.cbor")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out["blocks.cbor"], "rb").read() == open(g("riscv_blocks.cbor"), "rb").read()
    assert open(out["manifest.cbor"], "rb").read() == open(g("riscv_manifest.cbor"), "rb").read()
    art = cbor_min.loads(open(out["proof.cbor"], "rb").read())
    man = cbor_min.loads(open(g("riscv_manifest.cbor"), "rb").read())
    assert art["backend"] == "stark" and bytes(art["manifest_root"]) == bytes(man["root"])
    gold = json.load(open(g("v1_proofs.json")))["minimal_riscv"]
    assert hashlib.sha256(bytes(art["proof_bytes"])).hexdigest() == gold["proof_sha256"]
    assert art["meta"] == {"proto": "stark-v1", "domain_n": 256, "tau": 2}
    # JSON Lines blocks are committed with the Frontier root, as `commit` does for them
    r = subprocess.run(base + ["--out", out["proof.cbor"], "--out-blocks", out["blocks.jsonl"], "--out-manifest",
                               out["m2.cbor"]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([cli, "verify-commit", "--blocks", out["blocks.jsonl"], "--manifest", out["m2.cbor"]],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # a manifest of another trace
    os.remove(out["proof.cbor"])
    r = subprocess.run(base + ["--out", out["proof.cbor"], "--manifest", g("ref_manifest.cbor")],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "manifest root mismatch" in r.stderr
    assert not os.path.exists(out["proof.cbor"])


# ------------------------------------------------------------ proof parity
@pytest.mark.parametrize("t,tau,b", SHAPES)
def test_proof_from_trace_is_the_oracles(ctx, product, oracle, t, tau, b):
    moves = "random"
    want = want_blocks(t, tau, b, moves)
    root = want.manifest_root()
    ctx.upload_trace(*make_trace(t, tau, b, moves), b)
    art = ctx.prove()
    assert art.manifest_root == root
    assert art.proof_bytes == want_proof(t, tau, b, moves, root)
    assert ctx.prove().proof_bytes == art.proof_bytes
    assert bytes(ctx.prove_view()) == art.proof_bytes


@pytest.mark.parametrize("t,tau,b", [(64, 2, 8), (4096, 3, 333)])
def test_explicit_root_on_a_trace_image_is_used_as_given(ctx, product, oracle, t, tau, b):
    other = bytes(range(32))
    ctx.upload_trace(*make_trace(t, tau, b, "random"), b)
    art = ctx.prove(other)
    assert art.manifest_root == other
    assert art.proof_bytes == want_proof(t, tau, b, "random", other)
    assert ctx.manifest_root() == want_blocks(t, tau, b, "random").manifest_root()
    assert ctx.prove().proof_bytes == want_proof(t, tau, b, "random", ctx.manifest_root())


@pytest.mark.parametrize("moves", ["alt127", "minus"])
def test_proof_from_trace_designed_moves(ctx, product, oracle, moves):
    t, tau, b = 4096, 3, 333
    want = want_blocks(t, tau, b, moves)
    ctx.upload_trace(*make_trace(t, tau, b, moves), b)
    assert ctx.prove().proof_bytes == want_proof(t, tau, b, moves, want.manifest_root())


def test_stateless_prove_trace(gpu_ok, product, oracle):
    t, tau, b = 2048, 8, 7
    want = want_blocks(t, tau, b, "clean")
    art = product.StarkV1.prove_trace(*make_trace(t, tau, b, "clean"), b)
    assert art.manifest_root == want.manifest_root()
    assert art.proof_bytes == want_proof(t, tau, b, "clean", art.manifest_root)
    assert art.meta == {"proto": "stark-v1", "domain_n": 8 * t, "tau": tau}
    product.StarkV1.verify(art, want, art.manifest_root)


def test_dictionary_plans_do_not_depend_on_the_upload_path(gpu_ok, product):
    t, tau, b = 4096, 8, 512
    want = want_blocks(t, tau, b, "random")
    root = want.manifest_root()
    a, c = product.ProverContext(0), product.ProverContext(0)
    try:
        a.upload_trace(*make_trace(t, tau, b, "random"), b)
        c.upload(want)
        first = a.prove().proof_bytes
        assert first == c.prove(root).proof_bytes
        assert a.dict_plans() == c.dict_plans() and a.dict_plans()
        assert a.dict_cache_stats() == c.dict_cache_stats()
        assert a.prove().proof_bytes == c.prove(root).proof_bytes == first  # warm
        assert a.dict_cache_stats() == c.dict_cache_stats()
        assert a.dict_cache_stats()["cols_rebuilt"] == 0
        assert a.pw_table_stats() == c.pw_table_stats()
        assert a.head_wide_stats() == c.head_wide_stats()
    finally:
        a.close()
        c.close()


def test_block_upload_reports_nothing_of_a_trace(gpu_ok, product):
    """A block-uploaded image has no device partition: the reports and the
    flag say so, and its proofs and stage times are the ones of before."""
    t, tau, b = 4096, 8, 512
    want = want_blocks(t, tau, b, "random")
    c = product.ProverContext(0)
    try:
        c.upload(want)
        for call in (c.manifest_root, c.manifest_leaves, c.blocks):
            with pytest.raises(product.SezkpError, match="uploaded as blocks") as e:
                call()
            assert e.value.code == -1
        for call in (c.prove, c.prove_view, c.prove_async):
            with pytest.raises(product.SezkpError) as e:
                call()
            assert e.value.code == -1 and FROM_BLOCKS_MSG in str(e.value)
        art = c.prove(want.manifest_root())
        assert art.proof_bytes == want_proof(t, tau, b, "random", want.manifest_root())
        assert len(c.stage_times_ms()) == len(product.STAGES)
    finally:
        c.close()


# ------------------------------------------------------------ staging
def test_staged_traces_each_get_their_own_root_and_proof(gpu_ok, product, oracle):
    t, tau, b = 4096, 8, 512
    A, B = make_trace(t, tau, b, "random"), make_trace(t, tau, b, "alt127")
    wa, wb = want_blocks(t, tau, b, "random"), want_blocks(t, tau, b, "alt127")
    ra, rb = wa.manifest_root(), wb.manifest_root()
    pa, pb = want_proof(t, tau, b, "random", ra), want_proof(t, tau, b, "alt127", rb)
    c = product.ProverContext(0)
    try:
        c.upload_trace(*A, b)
        c.stage_trace(*B, b)
        with pytest.raises(product.SezkpError, match="staged trace is pending"):
            c.manifest_root()
        art = c.prove()
        assert (art.manifest_root, art.proof_bytes) == (rb, pb)
        assert_blocks_equal(product, c.blocks(), wb)
        c.prove_async()  # reads B: the image is fixed when the call is made
        c.stage_trace(*A, b)  # fills the other image while that proof may be in flight
        assert bytes(c.wait_view()) == pb
        art = c.prove()
        assert (art.manifest_root, art.proof_bytes) == (ra, pa)
        assert c.manifest_leaves() == wa.leaf_hashes()
        # another block size is another shape
        with pytest.raises(product.SezkpError) as e:
            c.stage_trace(*A, 256)
        assert e.value.code == -1
        assert c.prove().proof_bytes == pa
        # a block view staged on the trace context: proves with its root, has no root of its own
        c.stage(wb)
        assert c.prove(rb).proof_bytes == pb
        with pytest.raises(product.SezkpError) as e:
            c.prove()
        assert e.value.code == -1 and FROM_BLOCKS_MSG in str(e.value)
        with pytest.raises(product.SezkpError, match="uploaded as blocks"):
            c.manifest_root()
        # and a trace staged behind it again
        c.stage_trace(*A, b)
        assert c.prove().proof_bytes == pa
    finally:
        c.close()


def test_trace_staged_on_a_block_context(gpu_ok, product, oracle):
    t, tau, b = 4096, 3, 333
    wa, wb = want_blocks(t, tau, b, "random"), want_blocks(t, tau, b, "plus")
    c = product.ProverContext(0)
    try:
        c.upload(wa)
        c.stage_trace(*make_trace(t, tau, b, "plus"), b)
        art = c.prove()
        assert art.manifest_root == wb.manifest_root()
        assert art.proof_bytes == want_proof(t, tau, b, "plus", art.manifest_root)
        assert_blocks_equal(product, c.blocks(), wb)
    finally:
        c.close()


def test_staged_trace_with_host_hashed_leaves(gpu_ok, product, oracle):
    """41 tapes: the leaf message leaves one BLAKE3 chunk and the host hashes
    the leaves, also for a staged image."""
    t, tau, b = 1024, 41, 256
    w = want_blocks(t, tau, b, "alt127")
    c = product.ProverContext(0)
    try:
        c.upload_trace(*make_trace(t, tau, b, "random"), b)
        c.stage_trace(*make_trace(t, tau, b, "alt127"), b)
        art = c.prove()
        assert art.manifest_root == w.manifest_root()
        assert art.proof_bytes == want_proof(t, tau, b, "alt127", art.manifest_root)
    finally:
        c.close()


# ------------------------------------------------------------ device input
def test_trace_given_as_device_tensors(gpu_ok, product, oracle):
    torch = gpu_ok
    t, tau, b = 4096, 8, 512
    imv, mv, hw, ws = make_trace(t, tau, b, "random")
    want = want_blocks(t, tau, b, "random")
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (imv, mv, hw, ws.view(np.int16))]
    c = product.ProverContext(0)
    try:
        c.upload_trace(*dev, b)
        assert_blocks_equal(product, c.blocks(), want)
        art = c.prove()
        assert art.manifest_root == want.manifest_root()
        assert art.proof_bytes == want_proof(t, tau, b, "random", art.manifest_root)
        dev2 = [torch.from_numpy(np.array(a)).cuda()
                for a in (lambda tr: (tr[0], tr[1], tr[2], tr[3].view(np.int16)))(make_trace(t, tau, b, "alt127"))]
        c.stage_trace(*dev2, b)
        w2 = want_blocks(t, tau, b, "alt127")
        art = c.prove()
        assert art.manifest_root == w2.manifest_root()
        assert art.proof_bytes == want_proof(t, tau, b, "alt127", art.manifest_root)
        with pytest.raises(product.SezkpError, match="contiguous"):
            c.upload_trace(dev[0], dev[1].t().contiguous().t(), dev[2], dev[3], b)
    finally:
        c.close()


# ------------------------------------------------------------ neighbours
def test_air_audit_and_batch_verify_accept_trace_uploads(ctx, product):
    t, tau, b = 4096, 8, 512
    ctx.upload_trace(*make_trace(t, tau, b, "clean"), b)
    audit = ctx.air_audit()
    assert audit.ok and audit.families["boundary"]["cells"] == 0 and audit.n_rows == t
    arts = [ctx.prove(), ctx.prove(bytes(range(32)))]
    res = ctx.verify_batch(arts, [a.manifest_root for a in arts], [tau, tau])
    assert [r.ok for r in res] == [True, True], res
    res = ctx.verify_batch([arts[0]], [arts[1].manifest_root], [tau])
    assert not res[0].ok and "manifest root mismatch" in res[0].message


def test_head_outside_i32_fails_the_upload_and_the_next_one_works(gpu_ok, product):
    """One block of 2^25 rows moving +127 a row (test_gpu_parity.py's head-guard
    shape; at 2^24 rows the head stays below 2^31 and the trace is accepted):
    upload_trace fails with prove's message and leaves the context usable."""
    T = 1 << 25
    imv = np.zeros(T, np.int8)
    hw = np.zeros((T, 1), np.uint8)
    ws = np.zeros((T, 1), np.uint16)
    c = product.ProverContext(0)
    try:
        with pytest.raises(product.SezkpError, match="i32 range") as e:
            c.upload_trace(imv, np.full((T, 1), 127, np.int8), hw, ws, T)
        assert e.value.code == -1
        with pytest.raises(product.SezkpError, match="no trace uploaded"):
            c.prove()
        c.upload_trace(imv, np.ones((T, 1), np.int8), hw, ws, T)
        got = c.blocks()
        assert (int(got.win_left[0]), int(got.win_right[0]), int(got.off_out[0])) == (0, T, T)
        assert len(c.prove().proof_bytes) > 0
    finally:
        c.close()


def test_sharded_context_refuses_a_raw_trace(gpu_ok, product):
    c = product.ShardedProverContext(0, 1, 0, comm="solo")
    try:
        with pytest.raises(product.SezkpError, match="sharded") as e:
            c.upload_trace(*make_trace(4096, 8, 512, "random"), 512)
        assert e.value.code == -1
    finally:
        c.close()
