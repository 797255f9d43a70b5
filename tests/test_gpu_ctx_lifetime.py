"""One context through everything it owns: the upload workspace, the
dictionary tables and head ladders, the audit and the verify buffers, both
trace images and the trace metadata are allocated, reused, regrown and
released in one sequence, then a second context in the same process proves
again. Every proof is the oracle's, byte for byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, TAU, BLK = 4096, 2, 256


def random_trace(t, tau, seed):
    """Heads that never go below 0 and symbols below 16: the AIR holds on every row."""
    rng = np.random.Generator(np.random.PCG64(seed))
    hw = (rng.random((t, tau)) < 0.4).astype(np.uint8)
    ws = (rng.integers(0, 16, size=(t, tau), dtype=np.uint16) * hw).astype(np.uint16)
    imv = rng.integers(-1, 2, size=t, dtype=np.int8)
    mv = np.ascontiguousarray(rng.integers(0, 2, size=(t, tau), dtype=np.int8))
    return imv, mv, hw, ws


def test_one_context_through_every_owner(gpu_ok, product, oracle):
    tr = random_trace(N, TAU, 11)
    blocks = product.partition(*tr, BLK)
    root = blocks.manifest_root()
    want = oracle.prove_v1(blocks, root)
    blocks2 = product.partition(*random_trace(N, TAU, 12), BLK)
    root2 = blocks2.manifest_root()
    small = product.synthetic_blocks(1024, BLK, TAU, 13)
    small_root = small.manifest_root()

    ctx = product.ProverContext(0)
    try:
        # 1. upload blocks, then prove
        ctx.upload(blocks)
        first = ctx.prove(root)
        assert first.proof_bytes == want
        # 2. the audit's buffers
        audit = ctx.air_audit(bitmaps=True)
        assert (audit.n_rows, audit.tau, audit.rows_violating, audit.rows_rejectable) == (N, TAU, 0, 0)
        # 3. the verify buffers
        verdicts = ctx.verify_batch([first], [root], [TAU])
        assert [(v.ok, v.code) for v in verdicts] == [(True, 0)]
        # 4. the same movement log as a raw trace: the device's partition and root
        ctx.upload_trace(*tr, BLK)
        from_trace = ctx.prove()
        assert from_trace.manifest_root == root
        assert from_trace.proof_bytes == want
        # 5. the spare trace image
        ctx.stage(blocks2)
        assert ctx.prove(root2).proof_bytes == oracle.prove_v1(blocks2, root2)
        # 6. another shape: the workspace regrows, the audit's device buffer goes
        ctx.upload(small)
        assert ctx.prove(small_root).proof_bytes == oracle.prove_v1(small, small_root)
    finally:
        # 7. every owner released, then the streams
        ctx.close()

    again = product.ProverContext(0)
    try:
        again.upload(blocks)
        assert again.prove(root).proof_bytes == want
    finally:
        again.close()
