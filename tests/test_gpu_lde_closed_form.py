"""The closed-form first stages of the DEEP-polynomial LDE (DeepPoly,
csrc/sezkp_internal.h) on the GPU: whole proofs, byte for byte.

Three arms give the same proof: the closed-form group load (the default), the
point-by-point load (SEZKP_DP_CLOSED=0) and the per-point DEEP division
(SEZKP_NO_DEEP_POLY=1); all equal the C oracle. `lde_closed_stages()` says
which load the last prove's first LDE pass took, so an arm that silently took
the other load fails.

Single device: T = 2^10 (N = 2^13, passes [7, 6]: k_ntt4<.., 4, 3, ..>) and
T = 2^13 (N = 2^16, passes [8, 8]: the headline's k_ntt4<.., 4, 4, ..>), b = 3,
eight seeds each: eight different z, rho, c' and kappa.

Sharded through the host collectives of tests/test_gpu_sharded.py, with the
replicated and the distributed INTT (SEZKP_DIST_INTT=1, whose allgathered
coefficient layout the group load reads through src_slot). A sharded proof
needs n >= 4096 P rows, so each P runs at its smallest legal trace:
  P = 2, T = 2^13: every rank evaluates the whole domain (full_lde), b = 3,
                   passes [8, 8];
  P = 4, T = 2^14: E = 2^15 points per rank from n = 2^14, b = 1, passes [8, 7],
                   the rank's coset factor in rho and in qv;
  P = 8, T = 2^15: E = n, b = 0: no stage to close, the point-by-point load.
(b = 2 needs a rank that evaluates N/2 points; no sharding of this prover
does. Its code is the template the other two instantiate; the CPU model in
test_lde_closed_form_host.py covers its algebra.)
"""
import hashlib
import os
import sys

import pytest

from conftest import ORACLE, PKG, free_port

pytestmark = pytest.mark.gpu

TAU, B = 8, 64
SEEDS = [1, 2, 3, 5, 8, 13, 21, 34]


@pytest.mark.parametrize("T", [1 << 10, 1 << 13])
def test_three_arms_byte_equal_single_device(gpu_ok, product, oracle, monkeypatch, T):
    ctx = product.ProverContext(0)
    try:
        for seed in SEEDS:
            blocks = product.synthetic_blocks(T, B, TAU, seed)
            root = blocks.manifest_root()
            want = oracle.prove_v1(blocks, root)
            ctx.upload(blocks)
            assert ctx.lde_closed_stages() == 0  # no prove of this upload yet
            monkeypatch.delenv("SEZKP_DP_CLOSED", raising=False)
            monkeypatch.delenv("SEZKP_NO_DEEP_POLY", raising=False)
            closed = ctx.prove(root).proof_bytes
            assert ctx.lde_closed_stages() == 3, (T, seed)
            monkeypatch.setenv("SEZKP_DP_CLOSED", "0")
            pointwise = ctx.prove(root).proof_bytes
            assert ctx.lde_closed_stages() == 0, (T, seed)
            monkeypatch.delenv("SEZKP_DP_CLOSED")
            monkeypatch.setenv("SEZKP_NO_DEEP_POLY", "1")
            division = ctx.prove(root).proof_bytes
            assert ctx.lde_closed_stages() == 0, (T, seed)
            assert closed == want, (T, seed)
            assert pointwise == want, (T, seed)
            assert division == want, (T, seed)
    finally:
        ctx.close()


ARMS = [("closed", {}), ("pointwise", {"SEZKP_DP_CLOSED": "0"}),
        ("closed+dist_intt", {"SEZKP_DIST_INTT": "1"}),
        ("pointwise+dist_intt", {"SEZKP_DP_CLOSED": "0", "SEZKP_DIST_INTT": "1"})]


def _worker(rank, world, port, T, seed, q):
    sys.path[:0] = [PKG, ORACLE]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sezkp_amd
        blocks = sezkp_amd.synthetic_blocks(T, B, TAU, seed)
        ctx = sezkp_amd.ShardedProverContext(rank, world, device=0, comm="host")
        ctx.upload(blocks)
        root = blocks.manifest_root()
        out = []
        for name, env in ARMS:  # both switches are read per prove
            for k in ("SEZKP_DP_CLOSED", "SEZKP_DIST_INTT"):
                os.environ.pop(k, None)
            os.environ.update(env)
            p = ctx.prove(root).proof_bytes
            out.append((name, hashlib.sha256(p).hexdigest(), ctx.lde_closed_stages()))
        ctx.close()
        q.put((rank, out))
    except Exception as e:
        q.put((rank, f"ERR {type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,T,seed,stages", [(2, 1 << 13, 4, 3), (4, 1 << 14, 6, 1), (8, 1 << 15, 9, 0)])
def test_sharded_arms_equal_single_device(gpu_ok, product, oracle, world, T, seed, stages):
    blocks = product.synthetic_blocks(T, B, TAU, seed)
    root = blocks.manifest_root()
    single = product.StarkV1.prove(blocks, root).proof_bytes
    assert single == oracle.prove_v1(blocks, root)
    want = hashlib.sha256(single).hexdigest()
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = free_port()
    ps = [mpc.Process(target=_worker, args=(r, world, port, T, seed, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=600) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    assert [r for r, _ in res] == list(range(world))
    for rank, out in res:
        assert not isinstance(out, str), (rank, out)
        assert [name for name, _, _ in out] == [name for name, _ in ARMS]
        for name, digest, got in out:
            assert digest == want, (rank, name)
            assert got == (stages if name.startswith("closed") else 0), (rank, name, got)
