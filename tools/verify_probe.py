"""Batch verification on the GPU against the host verifier, on the headline
proof (T = 2^21, tau = 8, seeds 42..47), at batch sizes 1, 8 and 64.

Two arms per repetition, alternating, after a warm-up of both:
  host   sezkp_stark_v1_verify on one thread over the batch's proofs (the
         yardstick: the function computes what it did before the batch
         verifier existed), wall clock per proof;
  batch  one sezkp_ctx_verify_batch call, wall clock per proof, and its split
         from sezkp_ctx_verify_times: host parse + job building, packing the
         pinned block, the H2D copy, the kernel and the result readback (HIP
         events on the context's stream), the checks.
Medians over the repetitions; the verdicts of the two arms are compared on
every repetition.
  python3 tools/verify_probe.py [log_t] [tau] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "streaming-zero-knowledge-proofs_amd"))

import torch  # noqa: E402

import sezkp_amd  # noqa: E402
from sezkp_amd._lib import VERIFY_TIMES, BlockView, ProofRef, VerifyResultC, lib  # noqa: E402


def main():
    log_t = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    tau = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    out = sys.argv[3] if len(sys.argv) > 3 else None
    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = sezkp_amd.ProverContext(0)
    proofs, roots = [], []
    for seed in range(42, 48):
        blocks = sezkp_amd.reference_blocks(1 << log_t, 512, tau, seed)
        root = blocks.manifest_root()
        ctx.upload(blocks)
        proofs.append(ctx.prove(root).proof_bytes)
        roots.append(root)
        del blocks
    view = BlockView()
    view.n_blocks, view.tau = 1, tau
    bufs = [C.create_string_buffer(p, len(p)) for p in proofs]
    rbufs = [C.create_string_buffer(r, 32) for r in roots]
    err = C.create_string_buffer(1024)

    def host_arm(n):
        verdicts = []
        t0 = time.perf_counter()
        for i in range(n):
            k = i % len(proofs)
            rc = lib.sezkp_stark_v1_verify(C.cast(bufs[k], C.c_char_p), len(proofs[k]), C.byref(view), roots[k], err, 1024)
            verdicts.append((rc, err.value if rc else b""))
        return (time.perf_counter() - t0) * 1e3 / n, verdicts

    def batch_arm(n, refs, res):
        t0 = time.perf_counter()
        rc = lib.sezkp_ctx_verify_batch(ctx._h, refs, n, res, err, 1024)
        ms = (time.perf_counter() - t0) * 1e3 / n
        assert rc == 0, err.value
        return ms, [(r.code, r.msg) for r in res], ctx.verify_times()

    med = statistics.median
    result = {"trace": f"reference_blocks(1 << {log_t}, 512, {tau}, seed), seeds 42..47",
              "proof_bytes": [len(p) for p in proofs], "batches": {}}
    for n, reps in ((1, 30), (8, 15), (64, 8)):
        refs, res = (ProofRef * n)(), (VerifyResultC * n)()
        for i in range(n):
            k = i % len(proofs)
            refs[i].bytes, refs[i].len = C.addressof(bufs[k]), len(proofs[k])
            refs[i].manifest_root, refs[i].tau = C.addressof(rbufs[k]), tau
        for _ in range(3):  # warm-up: code objects, the staging buffers at this batch size
            batch_arm(n, refs, res)
        host_arm(n)
        host, rows = [], []
        for _ in range(reps):
            ms, want = host_arm(n)
            host.append(ms)
            ms, got, t = batch_arm(n, refs, res)
            assert got == want, (got, want)
            rows.append((ms, t))
        wall = [ms for ms, _ in rows]
        split = {k: med([t[k] for _, t in rows]) / n for k in VERIFY_TIMES if k.endswith("_ms")}
        result["batches"][str(n)] = {
            "reps": reps, "verdicts": sorted({f"{rc}:{m.decode()}" for rc, m in want}),
            "host_ms_per_proof": {"median": med(host), "min": min(host), "max": max(host)},
            "batch_ms_per_proof": {"median": med(wall), "min": min(wall), "max": max(wall)},
            "split_ms_per_proof_median": split, "jobs": rows[0][1]["jobs"], "slices": rows[0][1]["slices"],
            "host_over_batch": med(host) / med(wall)}
    ctx.close()
    print(json.dumps(result))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
