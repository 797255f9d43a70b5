#!/usr/bin/env python3
"""A raw trace against its blocks on sharded contexts: first and warm proofs.

P ranks on ONE GPU over host collectives (gloo), as the tests run them; the
figures in profiles/sharded_trace/README.md come from here.

    python tools/sharded_trace_probe.py --world 2 --log-t 21 --out DIR
    python tools/sharded_trace_probe.py --solo trace --world 2 --log-t 21   # one rank alone, for a kernel trace

Per repetition, alternating the two paths on the same trace (simulate(t, tau,
seed) and its partition): upload, the first proof of the image (host clock
around prove(), which ends in a device synchronise; a barrier before it), its
comm_stats, then `--warm` warm proofs. Both paths must give the same bytes.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "streaming-zero-knowledge-proofs_amd"), os.path.join(ROOT, "tests")]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def worker(rank, world, port, args, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import sezkp_amd
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        t = 1 << args.log_t
        tr = sezkp_amd.simulate(t, args.tau, args.seed)
        blocks, part_ms = timed(lambda: sezkp_amd.partition(*tr, args.b))
        root, root_ms = timed(blocks.manifest_root)
        row0, nrows = sezkp_amd.trace_shard_rows(t, args.b, rank, world)
        sl = tuple(a[row0:row0 + nrows] for a in tr)
        ctxs = {p: sezkp_amd.ShardedProverContext(rank, world, device=0, comm="host") for p in ("trace", "blocks")}
        out = {"rank": rank, "host_partition_ms": part_ms, "host_manifest_root_ms": root_ms, "rows": nrows, "reps": []}
        for rep in range(args.reps):
            rec = {}
            for path in ("trace", "blocks") if rep % 2 == 0 else ("blocks", "trace"):
                c = ctxs[path]
                dist.barrier()
                if path == "trace":
                    _, up = timed(lambda: c.upload_trace_rows(*sl, args.b, t, row0))
                else:
                    _, up = timed(lambda: c.upload(blocks))
                dist.barrier()
                art, first = timed(lambda: c.prove(None if path == "trace" else root))
                stats = c.comm_stats()
                warm = []
                for _ in range(args.warm):
                    dist.barrier()
                    a2, ms = timed(lambda: c.prove(None if path == "trace" else root))
                    warm.append(ms)
                    assert a2.proof_bytes == art.proof_bytes
                rec[path] = {"upload_ms": up, "first_ms": first, "warm_ms": warm,
                             "first_comm": [{k: s[k] for k in ("name", "bytes", "ms")} for s in stats],
                             "warm_comm_names": [s["name"] for s in c.comm_stats()],
                             "digest": hashlib.sha256(art.proof_bytes).hexdigest(), "root": art.manifest_root.hex()}
            assert rec["trace"]["digest"] == rec["blocks"]["digest"] and rec["trace"]["root"] == root.hex()
            out["reps"].append(rec)
        for c in ctxs.values():
            c.close()
        q.put(out)
    except Exception as e:  # report, do not hang the parent
        import traceback
        traceback.print_exc()
        q.put({"rank": rank, "error": f"{type(e).__name__}: {e}"})
    finally:
        dist.destroy_process_group()


def solo(args):
    """Rank 0 of `world` alone (sezkp_ctx_create_sharded_solo), one path: an
    upload, the first proof and `--warm` warm ones, for rocprofv3 --kernel-trace."""
    import sezkp_amd
    t = 1 << args.log_t
    tr = sezkp_amd.simulate(t, args.tau, args.seed)
    c = sezkp_amd.ShardedProverContext(0, args.world, device=0, comm="solo")
    if args.solo == "trace":
        c.upload_trace(*tr, args.b)
        root = None
    else:
        blocks = sezkp_amd.partition(*tr, args.b)
        root = blocks.manifest_root()
        c.upload(blocks)
    names = []
    for _ in range(1 + args.warm):
        c.prove(root)
        names.append([s["name"] for s in c.comm_stats()])
    c.close()
    print(json.dumps({"path": args.solo, "proofs": 1 + args.warm, "comm_names": names}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--log-t", type=int, default=21)
    ap.add_argument("--b", type=int, default=512)
    ap.add_argument("--tau", type=int, default=8)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--solo", choices=["trace", "blocks"])
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.solo:
        return solo(args)
    import torch.multiprocessing as mp
    from conftest import free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    ps = [ctx.Process(target=worker, args=(r, args.world, port, args, q)) for r in range(args.world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=900) for _ in ps), key=lambda o: o["rank"])
    for p in ps:
        p.join(timeout=60)
    bad = [o for o in res if "error" in o]
    doc = {"world": args.world, "t": 1 << args.log_t, "tau": args.tau, "b": args.b, "ranks": res}
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"probe_p{args.world}.json"), "w") as f:
            json.dump(doc, f, indent=1)
    if bad:
        print(bad)
        sys.exit(1)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for o in res:
        for path in ("trace", "blocks"):
            first = [r[path]["first_ms"] for r in o["reps"]]
            warm = [m for r in o["reps"] for m in r[path]["warm_ms"]]
            print(f"rank {o['rank']} {path:6s} first {med(first):8.2f} ms (min {min(first):.2f} max {max(first):.2f})  "
                  f"warm {med(warm):8.2f} ms (min {min(warm):.2f} max {max(warm):.2f})")
    r0 = res[0]["reps"][0]
    print("trace  first comm:", [(s["name"], s["bytes"], round(s["ms"], 3)) for s in r0["trace"]["first_comm"][:3]])
    print("trace  warm names:", r0["trace"]["warm_comm_names"])
    print("blocks warm names:", r0["blocks"]["warm_comm_names"])


if __name__ == "__main__":
    main()
