#!/usr/bin/env python3
"""trace -> proof for a stream of distinct traces: the host partition path
against the device partition path, in one run on one GPU.

Headline shape by default (T = 2^21, tau = 8, b = 512, seeds 42..47), K = 3
contexts in flight as bench.py runs them (one host thread per context; every
proof stages its own trace while the context's previous proof runs).

  path (a), blocks:  partition_trace and manifest_root on the host, then
                     stage(blocks) + prove(root)
  path (b), trace:   stage_trace(arrays) + prove() with the root from the trace

The host steps are timed on their own, on one thread (the generator is not
part of either path: a user holds the movement log already). partition_trace
has no entry point of its own, so its time is sezkp_simulate_blocks (generator
+ partition) minus sezkp_simulate_trace (generator), each the median of
`--host-reps` calls. The device part of (a) is measured with prebuilt blocks
and roots; (a) per proof is then bracketed by "host steps on the context's
thread, not overlapped" (device + partition + root) and "host steps spread
perfectly over the K threads" (max(device, (partition + root) / K)).

The default `--mode both` times the host steps, checks that both paths give
the same proof bytes, and then times each pipeline in a child process of its
own (`--mode blocks` / `--mode trace`), the two alternating `--repeats` times:
a context's streams take the device's hardware queues in creation order, so
two sets of contexts in one process do not run on the same queue layout.
`--mode blocks` alone is what a block-uploaded context pays per proof; with
`--pkg DIR` it loads sezkp_amd from DIR, so the same command times another
build of the library (the parent commit's) for the run-to-run spread. Prints
one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time


def pipeline(ctxs, stage, prove, proofs):
    """K threads, one per context: stage the next trace, start the proof,
    stage the one after while it runs, wait. Returns wall seconds."""
    K = len(ctxs)
    lock = threading.Lock()
    left = [proofs]
    errs = []
    go = threading.Barrier(K + 1)

    def take():
        with lock:
            if left[0] == 0:
                return -1
            left[0] -= 1
            return left[0]

    def run(i):
        try:
            go.wait()
            j = take()
            if j >= 0:
                stage(ctxs[i], i, j)
            while j >= 0:
                prove(ctxs[i], i, j)
                nxt = take()
                if nxt >= 0:
                    stage(ctxs[i], i, nxt)
                ctxs[i].wait_view()
                j = nxt
        except Exception as e:  # reported below
            errs.append(e)
            with lock:
                left[0] = 0

    ths = [threading.Thread(target=run, args=(i,)) for i in range(K)]
    for t in ths:
        t.start()
    t0 = time.perf_counter()
    go.wait()
    for t in ths:
        t.join()
    t1 = time.perf_counter()
    if errs:
        raise errs[0]
    return t1 - t0


def median_time(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-t", type=int, default=21)
    ap.add_argument("--tau", type=int, default=8)
    ap.add_argument("--b", type=int, default=512)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--proofs", type=int, default=240, help="proofs per timed window")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per path, alternated")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--mode", choices=["both", "blocks", "trace"], default="both")
    ap.add_argument("--pkg", default=None, help="directory holding the sezkp_amd package to load")
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, args.pkg or os.path.join(root_dir, "streaming-zero-knowledge-proofs_amd"))
    import torch
    if not torch.cuda.is_available():
        sys.exit("trace_probe needs a HIP device")
    import numpy as np
    import sezkp_amd as S
    lib = S.lib

    T, tau, b, K = 1 << args.log_t, args.tau, args.b, args.inflight
    seeds = list(range(42, 42 + 2 * K))
    traces = [S.reference_trace(T, tau, s) for s in seeds]
    for tr in traces:  # page-locked, as bench.py pins its block arrays: the staging copies are DMA
        for a in tr:
            lib.sezkp_host_register(a.ctypes.data, a.nbytes)
    blocks = [S.partition(*tr, b) for tr in traces] if args.log_t <= 16 else [S.reference_blocks(T, b, tau, s) for s in seeds]
    for bl in blocks:
        bl.pin()
    roots = [bl.manifest_root() for bl in blocks]
    out = {"label": args.label, "T": T, "tau": tau, "b": b, "inflight": K, "proofs_per_window": args.proofs,
           "distinct_traces": len(seeds), "version": lib.sezkp_version().decode()}

    # ---- host steps, one thread
    if args.mode == "both":
        im, mv = np.zeros(T, np.int8), np.zeros((T, tau), np.int8)
        hw, ws = np.zeros((T, tau), np.uint8), np.zeros((T, tau), np.uint16)
        gen = median_time(lambda: lib.sezkp_simulate_trace(T, tau, 42, im.ctypes.data, mv.ctypes.data, hw.ctypes.data,
                                                           ws.ctypes.data), args.host_reps)

        def gen_part():
            h = C.c_void_p()
            err = C.create_string_buffer(256)
            assert lib.sezkp_simulate_blocks(T, b, tau, 42, C.byref(h), err, 256) == 0
            lib.sezkp_blocks_free(h)
        both = median_time(gen_part, args.host_reps)
        mroot = median_time(lambda: blocks[0].manifest_root(), max(3, args.host_reps))
        out["host_ms"] = {"generator": 1e3 * gen[0], "generator_plus_partition": 1e3 * both[0],
                          "partition": 1e3 * (both[0] - gen[0]), "manifest_root": 1e3 * mroot[0],
                          "generator_min_max": [1e3 * gen[1], 1e3 * gen[2]],
                          "generator_plus_partition_min_max": [1e3 * both[1], 1e3 * both[2]]}

    # ---- the two pipelines
    # (streams take the device's hardware queues round-robin in creation
    # order, so the second set of contexts of `--mode both` sits on another
    # queue layout than the first: `--mode blocks` and `--mode trace` time one
    # set each, in a process of its own)
    paths = {}
    if args.mode != "trace":
        ctxs_a = [S.ProverContext(0) for _ in range(K)]
        for i, c in enumerate(ctxs_a):
            c.upload(blocks[i])

        def stage_a(c, i, j):
            c.stage(blocks[(i + K * (j % 2)) % len(blocks)])

        def prove_a(c, i, j):
            c.prove_async(roots[(i + K * (j % 2)) % len(blocks)])
        paths["blocks"] = (ctxs_a, stage_a, prove_a)
    if args.mode != "blocks":
        ctxs_b = [S.ProverContext(0) for _ in range(K)]
        for i, c in enumerate(ctxs_b):
            c.upload_trace(*traces[i], b)
            assert c.manifest_root() == roots[i]

        def stage_b(c, i, j):
            c.stage_trace(*traces[(i + K * (j % 2)) % len(traces)], b)

        def prove_b(c, i, j):
            c.prove_async()
        paths["trace"] = (ctxs_b, stage_b, prove_b)
        # same bytes on both paths before anything is timed
        for i in range(K if args.mode == "both" else 0):
            pa = bytes(ctxs_a[i].prove_view(roots[i]))
            assert bytes(ctxs_b[i].prove_view()) == pa, "trace and block uploads disagree"
    per = {name: [] for name in paths}
    if args.mode == "both":
        # the bytes agree; now each path in a process of its own (one set of
        # contexts, the same queue layout for both), the paths alternating:
        # measured with both sets alive in one process, the set created second
        # ran 0.13 ms per proof slower, whichever path it held
        for cs, _, _ in paths.values():
            for c in cs:
                c.close()
        import subprocess
        for _ in range(args.repeats):
            for name in paths:
                cmd = [sys.executable, os.path.abspath(__file__), "--mode", name, "--repeats", "1", "--log-t",
                       str(args.log_t), "--tau", str(tau), "--b", str(b), "--inflight", str(K), "--proofs",
                       str(args.proofs), "--warmup", str(args.warmup)] + (["--pkg", args.pkg] if args.pkg else [])
                r = subprocess.run(cmd, capture_output=True, text=True, check=True)
                per[name] += json.loads(r.stdout.strip().splitlines()[-1])["ms_per_proof"][name]["all"]
        paths = {}
    else:
        for name, (cs, st, pr) in paths.items():
            pipeline(cs, st, pr, args.warmup)
        for _ in range(args.repeats):
            for name, (cs, st, pr) in paths.items():
                per[name].append(1e3 * pipeline(cs, st, pr, args.proofs) / args.proofs)
        st = next(iter(paths.values()))[0][0].stage_times_ms()
        out["context_host_ms"] = {k: st[k] for k in ("host_wall", "host_sync_wait", "host_final_wait", "host_serialize")
                                  if k in st}
    out["ms_per_proof"] = {name: {"median": statistics.median(v), "all": v} for name, v in per.items()}
    if args.mode == "both":
        dev_a = out["ms_per_proof"]["blocks"]["median"]
        host = out["host_ms"]["partition"] + out["host_ms"]["manifest_root"]
        out["path_a_ms_per_proof"] = {"host_steps_not_overlapped": dev_a + host,
                                      "host_steps_spread_over_threads": max(dev_a, host / K)}
        out["path_b_ms_per_proof"] = out["ms_per_proof"]["trace"]["median"]
        out["elements_per_s"] = {"path_b": T * tau / (1e-3 * out["path_b_ms_per_proof"]),
                                 "path_a_best_case": T * tau / (1e-3 * out["path_a_ms_per_proof"]["host_steps_spread_over_threads"])}
    for cs, _, _ in paths.values():
        for c in cs:
            c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
