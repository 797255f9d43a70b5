"""Trace image to blocks file: the host encoder against the device encoder.

At the headline shape (T = 2^21, tau = 8, b = 512 by default) the trace
reference_trace(T, tau, 42) is uploaded (upload_trace) and proved once, and one
process runs, after one warm-up round that is dropped, ROUNDS alternating
rounds of

  (a) host     ctx.blocks().to_cbor(): the readback of every step array
               (sezkp_ctx_trace_blocks) and sezkp_blocks_encode_cbor, what
               `prove --trace --out-blocks` did before; and its two parts;
  (b) device   ctx.blocks_cbor(): the whole call on the host clock, and the
               stats' ms_kernels / ms_d2h split;
  (d) trace    ctx.trace_cbor() of the image against Trace.to_cbor() of the
               host arrays (sezkp_trace_encode_cbor alone).

Then (c): the same trace in blocks of --small-b steps (default 8), device arm
every round, the host arm three rounds. Every round compares the files of the
two arms byte for byte; a prove before the first and after the last round
must give the same bytes.

Every device arm ends in the call's own stream synchronisation. Reported per
arm: median, min, max in ms. One JSON object on stdout and in --out (default
profiles/cbor_encode/probe.json), written before (c) starts and again after.
The device encoder is the CLI's default when (b)'s median lies below (a)'s
minimum.

    python tools/cbor_encode_probe.py [--log-t 21] [--tau 8] [--b 512] [--small-b 8] [--rounds 10] [--out FILE]

The per-kernel times come from a run of their own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/cbor_encode_probe.py --kernels
    python tools/cbor_encode_probe.py --report DIR
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "streaming-zero-knowledge-proofs_amd"))


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def report(d):
    import collections
    import csv
    import glob
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    agg = collections.defaultdict(list)
    for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if "k_cbor" in name:
            agg[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, v in sorted(agg.items()):
        print(f"{k}: {len(v)} launches, us each {[round(x, 1) for x in v]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true",
                    help="three blocks_cbor at --b, three at --small-b, three trace_cbor (for a kernel trace)")
    ap.add_argument("--report", metavar="DIR", help="summarise the kernel_trace.csv under DIR")
    ap.add_argument("--log-t", type=int, default=21)
    ap.add_argument("--tau", type=int, default=8)
    ap.add_argument("--b", type=int, default=512)
    ap.add_argument("--small-b", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cbor_encode", "probe.json"))
    args = ap.parse_args()
    if args.report:
        return report(args.report)
    import torch
    import sezkp_amd as P
    assert torch.cuda.is_available(), "needs a HIP device"
    t = 1 << args.log_t
    out = {"t": t, "tau": args.tau, "rounds": args.rounds}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")

    tr = P.reference_trace(t, args.tau, 42)
    ctx = P.ProverContext(0)
    if args.kernels:
        for b in (args.b, args.small_b):
            ctx.upload_trace(*tr, b)
            for _ in range(3):
                ctx.blocks_cbor()
        for _ in range(3):
            ctx.trace_cbor()
        ctx.close()
        print("ok")
        return

    def shape(b, rounds_host):
        ctx.upload_trace(*tr, b)
        proof = ctx.prove().proof_bytes
        arms = {k: [] for k in ("a_host_blocks_to_cbor", "a_readback_trace_blocks", "a_encode_blocks_cbor",
                                "b_device_blocks_cbor", "b_ms_kernels", "b_ms_d2h")}
        size = 0
        for r in range(args.rounds + 1):  # round 0 warms every arm (allocations, first launches) and is dropped
            want = None
            if r <= rounds_host:
                d_rb, blocks = ms(ctx.blocks)
                d_enc, want = ms(blocks.to_cbor)
                del blocks
            d_dev, got = ms(ctx.blocks_cbor)
            st = ctx.encode_stats()
            assert st["path"] == "device", st
            assert want is None or got == want, "the two encoders wrote different files"
            size = len(got)
            del got
            if r == 0:
                continue
            if want is not None:
                for k, v in (("a_host_blocks_to_cbor", d_rb + d_enc), ("a_readback_trace_blocks", d_rb),
                             ("a_encode_blocks_cbor", d_enc)):
                    arms[k].append(v)
            for k, v in (("b_device_blocks_cbor", d_dev), ("b_ms_kernels", st["ms_kernels"]), ("b_ms_d2h", st["ms_d2h"])):
                arms[k].append(v)
        assert ctx.prove().proof_bytes == proof, "a proof after the encodes differs from the one before"
        return {"b": b, "n_blocks": -(-t // b), "bytes": size, "arms": {k: summary(v) for k, v in arms.items()}}

    # ---------------------------------------------------------------- headline: (a), (b)
    out["headline"] = shape(args.b, args.rounds)
    a = out["headline"]["arms"]
    out["headline"]["device_is_the_cli_default"] = (a["b_device_blocks_cbor"]["median_ms"] <
                                                    a["a_host_blocks_to_cbor"]["min_ms"])
    print(json.dumps(out["headline"]), flush=True)
    write()
    # ---------------------------------------------------------------- (d): the trace file of the same image
    host_trace = P.Trace(*tr)
    arms = {k: [] for k in ("d_host_trace_to_cbor", "d_device_trace_cbor", "d_ms_kernels", "d_ms_d2h")}
    for r in range(args.rounds + 1):
        d_host, want = ms(host_trace.to_cbor)
        d_dev, got = ms(ctx.trace_cbor)
        st = ctx.encode_stats()
        assert st["path"] == "device" and got == want, st
        size = len(got)
        del got, want
        if r:
            for k, v in (("d_host_trace_to_cbor", d_host), ("d_device_trace_cbor", d_dev),
                         ("d_ms_kernels", st["ms_kernels"]), ("d_ms_d2h", st["ms_d2h"])):
                arms[k].append(v)
    out["trace_file"] = {"bytes": size, "arms": {k: summary(v) for k, v in arms.items()}}
    print(json.dumps(out["trace_file"]), flush=True)
    write()
    # ---------------------------------------------------------------- (c): small blocks
    out["small_blocks"] = shape(args.small_b, 3)  # the host arm is slow here: three timed rounds
    write()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
