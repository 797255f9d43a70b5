"""Block file to trace image: the host decoder against the device decoder.

At the headline shape (T = 2^21, tau = 8, b = 512 by default) on
reference_blocks(T, b, tau, 42).to_cbor(), one process runs, after one warm-up
round that is dropped, ROUNDS rounds of

  host      BlockSoA.from_cbor (sezkp_blocks_decode_cbor and the copies into
            numpy arrays), and the C call alone: the yardstick;
  upload    ProverContext.upload of those blocks (what follows the host decoder);
  device    ProverContext.upload_blocks_cbor from pageable bytes: the whole
            call on the host clock, and the stats' ms_h2d / ms_decode split;
  pinned    the same from page-locked bytes;
  sibling   upload_trace_cbor of the same trace (Trace.to_cbor of the blocks'
            step arrays), the TraceFile decoder at the same shape.

Then the small-block shape (--small-b, default 8: B = T / 8 blocks, one lane
per block for head and tail): `ingest_blocks_cbor` (decode and tables home) per
round, the host decoder, and one upload_ingested.

Every device arm ends in the call's own stream synchronisation. Reported per
arm: median, min, max in ms. One JSON object on stdout and in --out
(default profiles/blocks_cbor/probe.json), which is written before the
small-block shape starts and again after it.

    python tools/blocks_cbor_probe.py [--log-t 21] [--tau 8] [--b 512] [--small-b 8] [--rounds 10] [--out FILE]
"""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-t", type=int, default=21)
    ap.add_argument("--tau", type=int, default=8)
    ap.add_argument("--b", type=int, default=512)
    ap.add_argument("--small-b", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks_cbor", "probe.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import sezkp_amd as P
    from sezkp_amd._lib import lib
    assert torch.cuda.is_available(), "needs a HIP device"
    t = 1 << args.log_t
    out = {"t": t, "tau": args.tau, "rounds": args.rounds}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")

    def host_c_call(raw):
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        d, rc = ms(lambda: lib.sezkp_blocks_decode_cbor(raw, len(raw), C.byref(h), err, 512))
        assert rc == 0, err.value
        lib.sezkp_blocks_free(h)
        return d

    ctx = P.ProverContext(0)
    # ---------------------------------------------------------------- headline
    blocks = P.reference_blocks(t, args.b, args.tau, 42)
    raw = blocks.to_cbor()
    traw = P.Trace(blocks.input_mv, blocks.mv.reshape(t, args.tau), blocks.has_write.reshape(t, args.tau),
                   blocks.wsym.reshape(t, args.tau)).to_cbor()
    root = blocks.manifest_root()
    del blocks
    pinned = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).pin_memory()
    arms = {k: [] for k in ("host_from_cbor", "host_c_call", "upload_of_decoded", "device_upload_blocks_cbor",
                            "device_ms_h2d", "device_ms_decode", "pinned_upload_blocks_cbor", "pinned_ms_h2d",
                            "pinned_ms_decode", "sibling_upload_trace_cbor", "sibling_ms_h2d", "sibling_ms_decode")}
    proofs = set()
    for r in range(args.rounds + 1):  # round 0 warms every arm (allocations, first launches) and is dropped
        d_host, dec = ms(lambda: P.BlockSoA.from_cbor(raw))
        d_c = host_c_call(raw)
        d_up, _ = ms(lambda: ctx.upload(dec))
        if r == 0:
            proofs.add(ctx.prove(root).proof_bytes)
        del dec
        d_dev, _ = ms(lambda: ctx.upload_blocks_cbor(raw))
        st = ctx.blocks_ingest_stats()
        assert st["path"] == "device", st
        if r == 0:
            proofs.add(ctx.prove(root).proof_bytes)
        d_pin, _ = ms(lambda: ctx.upload_blocks_cbor(pinned))
        sp = ctx.blocks_ingest_stats()
        assert sp["path"] == "device", sp
        d_sib, _ = ms(lambda: ctx.upload_trace_cbor(traw, args.b))
        ss = ctx.trace_ingest_stats()
        assert ss["path"] == "device", ss
        if r == 0:
            continue
        for k, v in (("host_from_cbor", d_host), ("host_c_call", d_c), ("upload_of_decoded", d_up),
                     ("device_upload_blocks_cbor", d_dev), ("device_ms_h2d", st["ms_h2d"]),
                     ("device_ms_decode", st["ms_decode"]), ("pinned_upload_blocks_cbor", d_pin),
                     ("pinned_ms_h2d", sp["ms_h2d"]), ("pinned_ms_decode", sp["ms_decode"]),
                     ("sibling_upload_trace_cbor", d_sib), ("sibling_ms_h2d", ss["ms_h2d"]),
                     ("sibling_ms_decode", ss["ms_decode"])):
            arms[k].append(v)
    assert len(proofs) == 1, "the two paths proved different bytes"
    out["headline"] = {"b": args.b, "n_blocks": t // args.b, "bytes": len(raw), "trace_file_bytes": len(traw),
                       "arms": {k: summary(v) for k, v in arms.items()}}
    a = out["headline"]["arms"]
    out["headline"]["device_h2d_plus_decode_ms"] = a["device_ms_h2d"]["median_ms"] + a["device_ms_decode"]["median_ms"]
    out["headline"]["device_is_the_cli_default"] = (out["headline"]["device_h2d_plus_decode_ms"] <
                                                    a["host_c_call"]["median_ms"])
    print(json.dumps(out["headline"]), flush=True)
    write()
    del raw, traw, pinned
    # ---------------------------------------------------------------- small blocks
    sb = args.small_b
    blocks = P.reference_blocks(t, sb, args.tau, 42)
    raw = blocks.to_cbor()
    del blocks
    arms = {k: [] for k in ("host_c_call", "device_ingest_blocks_cbor", "device_ms_h2d", "device_ms_decode")}
    for r in range(args.rounds + 1):
        d_c = host_c_call(raw) if r < 4 else None  # the host decoder is slow here: three timed rounds
        d_dev, _ = ms(lambda: ctx.ingest_blocks_cbor(raw))
        st = ctx.blocks_ingest_stats()
        assert st["path"] == "device", st
        if r == 0:
            continue
        if d_c is not None:
            arms["host_c_call"].append(d_c)
        for k, v in (("device_ingest_blocks_cbor", d_dev), ("device_ms_h2d", st["ms_h2d"]),
                     ("device_ms_decode", st["ms_decode"])):
            arms[k].append(v)
    out["small_blocks"] = {"b": sb, "n_blocks": t // sb, "bytes": len(raw), "arms": {k: summary(v) for k, v in arms.items()}}
    print(json.dumps(out["small_blocks"]), flush=True)
    write()
    d_up, _ = ms(lambda: ctx.upload_ingested())
    out["small_blocks"]["upload_ingested_once_ms"] = d_up
    write()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
