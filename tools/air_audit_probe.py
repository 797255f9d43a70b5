"""Device time of the full-trace AIR audit on the resident trace, against the
prover's `compose` stage on the same trace (the stage that reads the same mv /
wflag / wsym / head arrays and writes more).

The audit is timed with HIP events on the context's stream around each
ctx.air_audit() call: the span holds what the call enqueues (k_expand, two
memsets, k_air_audit, k_air_audit_first, the counter and guard copies) and
the gaps between them; `expand` (the prover's own stage time of the same
k_expand launch) is printed beside it, so audit - expand bounds the audit
kernels from above. Warm-up, then the median of `reps` calls. The yardstick
is the median of stage_times_ms()["compose"] over the same number of proves
(SEZKP_STAGE_EVENTS=1).
  python3 tools/air_audit_probe.py [log_t] [tau] [reps] [out.json]"""
import json
import os
import statistics
import sys

os.environ["SEZKP_STAGE_EVENTS"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "streaming-zero-knowledge-proofs_amd"))

import torch  # noqa: E402

import sezkp_amd  # noqa: E402


def main():
    log_t = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    tau = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    reps = max(20, int(sys.argv[3])) if len(sys.argv) > 3 else 30
    out = sys.argv[4] if len(sys.argv) > 4 else None
    assert torch.cuda.is_available(), "needs a HIP device"
    blocks = sezkp_amd.reference_blocks(1 << log_t, 512, tau, 42)
    root = blocks.manifest_root()
    ctx = sezkp_amd.ProverContext(0)
    ctx.upload(blocks)
    st = torch.cuda.ExternalStream(ctx.stream)

    def timed_audit(bitmaps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        a = ctx.air_audit(bitmaps=bitmaps)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1), a

    for _ in range(5):
        timed_audit(False)
        timed_audit(True)
        ctx.prove(root)
    audit, audit_bits, compose, expand = [], [], [], []
    for _ in range(reps):  # alternate, so that a drift of the clock hits all alike
        ms, a = timed_audit(False)
        audit.append(ms)
        audit_bits.append(timed_audit(True)[0])
        ctx.prove(root)
        t = ctx.stage_times_ms()
        compose.append(t["compose"])
        expand.append(t["expand"])
    med = statistics.median
    forms = {}  # rows per lane of k_air_audit (SEZKP_AUDIT_ROWS, read per launch)
    for rw in ("1", "2", "4"):
        os.environ["SEZKP_AUDIT_ROWS"] = rw
        for _ in range(3):
            timed_audit(False)
        forms[rw] = med([timed_audit(False)[0] for _ in range(reps)])
    del os.environ["SEZKP_AUDIT_ROWS"]
    ctx.close()
    n = a.n_rows
    read_bytes = n * tau * (1 + 1 + 2 + 4) + n * 5  # mv, wflag, wsym, head; row_blk + row_flags
    res = {
        "trace": f"reference_blocks(1 << {log_t}, 512, {tau}, 42)", "n_rows": n, "tau": tau, "reps": reps,
        "audit_ms_median": med(audit), "audit_ms_min": min(audit), "audit_ms_max": max(audit),
        "audit_with_bitmaps_ms_median": med(audit_bits),
        "audit_ms_median_by_rows_per_lane": forms,
        "expand_stage_ms_median": med(expand),
        "compose_stage_ms_median": med(compose), "compose_stage_ms_min": min(compose),
        "audit_over_compose": med(audit) / med(compose) if med(compose) > 0 else None,
        "audit_minus_expand_ms": med(audit) - med(expand),
        "audit_read_bytes": read_bytes,
        "audit_minus_expand_GBs": read_bytes / (med(audit) - med(expand)) / 1e6 if med(audit) > med(expand) else None,
        "families": a.families, "rows_violating": a.rows_violating, "first_violating": a.first_violating,
        "rows_rejectable": a.rows_rejectable, "first_rejectable": a.first_rejectable,
        "verify_reject_probability": a.verify_reject_probability(),
    }
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
