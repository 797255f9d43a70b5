#!/usr/bin/env python3
"""Headline benchmark: STARK v1 prove throughput on MI355X.

Metric (BASELINE.json): "STARK prove field-elements/sec (NTT+FRI+Merkle),
2^24 domain". One proof = one complete `prove_v1` (column commitments, AIR
composition, INTT + coset LDE + DEEP, layer-0 and all FRI layer trees, query
paths and column openings, bincode proof bytes back on the host) of a
T = 2^21-row, tau = 8 trace (N = 8T = 2^24 LDE points).

`value` is the throughput with every trace already resident in HBM when the
timed region starts (the bench contract): each of `inflight` resident contexts
proves on its own worker, re-proving its own trace; contexts are fed by
persistent host threads from a shared ticket counter. A step = `inflight`
proofs; value = N * proofs * ranks / max-over-ranks time. `host_to_proof`
beside it is SURVEY 8(d)'s t, PCIe-inclusive: blocks in pinned host memory ->
proof bytes on the host (crates/sezkp-stark/src/lib.rs:129-141 takes
&[BlockSummary]); every proof uploads its own trace with hipMemcpyAsync on the
context's copy stream into its spare trace image (sezkp_ctx_stage) while the
context's previous proof runs.

Timing: warmup proofs run straight into the timed ones in ONE continuous
pipeline (no drain, the start stagger applied once); the window runs from the
completion of the last warmup proof to the completion of the last proof and
counts the steps * inflight proofs that complete inside it. The run is
bracketed by barrier + device sync.

Multi-GPU (--gpus N, launched by torch.distributed.run): one process per GPU,
each proving its own traces (independent proofs, weak scaling, no data-path
collective); the barrier / max-time reduction runs over RCCL. With N > 1 the
`sharded` object times ONE T = 2^21 proof over all N GPUs (strong scaling).

A plain run sets up, warms up, times the steps and prints the result line
(the headline fields alone). --dump-outputs DIR also writes what the timed
pipeline returned in its last step: each context's proof bytes, one float32
value per byte, as DIR/proof_ctx<i>.npy. The traces are seeded, so two builds
run with the same arguments can be compared file by file. Everything below
takes runs of its own and is measured only with --full.

Objects beside the headline (--full):
  host_to_proof — the same pipeline with every proof uploading its own trace (PCIe)
  single_proof  — one proof at a time (latency), with the per-stage split
  roofline      — the dominant kernel, the longer of k_layer16 / k_forest16
                  (the BLAKE3 Merkle trees over the 2^24-point LDE and the FRI
                  layers, chosen live): VALU-issue-bound; achieved wave64 VALU
                  instructions/s (PMC count per launch / live HIP-event launch
                  time) against 256 CU x 4 SIMD x 2.4 GHz / 2 cycles, with its
                  HBM view (SURVEY bytes and PMC traffic) beside it
  roofline_ntt  — the HBM-bound kernel family, the LDE NTT passes
  worst_case    — the same prove with the dictionary path off and on a
                  high-entropy trace (full-range i8 moves, 16-bit symbols)
  cpu_baseline  — the C oracle on this host (OpenMP at the headline size, and
                  the reference's recomputing structure at config 1)
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "streaming-zero-knowledge-proofs_amd"))

METRIC = "STARK prove field-elements/sec (NTT+FRI+Merkle), 2^24 domain, 1/2/4/8 GPUs"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip table (spec)
# MI355X_MICROARCH.md: 256 CUs x 4 SIMDs; a wave64 VALU instruction issues over
# 2 cycles (32 lanes/cycle); 2.4 GHz max clock -> 1.2288e12 wave64 instr/s.
VALU_PEAK = 256 * 4 * 2.4e9 / 2
# k_layer16's static VALU mix (tools/isa_hist.py on merkle.hip, profiles/r02_isa_k_layer16.txt):
# 12177 full-rate (v_xor_b32, v_add_u32) and 9594 half-rate instructions (v_alignbit_b32,
# v_add3_u32, carry / 64-bit ops), i.e. 2 and 4 cycles per wave64 instruction
L16_FULL, L16_HALF = 12177, 9594
VALU_PEAK_L16_MIX = VALU_PEAK * 2 * (L16_FULL + L16_HALF) / (2 * L16_FULL + 4 * L16_HALF)


def alg_bytes(n: int, tau: int) -> dict:
    """SURVEY.md §8(d) compulsory traffic, per LDE element N = 8n:
    179 + 9*(3+7tau) B total; the column commitments account for
    72 B per column cell (8 B value + 64 B of tree nodes) = 9*(3+7tau) per LDE element."""
    N = 8 * n
    ncols = 3 + 7 * tau
    return {"total": (179 + 9 * ncols) * N, "col_commit": 72 * ncols * n}


def load_profile(kernel: str) -> dict:
    """Per-launch PMC figures of `kernel` from the committed profile summary
    (tools/profile_round.sh -> profiles/pmc_summary.json)."""
    p = os.path.join(ROOT, "profiles", "pmc_summary.json")
    try:
        allp = json.load(open(p))
    except Exception:
        return {}
    if kernel in allp:
        return allp[kernel]
    # keyed per template instance (k_forest16<4>, k_forest16<2>): the instance
    # with the most instructions per launch is the one the headline shape runs
    inst = [v for k, v in allp.items() if k.split("<")[0] == kernel]
    return max(inst, key=lambda v: v.get("valu_instr_per_launch") or 0) if inst else {}


def host_info() -> dict:
    model = None
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        allowed = len(os.sched_getaffinity(0))
    except AttributeError:
        allowed = os.cpu_count()
    quota = None  # cgroup v2 CPU bandwidth limit, in CPUs
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        quota = None if q == "max" else int(q) / int(per)
    except (OSError, ValueError):
        pass
    return {"cpu_model": model, "nproc": os.cpu_count(), "affinity_cpus": allowed, "cgroup_cpu_quota": quota,
            "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}


def cpu_baseline(T_mt: int, tau: int, T_faithful: int, T_single: int, check=None):
    """The C oracle (sezkp_oracle.c, the restated prove_v1) on this host:
    value = the OpenMP compute-once build on all allotted cores at the headline
    size (SURVEY 8(d) ii); beside it one thread, and the reference-faithful
    structure (1 + 60k LDE passes, prover.rs:312-398) run in full at config 1
    (T = 4096) as the reference runs, single-threaded. `check` = (blocks,
    root, gpu_proof_digest): the OpenMP oracle's proof of those blocks must
    equal the GPU's (the timed pipeline's trace)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_ctypes as O
    from sezkp_amd import reference_blocks
    O.build()
    hi = host_info()
    out = {"unit": "field-elements/s", "kind": "port", **hi}
    # reference-faithful, full run at config 1 (1 thread)
    b1 = reference_blocks(T_faithful, 512, tau)
    r1 = b1.manifest_root()
    progress("cpu baseline: reference-faithful structure at config 1, 1 thread")
    t0 = time.perf_counter()
    p_faith = O.prove_v1(b1, r1, mode=1)
    dt_f = time.perf_counter() - t0
    p_once = O.prove_v1(b1, r1)
    out["reference_faithful"] = {
        "value": 8 * T_faithful / dt_f, "cores": 1, "seconds": dt_f, "same_bytes_as_compute_once": p_faith == p_once,
        "sample": f"config 1: T={T_faithful}, b=512, tau={tau}, the reference's structure (LDE + layer-0 tree "
                  f"recomputed per FRI query path, prover.rs:312-398), 1 thread, full proof"}
    # one thread, compute-once
    bs = reference_blocks(T_single, 512, tau)
    rs = bs.manifest_root()
    progress("cpu baseline: compute-once, 1 thread")
    t0 = time.perf_counter()
    O.prove_v1(bs, rs)
    dt_s = time.perf_counter() - t0
    out["single_thread"] = {"value": 8 * T_single / dt_s, "cores": 1, "seconds": dt_s,
                            "sample": f"compute-once prove_v1, 1 thread, T=2^{T_single.bit_length() - 1}, tau={tau}"}
    # OpenMP at the headline size, at the job's thread budget (OMP_NUM_THREADS)
    # and on every CPU this process may run on; `value` = the faster
    if check is not None:
        bl, r, want = check
    else:
        bl = reference_blocks(T_mt, 512, tau)
        r, want = bl.manifest_root(), None
    N = 8 * T_mt
    env_t = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or hi["affinity_cpus"] or 1
    all_t = hi["affinity_cpus"] or 1
    runs = []
    # every allowed CPU first, on a bounded sample (T = 2^16): on a host whose
    # cgroup quota is below its affinity set (the GPU box: 128 CPUs allowed,
    # 16 CPUs of quota) the threads are throttled, and the headline size took
    # 154 s there (round 4); the headline proof runs at the faster count
    if all_t != env_t:
        used = O.use_mt(all_t)
        Ts = 1 << 16
        bsm = reference_blocks(Ts, 512, tau)
        progress(f"cpu baseline: OpenMP oracle, {used} threads, sample T=2^16")
        t0 = time.perf_counter()
        O.prove_v1(bsm, bsm.manifest_root())
        dta = time.perf_counter() - t0
        used_e = O.use_mt(env_t)
        t0 = time.perf_counter()
        O.prove_v1(bsm, bsm.manifest_root())
        dte = time.perf_counter() - t0
        runs.append({"label": "affinity_cpus", "cores": used, "seconds": dta, "value": 8 * Ts / dta,
                     "sample": "T=2^16 proof", "same_sample_at_env_threads": {"cores": used_e, "seconds": dte,
                                                                             "value": 8 * Ts / dte}})
    best_t = all_t if runs and runs[0]["value"] > runs[0]["same_sample_at_env_threads"]["value"] else env_t
    used = O.use_mt(best_t)
    progress(f"cpu baseline: OpenMP oracle, {used} threads, headline size")
    t0 = time.perf_counter()
    p = O.prove_v1(bl, r)
    dt = time.perf_counter() - t0
    runs.append({"label": "OMP_NUM_THREADS" if best_t == env_t else "affinity_cpus", "cores": used, "seconds": dt,
                 "value": N / dt, "matches_gpu": (hashlib.sha256(p).hexdigest() == want) if want is not None else None})
    best = runs[-1]
    out.update({"value": best["value"], "cores": best["cores"], "seconds": best["seconds"], "by_threads": runs,
                "sample": f"oracle compute-once prove_v1 (C restatement, OpenMP), one full proof at the headline "
                          f"size T=2^{T_mt.bit_length() - 1} (N=2^{N.bit_length() - 1}), tau={tau}, at the thread "
                          f"count that was faster on a T=2^16 sample (OMP_NUM_THREADS={env_t} or every allowed "
                          f"CPU, {all_t}); value = that run ({best['cores']} threads)"})
    if want is not None:
        out["gpu_proof_matches_oracle"] = best["matches_gpu"]
    return out


class Pipeline:
    """`K` resident contexts on one GPU, one persistent host thread each, fed
    from a shared ticket counter (a context takes the next proof when free).
    staged=True: every proof first stages its own trace (pinned host -> spare
    trace image, copy stream) while the context's previous proof runs."""

    def __init__(self, ctxs, traces, roots, staged: bool, stagger_s: float):
        self.ctxs, self.traces, self.roots = ctxs, traces, roots
        self.K = len(ctxs)
        self.staged, self.stagger = staged, stagger_s
        self.lock = threading.Lock()
        self.left = 0
        self.go = threading.Barrier(self.K + 1)
        self.done = threading.Barrier(self.K + 1)
        self.stop = False
        self.done_t, self.l0 = [], []
        self.last = [None] * self.K      # (trace index, view) of each context's last proof
        self.cur = list(range(self.K))  # trace index context i uploaded/staged last
        self.err = None
        self.ths = [threading.Thread(target=self._run, args=(i,), daemon=True) for i in range(self.K)]
        for t in self.ths:
            t.start()

    def _take(self):
        with self.lock:
            if self.left == 0:
                return False
            self.left -= 1
            return True

    def _next_trace(self, i):
        # context i alternates between its traces i, i + K, i + 2K, ...
        n = len(self.traces) // self.K
        j = (self.cur[i] // self.K + 1) % n
        self.cur[i] = i + self.K * j
        return self.cur[i]

    def _run(self, i):
        c = self.ctxs[i]
        while True:
            self.go.wait()
            if self.stop:
                return
            try:
                if i and self.stagger > 0:
                    time.sleep(i * self.stagger)
                have = self._take()
                if have and self.staged:
                    c.stage(self.traces[self._next_trace(i)])
                while have:
                    t = self.cur[i]
                    c.prove_async(self.roots[t])
                    have = self._take()
                    if have and self.staged:
                        c.stage(self.traces[self._next_trace(i)])  # overlaps the proof in flight
                    v = c.wait_view()
                    self.done_t.append(time.perf_counter())
                    self.l0.append(c.stage_times_ms().get("layer0_tree", float("nan")))
                    self.last[i] = (t, v)
            except Exception as e:  # reported by run()
                self.err = e
                with self.lock:
                    self.left = 0
            self.done.wait()

    def run(self, proofs: int) -> tuple:
        """Run `proofs` proofs through the pipeline; returns (t_start, t_end)."""
        self.left = proofs
        self.done_t, self.l0 = [], []
        t0 = time.perf_counter()
        self.go.wait()
        self.done.wait()
        t1 = time.perf_counter()
        if self.err:
            raise self.err
        return t0, t1

    def close(self):
        self.stop = True
        self.go.wait()
        for t in self.ths:
            t.join()


def jsonl_threads(nbytes: int) -> int:
    """Threads the JSONL decoder splits a file of `nbytes` over (codec.cpp
    decode_threads: SEZKP_HOST_THREADS, else OMP_NUM_THREADS, else the
    hardware; at most 64; one per 4 MiB)."""
    t = 0
    for v in ("SEZKP_HOST_THREADS", "OMP_NUM_THREADS"):
        if not t and os.environ.get(v):
            try:  # the C side reads it with atoi: garbage counts as unset
                t = max(0, int(os.environ[v]))
            except ValueError:
                t = 0
    t = t or (os.cpu_count() or 1)
    return min(max(t, 1), 64, max(1, nbytes >> 22))


def measure_host_rows(args, blocks, root: bytes, proof: bytes, seed: int) -> dict:
    """SURVEY 8(f) rows either side of the GPU path, on this host at the
    headline size (T = 2^21, b = 512, tau = 8; one host thread each, as the
    reference runs them, except JSONL decode, timed on its line-range
    threads and on one): the trace generator + partition (`sezkp-cli
    simulate`, generator.rs:38-73 + partition.rs:43-150), the block file
    formats (CBOR io.rs:57-65 / 176-183, JSONL io_jsonl.rs:43-106), the
    manifest root of the CLI's precheck (sezkp-merkle lib.rs:85-157) and the
    verifier (v1/verify.rs:60-196) on the bench's own proof. Each output is
    checked (round trips, the generator's blocks against the bench trace,
    verification accepted)."""
    from sezkp_amd import BlockSoA, ProofArtifact, StarkV1, reference_blocks
    T = blocks.n_rows
    nb = int(blocks.n_blocks)
    out = {"T": T, "blocks": nb, "threads": 1}

    def timed(fn, reps=1):
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        return r, (time.perf_counter() - t0) / reps

    def best(fn, reps=3):  # first-touch page faults dominate a single parallel decode
        r, dt = None, float("inf")
        for _ in range(reps):
            r, d = timed(fn)
            dt = min(dt, d)
        return r, dt

    gen, dt = timed(lambda: reference_blocks(T, args.b, args.tau, seed))
    same = gen.to_cbor() == blocks.to_cbor()
    out["simulate"] = {"seconds": dt, "steps_per_s": T / dt, "seed": seed, "same_as_bench_trace": same}
    cb, dt = timed(lambda: blocks.to_cbor())
    out["cbor_encode"] = {"seconds": dt, "MB": len(cb) / 1e6, "MB_per_s": len(cb) / dt / 1e6}
    back, dt = timed(lambda: BlockSoA.from_cbor(cb))
    out["cbor_decode"] = {"seconds": dt, "MB_per_s": len(cb) / dt / 1e6, "blocks_per_s": nb / dt,
                          "round_trip": back.to_cbor() == cb}
    jl, dt = timed(lambda: blocks.to_jsonl())
    out["jsonl_encode"] = {"seconds": dt, "MB": len(jl) / 1e6, "MB_per_s": len(jl) / dt / 1e6}
    back, dt = best(lambda: BlockSoA.from_jsonl(jl))
    out["jsonl_decode"] = {"seconds": dt, "MB_per_s": len(jl) / dt / 1e6, "blocks_per_s": nb / dt,
                           "round_trip": back.to_cbor() == cb, "threads": jsonl_threads(len(jl))}
    # the one-thread figure the reference's serde_json reader compares with
    old = os.environ.get("SEZKP_HOST_THREADS")
    os.environ["SEZKP_HOST_THREADS"] = "1"
    try:
        back, dt = best(lambda: BlockSoA.from_jsonl(jl))
    finally:
        if old is None:
            del os.environ["SEZKP_HOST_THREADS"]
        else:
            os.environ["SEZKP_HOST_THREADS"] = old
    out["jsonl_decode_1t"] = {"seconds": dt, "MB_per_s": len(jl) / dt / 1e6, "round_trip": back.to_cbor() == cb}
    del back, jl, cb
    mr, dt = timed(lambda: blocks.manifest_root(), 5)
    out["manifest_root"] = {"seconds": dt, "blocks_per_s": nb / dt, "matches": mr == root}
    art = ProofArtifact("stark", root, proof, {})
    ok = True
    try:
        _, dt = timed(lambda: StarkV1.verify(art, blocks, root), 3)
    except Exception as e:  # reported, never fatal
        ok, dt = f"{type(e).__name__}: {e}", float("nan")
    out["verify"] = {"seconds": dt, "accepted": ok, "proof_bytes": len(proof)}
    return out


def high_entropy_blocks(T: int, b: int, tau: int, seed: int):
    """Worst-case input for the dictionary commitments: full-range i8 moves,
    16-bit symbols written with p = 1/2, full-range input moves."""
    import numpy as np
    from sezkp_amd import partition
    rng = np.random.default_rng(seed)
    im = rng.integers(-128, 128, T, dtype=np.int8)
    mv = rng.integers(-128, 128, (T, tau), dtype=np.int8)
    hw = (rng.random((T, tau)) < 0.5).astype(np.uint8)
    ws = (rng.integers(0, 1 << 16, (T, tau), dtype=np.uint16) * hw).astype(np.uint16)
    return partition(im, mv, hw, ws, b)


DUMP_MAX_BYTES = 60_000_000  # of .npy data per --dump-outputs directory (under 64 MB with the headers)


def dump_outputs(outdir: str, proofs, prefix: str = "", max_bytes: int = DUMP_MAX_BYTES) -> dict:
    """Write the proof bytes the timed pipeline returned in its last step, one
    file per context: `outdir`/<prefix>proof_ctx<i>.npy, float32, one value per
    byte. `proofs` = [(trace index, proof bytes)] in context order. When the
    arrays together would pass `max_bytes`, each keeps a fixed sample of its
    positions (seeded by its length alone, ascending), the same from run to
    run. Returns {file name: values written}."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    cap = max(1, max_bytes // (4 * max(1, len(proofs))))
    written = {}
    for i, (_, pb) in enumerate(proofs):
        a = np.frombuffer(pb, dtype=np.uint8)
        if a.size > cap:
            a = a[np.sort(np.random.default_rng(a.size).choice(a.size, cap, replace=False))]
        name = f"{prefix}proof_ctx{i}.npy"
        np.save(os.path.join(outdir, name), a.astype(np.float32))
        written[name] = int(a.size)
    return written


# SEZKP_BENCH_HOST_COMM=1: rehearse the N > 1 paths on ONE GPU (every rank on
# device 0, gloo instead of RCCL, the sharded contexts' exchanges staged
# through host memory): the code paths of `--gpus N`, not its numbers
REHEARSE = os.environ.get("SEZKP_BENCH_HOST_COMM") == "1"
RED_DEV = "cpu" if REHEARSE else "cuda"  # device of the timing reductions
COMM = "host" if REHEARSE else "rccl"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline (host_to_proof, single_proof, rooflines, "
                         "worst case, host rows, CPU baseline, configs, dist_ntt, sharded) and check the timed proofs "
                         "against re-proofs and the oracle; a plain run times the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write each context's last timed proof to DIR/proof_ctx<i>.npy")
    ap.add_argument("--log-t", type=int, default=21, help="trace rows T = 2^log_t (N = 8T)")
    ap.add_argument("--tau", type=int, default=8)
    ap.add_argument("--b", type=int, default=512)
    ap.add_argument("--stagger-ms", type=float, default=-1.0,
                    help="start offset between the in-flight pipelines (-1 = one proof time / inflight)")
    ap.add_argument("--inflight", type=int, default=3,
                    help="independent proofs in flight per GPU (one resident context each, sezkp_ctx_prove_async)")
    ap.add_argument("--traces-per-ctx", type=int, default=2, help="distinct pinned traces each context cycles through")
    ap.add_argument("--cpu-mt-log-t", type=int, default=21)
    ap.add_argument("--cpu-single-log-t", type=int, default=16)
    ap.add_argument("--cpu-faithful-log-t", type=int, default=12,
                    help="reference-faithful (recomputing) oracle run size; 12 = config 1 (T = 4096, ~35 s, 1 thread)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-to-proof", action="store_true", help="skip the staged-upload (host blocks) run")
    ap.add_argument("--no-worst-case", action="store_true")
    ap.add_argument("--no-host-rows", action="store_true",
                    help="skip the SURVEY 8(f) host-side rows (ingest, manifest, trace generator, verifier)")
    ap.add_argument("--worst-steps", type=int, default=10)
    ap.add_argument("--no-configs", action="store_true",
                    help="skip the BASELINE config 2 (2^20 NTT) and config 3 (T=2^18 prove) objects")
    ap.add_argument("--no-sharded", action="store_true",
                    help="N>1: skip the extra sharded (one proof over all GPUs) measurement")
    ap.add_argument("--sharded-steps", type=int, default=5)
    ap.add_argument("--sharded-timeout", type=float, default=240.0,
                    help="watchdog: print the main line and exit (status 3) if an extra measurement stalls")
    ap.add_argument("--dntt-log-n", type=int, default=26,
                    help="distributed four-step NTT sub-measurement size (BASELINE config 4: 2^26); 0 = skip")
    ap.add_argument("--dntt-steps", type=int, default=20)
    ap.add_argument("--detail", default=os.path.join("gpurun_out", "bench_detail.json"),
                    help="file that receives the full measurement record (the stdout line keeps the summary)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(0 if REHEARSE else local)
        dist.init_process_group("gloo" if REHEARSE else "nccl")
    else:
        torch.cuda.set_device(0)

    from sezkp_amd import ProverContext, reference_blocks
    T = 1 << args.log_t
    N = 8 * T
    dev = local if world > 1 and not REHEARSE else 0
    numa = bind_gpu_local_cpus(torch, dev)
    K = max(1, args.inflight)
    # trace pool: context i cycles through traces i, i+K, ...; each is exactly
    # what `sezkp-cli simulate` writes at its seed (42 = the reference's own),
    # its arrays page-locked so staged uploads are DMA
    n_tr = K * max(1, args.traces_per_ctx)
    traces = [reference_blocks(T, args.b, args.tau, 42 + j + 1000 * rank).pin() for j in range(n_tr)]
    roots = [t.manifest_root() for t in traces]
    ctxs = []
    for i in range(K):
        c = ProverContext(dev)
        c.upload(traces[i])  # the first trace of this shape: workspace + image (untimed setup)
        ctxs.append(c)
    ctx = ctxs[0]

    def barrier():
        if dist:
            dist.barrier()
        torch.cuda.synchronize()

    # one proof's latency sets the stagger between the pipelines' starts
    ctx.prove_view(roots[0])
    t_s = time.perf_counter()
    ctx.prove_view(roots[0])
    lat = time.perf_counter() - t_s
    stagger = args.stagger_ms * 1e-3 if args.stagger_ms >= 0 else lat / K

    import gc

    def timed(pipe, steps, warmup):
        """One continuous pipeline run: `warmup` steps straight into `steps`
        timed steps (no drain, no second stagger). The timed window runs from
        the completion of the last warmup proof to the completion of the last
        proof, and counts the steps * K proofs that complete inside it; the run
        is bracketed by barrier + device sync on both sides."""
        w = max(1, warmup) * K
        gc.collect()
        gc.disable()  # no collector pauses in the host threads while proofs are in flight
        barrier()
        c0 = time.process_time()
        pipe.run(w + steps * K)
        barrier()
        ts = sorted(pipe.done_t)
        t_start, t_end = ts[w - 1], ts[-1]
        dt = t_end - t_start
        cpu = (time.process_time() - c0) / (ts[-1] - ts[0] + 1e-9)
        gc.enable()
        if dist:
            t = torch.tensor([dt], dtype=torch.float64, device=RED_DEV)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, halves(ts[w:], t_start), cpu

    total = args.steps * K
    upload_bytes = traces[0].mv.nbytes * 4 + traces[0].input_mv.nbytes
    # ---- `value`: every trace resident in HBM when the timed region starts,
    # each context re-proving its own (the bench contract's value)
    pipe = Pipeline(ctxs, traces, roots, staged=False, stagger_s=stagger)
    dt, halves_, cpu_frac = timed(pipe, args.steps, args.warmup)
    l0_conc = list(pipe.l0)
    resident_last = [(t, bytes(v)) for t, v in pipe.last]  # outside the timed region
    value = N * total * world / dt
    progress(f"pipeline (trace resident): {value / 1e9:.3f}e9 field-elements/s")
    # why `value` is trace-resident and not SURVEY 8(d)'s t (host blocks ->
    # proof bytes): the bench contract this line answers to fixes `value` as
    # the throughput with inputs already resident in HBM and says the
    # PCIe-inclusive rate is never `value`; host_to_proof beside it is 8(d)'s t
    headline = ("trace_resident: the bench contract fixes value as the rate with every input already in HBM "
                "(PCIe-inclusive rates are never value); SURVEY 8(d)'s t, host blocks -> proof bytes, is "
                "host_to_proof on the same line")

    def headline_record(proof_len):
        return {
            "metric": METRIC, "value": value, "unit": "field-elements/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "proofs_per_step": K, "ms_per_proof": dt / total * 1e3,
            "scaling": "weak", "vs_baseline": None, "dtype": "u64",
            "data": f"synthetic: the blocks `sezkp-cli simulate --t {T} --b {args.b} --tau {args.tau}` writes at seeds "
                    f"42..{41 + n_tr} (reference generator + partition, bit-exact restatement)",
            "config": {"workload": f"stark-v1 prove, T=2^{args.log_t} rows (N=2^{args.log_t + 3} LDE domain), "
                                   f"b={args.b}, tau={args.tau}, trace resident in HBM when the timed region starts, "
                                   "proof bytes on the host (host_to_proof beside it: every proof uploads its own "
                                   "trace over PCIe)",
                       "value_is": headline, "upload_bytes_per_proof": upload_bytes,
                       "T": T, "N": N, "tau": args.tau, "b": args.b, "proof_bytes": proof_len,
                       "proofs_in_flight_per_gpu": K, "distinct_traces": n_tr,
                       "parallelism": f"replicas x{world}, {K} independent proofs in flight per GPU"
                                      + (" (REHEARSAL: every rank on GPU 0, gloo + host-staged exchanges; not a "
                                         "multi-GPU measurement)" if REHEARSE and world > 1 else "")},
            "halves_ms_per_proof": halves_, "host_cpu_per_wall": cpu_frac,
            "timing": "one continuous pipeline: warmup proofs run straight into the timed ones; the window runs "
                      "from the last warmup proof's completion to the last proof's completion (steps x inflight "
                      "proofs complete inside it), barrier + device sync around the run",
        }

    dumped = None
    if args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, resident_last, f"rank{rank}_" if world > 1 else "")
    if not args.full:
        # a plain run ends here: the headline alone (every other measurement
        # and the proof checks take runs of their own: --full)
        pipe.close()
        for c in ctxs:
            c.close()
        for t in traces:
            t.unpin()
        if rank == 0:
            out = headline_record(len(resident_last[0][1]))
            if numa is not None:
                out["numa"] = numa
            if dumped is not None:
                out["dumped_outputs"] = dumped
            emit(out, args.detail)
        if dist:
            dist.destroy_process_group()
        return

    # ---- beside it, SURVEY 8(d)'s t: host blocks -> proof bytes, every proof
    # stages its own trace over PCIe (the PCIe-inclusive rate; never `value`)
    last = resident_last
    host = None
    if not args.no_host_to_proof:
        pipe.staged = True
        dt_h, halves_h, cpu_h = timed(pipe, args.steps, args.warmup)
        last = [(t, bytes(v)) for t, v in pipe.last]
        host = {"value": N * total * world / dt_h, "unit": "field-elements/s", "ms_per_proof": dt_h / total * 1e3,
                "ms_per_step": dt_h / args.steps * 1e3, "halves_ms_per_proof": halves_h, "host_cpu_per_wall": cpu_h,
                "note": "the same pipeline with every proof uploading its own trace from pinned host memory over "
                        "PCIe (staged while the context's previous proof runs): SURVEY 8(d)'s t, PCIe-inclusive"}
        progress(f"pipeline (host -> proof): {host['value'] / 1e9:.3f}e9 field-elements/s")
    holds = list(pipe.cur)  # trace each context holds
    pipe.close()
    # consistency: each context's last timed proof (both pipelines) equals an
    # untimed proof of the same trace on another context (other trace slot,
    # other streams)
    consistent = True
    check_digest = {}
    for i, (t, pb) in enumerate(last + resident_last):
        i %= K
        j = (i + 1) % K
        ctxs[j].stage(traces[t])
        consistent &= bytes(ctxs[j].prove_view(roots[t])) == pb
        holds[j] = t
        check_digest[t] = hashlib.sha256(pb).hexdigest()
    if 0 not in check_digest:  # the oracle (cpu_baseline leg) checks trace 0
        ctx.stage(traces[0])
        check_digest[0] = hashlib.sha256(bytes(ctx.prove_view(roots[0]))).hexdigest()
        holds[0] = 0

    # ---- one proof at a time on context 0: latency, stage split, roofline timing
    stage_sum = {}
    nsp = max(5, min(args.steps, 50))
    barrier()
    t1 = time.perf_counter()
    for _ in range(nsp):
        proof = ctx.prove_view(roots[holds[0]])
        for k, v in ctx.stage_times_ms().items():
            if k.startswith("host_"):
                stage_sum[k] = stage_sum.get(k, 0.0) + v
    barrier()
    dt1 = time.perf_counter() - t1
    single_ms = dt1 / nsp * 1e3
    # the same proofs again with timed events around every stage and around
    # the forest launch: the device stage
    # split and the live per-kernel times of the rooflines, kept out of the
    # latency figure above (the events lengthen a proof by ~45 us)
    os.environ["SEZKP_KERNEL_EVENTS"] = "1"
    ksum = {}
    for _ in range(nsp):
        ctx.prove_view(roots[holds[0]])
        for k, v in ctx.stage_times_ms().items():
            if k.startswith("k_") or k == "layer0_tree":
                ksum[k] = ksum.get(k, 0.0) + v
            if not k.startswith(("host_", "k_")):
                stage_sum[k] = stage_sum.get(k, 0.0) + v
    os.environ.pop("SEZKP_KERNEL_EVENTS", None)
    kern_ms = {k: v / nsp for k, v in ksum.items()}
    proof_len = len(proof)
    single_pb = bytes(proof)  # trace holds[0]'s proof, for the host verifier timing (outside every bracket)
    stages = {k: v / nsp for k, v in stage_sum.items()}
    # the staged upload alone: pinned host -> HBM image (copy stream)
    st = torch.cuda.ExternalStream(ctx.stream)
    barrier()
    t1 = time.perf_counter()
    ctx.stage(traces[K])
    ctx.prove_view(roots[K])
    t_up_prove = time.perf_counter() - t1
    up_bytes = traces[K].mv.nbytes * 4 + traces[K].input_mv.nbytes
    del st

    out = None
    if rank == 0:
        # the two tree kernels (each launched once per proof): the layer-0 tree
        # over N leaves and the forest of every FRI layer (N - 1 leaves in all)
        trees = {"k_layer16": tree_roofline("k_layer16", stages.get("layer0_tree", float("nan")), N),
                 "k_forest16": tree_roofline("k_forest16", kern_ms.get("k_forest16", 0.0), N - 1)}
        trees["k_layer16"]["concurrent_mean_launch_ms"] = sum(l0_conc) / len(l0_conc) if l0_conc else None
        # the dominant kernel: the longer of the two, live
        dom = max(trees, key=lambda k: trees[k]["mean_launch_ms"] or 0.0)
        roof = dict(trees[dom])
        roof["selected_as"] = ("the longest kernel of the proof, by its live launch time in this run (both tree "
                               "kernels launch once per proof); the other is in roofline_trees")
        committed = committed_top_kernel()
        if committed:
            roof["committed_stats_top_kernel"] = committed
        out = {
            **headline_record(proof_len),
            "proofs_consistent": consistent,
            "host_to_proof": host,
            "single_proof": {"value": N * nsp / dt1, "unit": "field-elements/s", "ms_per_proof": dt1 / nsp * 1e3,
                             "note": "one proof at a time on one context (rank 0), trace resident: the latency view; "
                                     "stages_ms and roofline come from this pass"},
            "upload": {"bytes": up_bytes, "stage_plus_prove_ms": t_up_prove * 1e3,
                       "note": "one staged upload (pinned host -> HBM image over PCIe) then its proof, alone"},
            "roofline": roof, "roofline_trees": trees, "stages_ms": stages,
        }
        out["roofline_ntt"] = roofline_ntt(args, torch, stages, N, T)
        whole = {"alg_bytes_per_proof": alg_bytes(T, args.tau)["total"]}
        whole["achieved_GBs"] = whole["alg_bytes_per_proof"] * total / dt / 1e9
        whole["frac"] = whole["achieved_GBs"] / HBM_PEAK_GBS
        whole["note"] = ("SURVEY 8(d) bookkeeping (710 B per LDE element); the dictionary/memoised commitments never "
                         "move most of these bytes, so this is not a bandwidth measurement")
        out["whole_prove_alg_bytes"] = whole
    if not consistent and rank == 0:
        out["error"] = "timed proofs differ from an untimed re-proof of the same trace"
        out["value"] = None
    del proof
    worst = None
    if rank == 0 and not args.no_worst_case:
        progress("worst-case inputs")
        worst = measure_worst_case(args, T)
    host_rows = None
    if rank == 0 and not args.no_host_rows:
        progress("host rows")
        host_rows = measure_host_rows(args, traces[holds[0]], roots[holds[0]], single_pb, 42 + holds[0])
    for c in ctxs:
        c.close()
    del ctxs, ctx
    if rank == 0:
        if numa is not None:
            out["numa"] = numa
        if dumped is not None:
            out["dumped_outputs"] = dumped
        out["worst_case"] = worst
        out["host_rows"] = host_rows
        if not args.no_cpu_baseline and world == 1:
            chk = None
            if args.cpu_mt_log_t == args.log_t:
                chk = (traces[0], roots[0], check_digest[0])
            progress("cpu baseline")
            out["cpu_baseline"] = cpu_baseline(1 << args.cpu_mt_log_t, args.tau, 1 << args.cpu_faithful_log_t,
                                               1 << args.cpu_single_log_t, chk)
            if out["cpu_baseline"].get("gpu_proof_matches_oracle") is False:
                out["error"] = "GPU proof of the timed trace differs from the oracle's"
                out["value"] = None
    for t in traces:
        t.unpin()
    del traces

    def guarded(key, fn):
        # extra measurements are reported beside the main line; a watchdog
        # keeps a stalled collective from costing it (and exits non-zero)
        def _bail():
            if rank == 0:
                out[key] = {"error": f"watchdog: no result within {args.sharded_timeout:.0f} s"}
                emit(out, args.detail)
            os._exit(3)
        # the other ranks wait longer: rank 0 enters late (it alone runs the
        # configs) and must print the main line before any rank's exit makes
        # the launcher tear the job down
        wd = threading.Timer(args.sharded_timeout + (0 if rank == 0 else 300.0), _bail)
        wd.daemon = True
        wd.start()
        try:
            res = fn()
        except Exception as e:  # reported, never fatal to the main line
            res = {"error": f"{type(e).__name__}: {e}"}
        wd.cancel()
        if rank == 0:
            out[key] = res

    if rank == 0 and not args.no_configs:
        progress("configs")
        guarded("configs", lambda: measure_configs(args, torch))
    if args.dntt_log_n:
        # BASELINE config 4 (at N = 8): 2^26-point four-step NTT over all ranks
        progress("dist_ntt")
        guarded("dist_ntt", lambda: measure_dist_ntt(args, world, rank, dev, dist, torch))
    if world > 1 and not args.no_sharded:
        # ONE T = 2^21 proof over all ranks (strong scaling)
        progress("sharded")
        guarded("sharded", lambda: measure_sharded(args, world, rank, dev, dist, torch))
    if world == 1 and rank == 0 and not args.no_sharded:
        # the same strong-scaling proof predicted for 2/4/8 GPUs from each
        # rank's own work measured here, plus a link model of its collectives
        progress("sharded_predicted")
        guarded("sharded_predicted", lambda: measure_sharded_predicted(args, torch, single_ms))
    if rank == 0:
        if isinstance(out.get("sharded"), dict):
            # the strong-scaling figure up front, beside the weak-scaling value
            sh = out["sharded"]
            head = {k: out[k] for k in ("metric", "value", "unit", "n_gpus")}
            head["sharded_value"] = sh.get("value")
            head["sharded_ms_per_proof"] = sh.get("ms_per_proof")
            head["sharded_speedup_vs_1gpu_proof"] = (single_ms / sh["ms_per_proof"]) if sh.get("ms_per_proof") else None
            out = {**head, **{k: v for k, v in out.items() if k not in head}}
        emit(out, args.detail)
    if dist:
        dist.destroy_process_group()


LINE_MAX_BYTES = 8192  # the driver read round 3's 10.3 KB line but not round 4's 25.7 KB one


def _pick(d, keys, nd=None):
    """The subset `keys` of dict `d` (missing keys dropped), floats rounded to
    `nd` significant digits when given."""
    if not isinstance(d, dict):
        return d
    out = {}
    for k in keys:
        if k in d:
            v = d[k]
            if nd is not None and isinstance(v, float):
                v = float(f"{v:.{nd}g}")
            out[k] = v
    return out


def compact_line(out: dict, detail_path) -> dict:
    """The stdout line: BASELINE's fields, the dominant kernel's roofline (with
    its HBM view), the CPU baseline and one-number summaries of every other
    measurement. Everything else stays in the detail file the line names."""
    line = _pick(out, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                       "scaling", "vs_baseline", "dtype", "data", "ms_per_proof", "proofs_consistent", "error",
                       "sharded_value", "sharded_ms_per_proof", "sharded_speedup_vs_1gpu_proof", "dumped_outputs"))
    cfg = out.get("config")
    if isinstance(cfg, dict):
        line["config"] = _pick(cfg, ("workload", "value_is", "T", "N", "tau", "b", "proof_bytes",
                                     "proofs_in_flight_per_gpu", "upload_bytes_per_proof", "parallelism"))
    roof = out.get("roofline")
    if isinstance(roof, dict):
        r = _pick(roof, ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "mean_launch_ms",
                         "frac_mix", "measured_on"), 5)
        if isinstance(roof.get("hbm"), dict):
            r["hbm"] = _pick(roof["hbm"], ("alg_bytes_per_launch", "achieved_alg_GBs", "frac_alg",
                                           "traffic_bytes_per_launch", "frac_traffic"), 5)
        top = roof.get("committed_stats_top_kernel")
        if isinstance(top, dict):
            r["rocprof"] = _pick(top, ("name", "average_ms", "file"), 5)
        if isinstance(roof.get("clock"), dict):
            r["clock"] = _pick(roof["clock"], ("clock_ghz_one_proof", "clock_ghz_three_in_flight",
                                               "valu_frac_at_held_clock", "file"), 4)
        line["roofline"] = r
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        c = _pick(cb, ("value", "unit", "cores", "kind", "seconds", "sample", "gpu_proof_matches_oracle", "error"), 5)
        if isinstance(cb.get("reference_faithful"), dict):
            c["reference_faithful"] = _pick(cb["reference_faithful"], ("value", "cores", "seconds", "sample"), 4)
        line["cpu_baseline"] = c
    for k in ("host_to_proof", "trace_resident", "single_proof"):
        if isinstance(out.get(k), dict):
            line[k] = _pick(out[k], ("value", "ms_per_proof"), 5)
    rn = out.get("roofline_ntt")
    if isinstance(rn, dict):
        line["roofline_ntt"] = _pick(rn, ("bound", "achieved", "peak", "unit", "frac", "traffic", "ms"), 4)
    cf = out.get("configs")
    if isinstance(cf, dict):
        s = {}
        for k, keys in (("c2_ntt_2e20", ("ms_fwd_plus_inv", "roundtrip_ok")),
                        ("ntt_2e24", ("ms_per_transform", "roundtrip_ok")),
                        ("ntt_2e26", ("ms_per_transform", "roundtrip_ok")),
                        ("c3_prove_2e18", ("single_proof_ms", "inflight3_ms_per_proof", "matches_oracle")),
                        ("error", None)):
            if k in cf:
                s[k] = cf[k] if keys is None else _pick(cf[k], keys + ("error",), 4)
        line["configs"] = s
    dn = out.get("dist_ntt")
    if isinstance(dn, dict):
        line["dist_ntt"] = _pick(dn, ("value", "ms_per_transform", "roundtrip_ok", "frac_hbm_alg", "error"), 4)
    sp = out.get("sharded_predicted")
    if isinstance(sp, dict):
        s = {str(P): _pick(v, ("predicted_ms_per_proof", "predicted_speedup"), 4)
             for P, v in (sp.get("by_gpus") or {}).items()}
        if "error" in sp:
            s["error"] = sp["error"]
        line["sharded_predicted"] = s
    sh = out.get("sharded")
    if isinstance(sh, dict):
        line["sharded"] = _pick(sh, ("value", "ms_per_proof", "ranks_agree", "matches_single_gpu_proof", "error"), 5)
    wc = out.get("worst_case")
    if isinstance(wc, dict):
        line["worst_case"] = {k: _pick(v, ("single_proof_ms", "inflight3_ms_per_proof"), 4) for k, v in wc.items() if isinstance(v, dict)}
    line["detail"] = detail_path
    return line


def emit(out: dict, detail_path) -> None:
    """Write the full record to `detail_path`, print the compact line (rank 0)."""
    try:
        d = os.path.dirname(detail_path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(detail_path, "w") as f:
            json.dump(out, f, indent=1)
    except OSError as e:
        detail_path = f"not written: {e}"
    s = json.dumps(compact_line(out, detail_path))
    if len(s) > LINE_MAX_BYTES:  # never lose the headline to the line length
        s = json.dumps(_pick(compact_line(out, detail_path),
                             ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
                              "cpu_baseline", "error", "detail")))
    print(s, flush=True)


def bind_gpu_local_cpus(torch, dev):
    """Run this process (its proof threads, the pinned trace buffers they
    first touch, the DMA reads of the uploads) on the CPUs of the GPU's own
    NUMA node (sysfs local_cpulist of its PCI device), capped to the CPUs it
    may already use; SEZKP_BENCH_NUMA=0 leaves placement to the scheduler.
    The PCI address comes from the HIP device properties, so the runtime is
    up by now: every thread the process already has (/proc/self/task: the
    HIP runtime's own threads too) is bound, not only the calling one, and
    threads created later inherit the mask. Measured round 3
    (tools/ab_numa.sh, profiles/r03/ab/ab_numa.txt, three alternating pairs
    on one box, binding the calling thread only): host -> proof 7.75 / 8.03 /
    7.68 -> 8.02 / 7.97 / 7.91e9, trace resident even. Returns what was done."""
    if os.environ.get("SEZKP_BENCH_NUMA", "1") == "0":
        return None
    try:
        p = torch.cuda.get_device_properties(dev)
        bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
        with open(f"/sys/bus/pci/devices/{bdf}/local_cpulist") as f:
            spec = f.read().strip()
        cpus = set()
        for part in spec.split(","):
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return {"pci": bdf, "error": "no allowed CPU on the GPU's node"}
        bound = 0
        for tid in os.listdir("/proc/self/task"):
            try:
                os.sched_setaffinity(int(tid), cpus)
                bound += 1
            except OSError:  # a thread that exited meanwhile
                pass
        return {"pci": bdf, "cpus": len(cpus), "threads_bound": bound,
                "note": "every existing thread of the process (incl. the HIP runtime's) bound; later ones inherit"}
    except Exception as e:  # reported, never fatal
        return {"error": f"{type(e).__name__}: {e}"}


T_START = time.perf_counter()


def progress(msg: str) -> None:
    """A progress line on stderr (the JSON line alone goes to stdout)."""
    print(f"[bench {time.perf_counter() - T_START:7.1f} s] {msg}", file=sys.stderr, flush=True)


def held_clock(kernel: str) -> dict | None:
    """The clock the chip holds during `kernel` (GRBM_GUI_ACTIVE / 8 / wall,
    MI355X_MICROARCH.md "DVFS give-back"), one proof at a time and with the
    bench's 3 proofs in flight, from the committed PMC passes
    (tools/r6_clock.sh -> tools/pmc_clock.py -> profiles/r06/clock.json)."""
    p = os.path.join(ROOT, "profiles", "r06", "clock.json")
    if not os.path.exists(p):
        return None
    c = json.load(open(p))
    pick = lambda d: next((v for k, v in d.items() if k.startswith(kernel + "<") or k == kernel), None)
    one, three = pick(c.get("one_proof", {})), pick(c.get("three_in_flight", {}))
    if not one:
        return None
    return {"clock_ghz_one_proof": one["clock_ghz"], "clock_ghz_three_in_flight": three["clock_ghz"] if three else None,
            "valu_frac_at_held_clock": one["valu_frac_held"], "valu_frac_at_2p4": one["valu_frac_2p4"],
            "reading": "the clock is held (>= 0.94 of 2.4 GHz): the tree kernels are issue-bound, not clock-bound",
            "file": "profiles/r06/clock.json"}


def tree_roofline(kernel: str, ms: float, leaves: int) -> dict:
    """VALU roofline of a BLAKE3 tree kernel from its live launch time and its
    PMC instruction count (profiles/pmc_summary.json), with the HBM view on
    SURVEY 8(d)'s 72 B per leaf (8 B value + 64 B of nodes)."""
    t = ms * 1e-3 if ms and ms > 0 else float("nan")
    prof = load_profile(kernel)
    vi = prof.get("valu_instr_per_launch")
    traffic = prof.get("hbm_bytes_per_launch")
    alg = 72 * leaves
    ok = vi and t == t
    return {"bound": "valu", "kernel": kernel, "achieved": vi / t if ok else None, "peak": VALU_PEAK,
            "unit": "wave64 VALU instr/s", "frac": vi / t / VALU_PEAK if ok else None, "traffic": traffic,
            "mean_launch_ms": ms, "valu_instr_per_launch": vi, "peak_mix": VALU_PEAK_L16_MIX,
            "frac_mix": vi / t / VALU_PEAK_L16_MIX if ok else None,
            "peak_mix_basis": "the same peak with the tree kernels' static instruction mix priced at 2 cycles (full "
                              "rate) / 4 cycles (half rate) per wave64 instruction (profiles/r02_isa_k_layer16.txt)",
            "peak_basis": "MI355X_MICROARCH.md: 256 CU x 4 SIMD, one wave64 VALU instruction per 2 cycles per SIMD, "
                          "2.4 GHz. BLAKE3's rotates (v_alignbit) and 3-input adds issue at half rate on gfx950 "
                          "(tools/micro/valu_rates.hip), so a saturated tree kernel stays below 1.0",
            "hbm": {"alg_bytes_per_launch": alg, "achieved_alg_GBs": alg / t / 1e9 if t == t else None,
                    "frac_alg": alg / t / 1e9 / HBM_PEAK_GBS if t == t else None,
                    "traffic_bytes_per_launch": traffic,
                    "achieved_traffic_GBs": traffic / t / 1e9 if traffic and t == t else None,
                    "frac_traffic": traffic / t / 1e9 / HBM_PEAK_GBS if traffic and t == t else None,
                    "note": "SURVEY 8(d) counts 72 B per leaf (every tree node written); the kernels keep levels "
                            "< 6 in registers/LDS, so their HBM traffic is ~0.12 of that"},
            "clock": held_clock(kernel),
            "measured_on": "single-proof pass: HIP events bracketing exactly the launch on the prover stream",
            "profile": "profiles/pmc_summary.json (tools/profile_round.sh), profiles/*kernel_stats*.csv"}


def committed_top_kernel():
    """The longest kernel of the newest committed single-proof kernel stats
    (profiles/r*/kernel_stats_if1.csv, tools/profile_round.sh), for the record."""
    import csv
    import glob
    cand = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "kernel_stats_if1.csv")) +
                  glob.glob(os.path.join(ROOT, "profiles", "r*", "final", "kernel_stats_if1.csv")))
    if not cand:
        return None
    p = cand[-1]
    try:
        rows = list(csv.DictReader(open(p)))
        top = max(rows, key=lambda r: float(r["TotalDurationNs"]))
        return {"name": top["Name"].split("(")[0].replace("sezkp::", "").replace("void ", ""),
                "average_ms": float(top["AverageNs"]) * 1e-6, "file": os.path.relpath(p, ROOT)}
    except Exception:
        return None


def halves(done_t, t0):
    """Steady-state check: ms per proof over the first and the second half of
    the timed completions `done_t` (sorted), the window opening at `t0` (the
    last warmup completion). Equal halves mean the pipeline was already full
    when the window opened and did not drain inside it."""
    ts = sorted(done_t)
    if len(ts) < 4:
        return None
    h = len(ts) // 2
    return {"first_half": (ts[h - 1] - t0) / h * 1e3, "second_half": (ts[-1] - ts[h - 1]) / (len(ts) - h) * 1e3}


# k_ntt4's static VALU mix (the plain 256-point pass, tools/isa_hist.py on ntt.hip):
# 2142 full-rate and 6510 half-rate instructions (v_cndmask, v_mad_u64_u32, carry
# and 64-bit ops), priced at 2 / 4 cycles per wave64 instruction
NTT_FULL, NTT_HALF = 2142, 6510
VALU_PEAK_NTT_MIX = VALU_PEAK * 2 * (NTT_FULL + NTT_HALF) / (2 * NTT_FULL + 4 * NTT_HALF)
LDE_WIDE = "k_ntt4<false, false, 4, 4, 0, false, false, false>"    # passes 2.. of the LDE
LDE_NARROW = "k_ntt4<false, false, 4, 4, 0, false, true, false>"   # pass 1: DEEP-polynomial coefficients, staged stores


def roofline_ntt(args, torch, stages, N, T):
    """Roofline of the LDE NTT (3 passes over N = 2^24, the DEEP polynomial's
    coefficients generated in the first pass): bytes moved = 16 B per point per
    pass (the first pass reads only the n coefficients); traffic and VALU
    instructions per proof from the per-template PMC summary (the first pass is
    the NARROW instance, the others the wide one)."""
    t_lde = (stages.get("lde_ntt") or float("nan")) * 1e-3  # nan, not 0, when the stage was not timed
    p = os.path.join(ROOT, "profiles", "pmc_summary.json")
    allp = json.load(open(p)) if os.path.exists(p) else {}
    from sezkp_amd._lib import lib
    passes = getattr(lib, "sezkp_gl_lde_passes", None)
    np_ = int(passes(N.bit_length() - 1)) if passes else 3
    moved = 16 * N * np_ - 8 * N + 8 * T  # first pass: n coefficient reads + N writes
    out = {"bound": "hbm", "kernel": f"LDE NTT, {np_} passes over N=2^{N.bit_length() - 1} (DEEP included)",
           "achieved": moved / t_lde / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": moved / t_lde / 1e9 / HBM_PEAK_GBS, "traffic": None, "ms": t_lde * 1e3, "moved_bytes": moved,
           "alg_bytes_survey": 9 * N,
           "measured_on": "single-proof pass: HIP events around the LDE launches on the prover stream"}
    wide, narrow = allp.get(LDE_WIDE, {}), allp.get(LDE_NARROW, {})
    if wide.get("hbm_bytes_per_launch") and narrow.get("hbm_bytes_per_launch"):
        out["traffic"] = (np_ - 1) * wide["hbm_bytes_per_launch"] + narrow["hbm_bytes_per_launch"]
        out["pmc"] = {LDE_WIDE: wide, LDE_NARROW: narrow}
    out["binding_resource"] = "valu (see valu.frac_mix); HBM frac is what the passes move over their duration"
    if wide.get("valu_instr_per_launch") and narrow.get("valu_instr_per_launch"):
        vi = (np_ - 1) * wide["valu_instr_per_launch"] + narrow["valu_instr_per_launch"]
        out["valu"] = {"instr_per_proof": vi, "achieved": vi / t_lde, "unit": "wave64 VALU instr/s",
                       "peak": VALU_PEAK, "frac": vi / t_lde / VALU_PEAK,
                       "peak_mix": VALU_PEAK_NTT_MIX, "frac_mix": vi / t_lde / VALU_PEAK_NTT_MIX,
                       "note": "the passes are VALU-bound: canonical Goldilocks on 32-bit lanes is mostly "
                               "half-rate instructions (carry chains, v_mad_u64_u32, selects); peak_mix prices "
                               "the kernel's static mix at 2 / 4 cycles per wave64 instruction"}
    return out


def measure_worst_case(args, T):
    """The dictionary commitments are exact memoisation: correct for any input,
    fast on the generator's low-entropy traces. Here the same T = 2^21 prove
    (one proof at a time and 3 in flight, trace resident) with the dictionary
    path off (SEZKP_NO_DICT=1) and on a high-entropy trace."""
    from sezkp_amd import ProverContext, reference_blocks
    res = {}
    N = 8 * T
    cases = [("no_dict", lambda: reference_blocks(T, args.b, args.tau, 42), True),
             ("high_entropy", lambda: high_entropy_blocks(T, args.b, args.tau, 7), False)]
    for name, mk, nodict in cases:
        bl = mk()
        r = bl.manifest_root()
        if nodict:
            os.environ["SEZKP_NO_DICT"] = "1"
        try:
            cs = []
            for i in range(3):
                c = ProverContext(0)
                c.upload(bl)  # the dictionary choice is made at upload
                cs.append(c)
        finally:
            os.environ.pop("SEZKP_NO_DICT", None)
        p = bytes(cs[0].prove_view(r))
        t0 = time.perf_counter()
        for _ in range(args.worst_steps):
            cs[0].prove_view(r)
        t1 = (time.perf_counter() - t0) / args.worst_steps
        st = cs[0].stage_times_ms()
        lock = threading.Lock()
        left = [3 * args.worst_steps]

        def pipe(i):
            while True:
                with lock:
                    if left[0] == 0:
                        return
                    left[0] -= 1
                cs[i].prove_async(r)
                cs[i].wait_view()
        t0 = time.perf_counter()
        ws = [threading.Thread(target=pipe, args=(i,)) for i in range(3)]
        for w in ws:
            w.start()
        for w in ws:
            w.join()
        t3 = (time.perf_counter() - t0) / (3 * args.worst_steps)
        same = all(bytes(c.prove_view(r)) == p for c in cs[1:])
        for c in cs:
            c.close()
        res[name] = {"single_proof_ms": t1 * 1e3, "value_single": N / t1, "inflight3_ms_per_proof": t3 * 1e3,
                     "value_inflight3": N / t3, "unit": "field-elements/s", "contexts_agree": same,
                     "col_commit_ms": st.get("col_commit"), "proof_sha256": hashlib.sha256(p).hexdigest()}
    res["note"] = ("trace resident in HBM; no_dict: the generator's trace (seed 42) with SEZKP_NO_DICT=1 (every dense "
                   "column leaf hashed); high_entropy: full-range i8 moves, 16-bit symbols written with p=1/2")
    return res


def det_vec(n: int, seed: int):
    """crates/sezkp-ffts/benches/ntt.rs:21-34: LCG (A=1664525, C=1013904223,
    mod 2^32) started at A*seed + C, stepped before each use; value
    (a_i ^ i*0x9E3779B97F4A7C15) mod p. Vectorised with the affine powers
    f^(j+1)(x) = mul_j x + add_j (mod 2^32) per block of 4096."""
    import numpy as np
    P = 0xFFFFFFFF00000001
    A, Cc, M32 = 1664525, 1013904223, 0xFFFFFFFF
    blk = 1 << 12
    mul = np.empty(blk, dtype=np.uint64)
    add = np.empty(blk, dtype=np.uint64)
    m, c = 1, 0
    for j in range(blk):
        m, c = (A * m) & M32, (A * c + Cc) & M32
        mul[j], add[j] = m, c
    a = np.empty(n, dtype=np.uint64)
    x = (A * seed + Cc) & M32
    for lo in range(0, n, blk):
        hi = min(n, lo + blk)
        a[lo:hi] = (mul[: hi - lo] * np.uint64(x) + add[: hi - lo]) & np.uint64(M32)
        x = (int(mul[-1]) * x + int(add[-1])) & M32
    v = a ^ (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    return np.where(v >= np.uint64(P), v - np.uint64(P), v)


def measure_configs(args, torch):
    """BASELINE configs 2 and 3 on this GPU: the 2^20-point forward + inverse
    NTT of det_vec(2^20, 2024) through sezkp_gl_ntt (round trip checked), and
    the full T = 2^18 prove (one proof at a time and 3 in flight)."""
    from sezkp_amd import ProverContext, reference_blocks
    from sezkp_amd._lib import lib
    out = {}
    n = 1 << 20
    x = torch.from_numpy(det_vec(n, 2024).view("int64")).cuda()
    d, s = x.clone(), torch.empty_like(x)
    for _ in range(3):
        assert lib.sezkp_gl_ntt(d.data_ptr(), s.data_ptr(), 20, 1, None) == 0
        assert lib.sezkp_gl_ntt(d.data_ptr(), s.data_ptr(), 20, -1, None) == 0
    torch.cuda.synchronize()
    ok = bool(torch.equal(d, x))
    # on torch's current stream (the one its events record on), 200 round
    # trips as tools/c2_probe.py: 50 read ~3 us higher (the first ones)
    stream = torch.cuda.current_stream().cuda_stream
    reps = 200
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        lib.sezkp_gl_ntt(d.data_ptr(), s.data_ptr(), 20, 1, stream)
        lib.sezkp_gl_ntt(d.data_ptr(), s.data_ptr(), 20, -1, stream)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    out["c2_ntt_2e20"] = {"workload": "2^20-point Goldilocks NTT, forward + inverse (natural order in and out), "
                                      "det_vec(2^20, 2024) input, sezkp_gl_ntt",
                          "ms_fwd_plus_inv": ms, "value": 2 * n / (ms * 1e-3), "unit": "field-elements/s",
                          "roundtrip_ok": ok and bool(torch.equal(d, x))}
    # 2^24 and 2^26 single-GPU transforms (the LDE size and config 4's size on one device)
    for lg in (24, 26):
        m = 1 << lg
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        x = torch.randint(0, 0xFFFFFFFF00000001 >> 1, (m,), dtype=torch.int64, device="cuda", generator=g)
        d, s = x.clone(), torch.empty_like(x)
        for _ in range(10 if lg < 26 else 5):
            lib.sezkp_gl_ntt(d.data_ptr(), s.data_ptr(), lg, 1, stream)
            lib.sezkp_gl_ntt(d.data_ptr(), s.data_ptr(), lg, -1, stream)
        torch.cuda.synchronize()
        ok = bool(torch.equal(d, x))
        reps = 50 if lg < 26 else 20
        e0.record()
        for _ in range(reps):
            lib.sezkp_gl_ntt(d.data_ptr(), s.data_ptr(), lg, 1, stream)
            lib.sezkp_gl_ntt(d.data_ptr(), s.data_ptr(), lg, -1, stream)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / (2 * reps)
        out[f"ntt_2e{lg}"] = {"workload": f"2^{lg}-point NTT, natural order in and out, sezkp_gl_ntt, one GPU",
                              "ms_per_transform": ms, "roundtrip_ok": ok and bool(torch.equal(d, x)),
                              "alg_GBs": 16 * m / (ms * 1e-3) / 1e9,
                              "frac_hbm_alg": 16 * m / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              "note": "alg = 16 B per point (one read + one write of the array)"}
        del x, d, s
    # config 3: T = 2^18 full prove
    T = 1 << 18
    ctxs, roots = [], []
    for i in range(3):
        bl = reference_blocks(T, args.b, args.tau, 42 + i)
        c = ProverContext(0)
        c.upload(bl)
        ctxs.append(c)
        roots.append(bl.manifest_root())
    for c, r in zip(ctxs, roots):
        c.prove_view(r)
    torch.cuda.synchronize()
    steps = 20
    t0 = time.perf_counter()
    for _ in range(steps):
        ctxs[0].prove_view(roots[0])
    t1 = (time.perf_counter() - t0) / steps
    lock = threading.Lock()
    left = [3 * steps]

    def pipe(i):
        while True:
            with lock:
                if left[0] == 0:
                    return
                left[0] -= 1
            ctxs[i].prove_async(roots[i])
            ctxs[i].wait_view()
    t0 = time.perf_counter()
    ws = [threading.Thread(target=pipe, args=(i,)) for i in range(3)]
    for w in ws:
        w.start()
    for w in ws:
        w.join()
    t3 = (time.perf_counter() - t0) / (3 * steps)
    for c in ctxs:
        c.close()
    N = 8 * T
    out["c3_prove_2e18"] = {"workload": f"stark-v1 prove T=2^18 (N=2^21), b={args.b}, tau={args.tau}",
                            "single_proof_ms": t1 * 1e3, "value_single": N / t1,
                            "inflight3_ms_per_proof": t3 * 1e3, "value_inflight3": N / t3,
                            "unit": "field-elements/s"}
    return out


def measure_dist_ntt(args, world, rank, local, dist, torch):
    """sezkp_ctx_dist_ntt: n = 2^dntt_log_n points split over the ranks
    (strong scaling: fixed n), forward + inverse per step on the context
    stream; one RCCL all-to-all per transform. Round trip checked."""
    from sezkp_amd import ProverContext, ShardedProverContext
    ctx = ShardedProverContext(rank, world, device=local, comm=COMM) if world > 1 else ProverContext(0)
    log_n = args.dntt_log_n
    M = (1 << log_n) // world
    g = torch.Generator(device="cuda")
    g.manual_seed(1234 + rank)
    x = torch.randint(0, 0xFFFFFFFF00000001 >> 1, (M,), dtype=torch.int64, device="cuda", generator=g)
    d = x.clone()
    scratch = torch.empty_like(d)
    for _ in range(2):
        ctx.dist_ntt(d, scratch)
        ctx.dist_ntt(d, scratch, inverse=True)
    ok = bool(torch.equal(d, x))
    st = torch.cuda.ExternalStream(ctx.stream)
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.dntt_steps):
        ctx.dist_ntt(d, scratch, sync=False)
        ctx.dist_ntt(d, scratch, inverse=True, sync=False)
    st.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dist:
        t = torch.tensor([dt], dtype=torch.float64, device=RED_DEV)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        oks = [None] * world
        dist.all_gather_object(oks, ok)
        ok = all(oks)
    ctx.close()
    n = 1 << log_n
    per = dt / (2 * args.dntt_steps)
    alg = 16 * M / per / 1e9  # read + write each local element once, per GPU
    xchg = "1 host-staged (gloo) all-to-all, REHEARSAL on one GPU" if REHEARSE else "1 RCCL all-to-all"
    shape = (f"four-step: local 2^{log_n - (world.bit_length() - 1)} NTT, twiddle, {xchg}, "
             f"{world}-point DFTs" if world > 1 else
             "one rank: natural-order local NTT (DIF passes with the transposed last pass), no exchange")
    return {"workload": f"2^{log_n}-point Goldilocks NTT over {world} GPU(s), forward + inverse ({shape})",
            "value": n / per, "unit": "field-elements/s", "ms_per_transform": per * 1e3, "steps": args.dntt_steps,
            "scaling": "strong", "roundtrip_ok": ok, "alg_GBs_per_gpu": alg, "frac_hbm_alg": alg / HBM_PEAK_GBS}


XGMI_LINK_GBS = 153.0   # per link, per direction (7 links per GPU)
COLL_LATENCY_US = 25.0  # per RCCL call, small-message floor


def measure_sharded_predicted(args, torch, single_ms: float) -> dict:
    """Per-rank cost model of the sharded proof on ONE GPU:
    each rank r of P = 2, 4, 8 runs alone (comm "solo": its own kernels at
    their real shapes, the collectives reduced to its own part), timed wall
    per proof; its collectives are then priced at the bytes it puts on the
    links over min(P-1, 7) xGMI links plus a per-call latency. Predicted
    time(P) = max over ranks of (solo wall - solo collective time + modelled
    collective time). The proof bytes of a solo rank are not a proof."""
    from sezkp_amd import ShardedProverContext, reference_blocks
    T = 1 << args.log_t
    N = 8 * T
    blocks = reference_blocks(T, args.b, args.tau)
    mroot = blocks.manifest_root()
    reps = 5
    res = {"basis": measure_sharded_predicted.__doc__.split("\n\n")[0].replace("\n", " "),
           "link_GBs": XGMI_LINK_GBS, "latency_us_per_collective": COLL_LATENCY_US,
           "single_gpu_ms_per_proof": single_ms, "by_gpus": {}}
    for P in (2, 4, 8):
        progress(f"sharded_predicted: P = {P}")
        ranks = []
        for r in range(P):
            ctx = ShardedProverContext(r, P, device=0, comm="solo")
            ctx.upload(blocks)
            ctx.prove_view(mroot)  # warmup
            torch.cuda.synchronize()
            wall, coll_ms, model_ms, wire = [], 0.0, 0.0, 0
            st_sum = {}
            for _ in range(reps):
                t0 = time.perf_counter()
                ctx.prove_view(mroot)
                wall.append((time.perf_counter() - t0) * 1e3)
            stats = ctx.comm_stats()
            # the stage split from two more proofs with timed stage events
            # (kept out of the wall times: the events lengthen a proof)
            os.environ["SEZKP_STAGE_EVENTS"] = "1"
            for _ in range(2):
                ctx.prove_view(mroot)
                for k, v in ctx.stage_times_ms().items():
                    st_sum[k] = st_sum.get(k, 0.0) + v / 2
            os.environ.pop("SEZKP_STAGE_EVENTS", None)
            for c in stats:
                coll_ms += c["ms"]
                wire += c["bytes"]
                model_ms += c["bytes"] / (min(P - 1, 7) * XGMI_LINK_GBS * 1e9) * 1e3 + COLL_LATENCY_US * 1e-3
            ctx.close()
            w = statistics.median(wall)
            ranks.append({"rank": r, "solo_wall_ms": w, "solo_collective_ms": coll_ms, "collectives": len(stats),
                          "wire_bytes": wire, "model_collective_ms": model_ms,
                          "predicted_ms": w - coll_ms + model_ms,
                          "stages_ms": {k: round(v, 4) for k, v in st_sum.items() if v > 0},
                          "collectives_detail": [{"name": c["name"], "bytes": c["bytes"], "ms": round(c["ms"], 4)}
                                                 for c in stats] if r == 0 else None})
        pm = max(x["predicted_ms"] for x in ranks)
        res["by_gpus"][str(P)] = {"predicted_ms_per_proof": pm, "predicted_value": N / (pm * 1e-3),
                                  "predicted_speedup": single_ms / pm if pm > 0 else None,
                                  "ranks": ranks}
    res["unit"] = "field-elements/s"
    return res


def measure_sharded(args, world, rank, local, dist, torch):
    """ONE proof of the headline trace (T = 2^21, N = 2^24) over all ranks
    (strong scaling), its bytes compared with the single-GPU proof of the same
    blocks; per-stage device times of rank 0."""
    from sezkp_amd import ProverContext, ShardedProverContext, reference_blocks
    T = 1 << args.log_t
    blocks = reference_blocks(T, args.b, args.tau)
    mroot = blocks.manifest_root()
    single = None
    if rank == 0:
        c1 = ProverContext(local)
        c1.upload(blocks)
        single = hashlib.sha256(bytes(c1.prove_view(mroot))).hexdigest()
        c1.close()
    ctx = ShardedProverContext(rank, world, device=local, comm=COMM)
    ctx.upload(blocks)
    del blocks
    ctx.prove(mroot)  # warmup
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stage_sum = {}
    coll_sum = {}
    for _ in range(args.sharded_steps):
        view = ctx.prove_view(mroot)
        for c in ctx.comm_stats():
            a = coll_sum.setdefault(c["name"], {"bytes": c["bytes"], "ms": 0.0})
            a["ms"] += c["ms"]
    dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # rank 0's stage split from a few more proofs with timed stage events (every
    # rank runs them: the proof is collective), outside the timed window
    n_st = min(3, args.sharded_steps)
    os.environ["SEZKP_STAGE_EVENTS"] = "1"
    for _ in range(n_st):
        ctx.prove_view(mroot)
        for k, v in ctx.stage_times_ms().items():
            stage_sum[k] = stage_sum.get(k, 0.0) + v
    os.environ.pop("SEZKP_STAGE_EVENTS", None)
    t = torch.tensor([dt], dtype=torch.float64, device=RED_DEV)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    digest = hashlib.sha256(view).hexdigest()
    plen = len(view)
    ds = [None] * world
    dist.all_gather_object(ds, digest)
    ctx.close()
    N = 8 * T
    ok = len(set(ds)) == 1 and (rank != 0 or ds[0] == single)
    res = {"metric": METRIC, "value": N * args.sharded_steps / dt if ok else None, "unit": "field-elements/s",
           "ms_per_proof": dt / args.sharded_steps * 1e3, "steps": args.sharded_steps, "scaling": "strong",
           "config": {"workload": f"ONE stark-v1 proof over {world} GPUs, T=2^{T.bit_length() - 1} rows "
                                  f"(N=2^{N.bit_length() - 1}), b={args.b}, tau={args.tau}, trace resident",
                      "parallelism": f"sharded x{world}: coset-split LDE, 1 {'host-staged' if REHEARSE else 'RCCL'} "
                                     f"all-to-all, allgathered Merkle caps, byte-sum proof assembly"
                                     + (" (REHEARSAL: all ranks on GPU 0)" if REHEARSE else "")},
           "ranks_agree": len(set(ds)) == 1, "matches_single_gpu_proof": ds[0] == single, "proof_bytes": plen,
           "stages_ms_rank0": {k: v / n_st for k, v in stage_sum.items()},
           "collectives_rank0": {k: {"bytes_sent": v["bytes"], "ms": v["ms"] / args.sharded_steps,
                                     "GBs": v["bytes"] / (v["ms"] / args.sharded_steps) / 1e6 if v["ms"] > 0 else None}
                                 for k, v in coll_sum.items()},
           "collectives_note": "HIP events around each RCCL call on rank 0's prover stream (includes the wait for "
                               "peers to arrive); bytes_sent = what rank 0 puts on its xGMI links per call"}
    if not ok:
        res["error"] = "sharded proof differs across ranks or from the single-GPU proof"
    return res


if __name__ == "__main__":
    main()
