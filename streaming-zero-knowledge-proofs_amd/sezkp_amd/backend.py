"""Host-side mirror of the reference's `ProvingBackend` for `StarkV1`
(crates/sezkp-core/src/backend.rs:41-61, crates/sezkp-stark/src/lib.rs:126-190)
over the MI355X C ABI. Same names, same argument meaning, same artifact
(`ProofArtifact`, crates/sezkp-core/src/artifact.rs:55-68); errors raise
`SezkpError` where the reference returns `anyhow::Error`.
"""
from __future__ import annotations

import ctypes as C
import json
import struct
from dataclasses import dataclass, field

from ._lib import (AIR_FAMILIES, INGEST_PATHS, INGEST_REASONS, SEZKP_FLAG_ROOT_FROM_TRACE, SEZKP_FLAG_STREAMING,
                   VERIFY_TIMES, AirAuditC, Buf, ProofRef, SezkpError, TraceIngestInfo, BlocksIngestInfo, BLOCKS_INGEST_REASONS, VerifyResultC, check, lib,
                   take_buf, ENCODE_REASONS, VIEW_FIELDS, EncodeInfo)
from .blocks import BlockSoA
from .trace import Trace, cbor_bytes, trace_view

STAGES = ["expand", "col_commit", "col_outer", "compose", "intt", "lde_ntt", "deep", "layer0_tree",
          "layer0_upper", "fri_fold_trees", "col_openings", "fri_paths", "total",
          # host-side split of the same prove() call (wall clock)
          "host_wall", "host_sync_wait", "host_final_wait", "host_serialize",
          # the FRI forest launch (SEZKP_KERNEL_EVENTS=1; 0 when not recorded)
          "k_forest16"]


@dataclass
class ProofArtifact:
    backend: str
    manifest_root: bytes
    proof_bytes: bytes
    meta: dict = field(default_factory=dict)

    def to_cbor(self) -> bytes:
        """ciborium encoding (io.rs:176-183): map{backend, manifest_root, proof_bytes, meta},
        byte vectors as arrays of uints, meta keys sorted."""
        out = bytearray(b"\xa4")
        def text(s: str):
            b = s.encode()
            return _head(3, len(b)) + b
        def barr(bs: bytes):
            return _head(4, len(bs)) + b"".join(bytes([x]) if x < 24 else bytes([0x18, x]) for x in bs)
        out += text("backend") + text(self.backend)
        out += text("manifest_root") + barr(self.manifest_root)
        out += text("proof_bytes") + barr(self.proof_bytes)
        out += text("meta") + _head(5, len(self.meta))
        for k in sorted(self.meta):
            v = self.meta[k]
            out += text(k) + (text(v) if isinstance(v, str) else _head(0, int(v)))
        return bytes(out)


NUM_QUERIES = 30  # params.rs:31
NO_ROW = (1 << 64) - 1  # first_row / first_violating / first_rejectable when there is none


@dataclass
class AirAudit:
    """Full-trace AIR audit (sezkp_ctx_air_audit): per constraint family
    (mv_domain, head_range, slack_range, sym_range, boundary) a dict {cells,
    rows, first_row, first_tape, first_value}, and two classes of rows:
    violating (some cell of some family is non-zero) and rejectable (the
    reference verifier fails when it queries the row). NO_ROW = no such row."""
    n_rows: int
    tau: int
    families: dict
    rows_violating: int
    first_violating: int
    rows_rejectable: int
    first_rejectable: int
    violating_bits: bytes | None = None
    rejectable_bits: bytes | None = None

    @property
    def ok(self) -> bool:
        return self.rows_violating == 0

    def _rows(self, bits):
        if bits is None:
            return None
        import numpy as np
        b = np.unpackbits(np.frombuffer(bits, np.uint8), bitorder="little")[:self.n_rows]
        return np.flatnonzero(b).astype(np.uint64)

    def violating_rows(self):
        """Ascending rows on which the AIR fails (None without bitmaps)."""
        return self._rows(self.violating_bits)

    def rejectable_rows(self):
        """Ascending rows the verifier rejects when queried (None without bitmaps)."""
        return self._rows(self.rejectable_bits)

    def verify_reject_probability(self) -> float:
        """Chance that verify fails: the NUM_QUERIES query rows are independent
        draws mod n (params.rs:95-105)."""
        return 1.0 - (1.0 - self.rows_rejectable / self.n_rows) ** NUM_QUERIES

    def first_rejected_query(self, rows):
        """The first of a proof's query rows that is rejectable (the row the
        verifier's error names), or None. Needs the bitmaps."""
        if self.rejectable_bits is None:
            raise SezkpError(-1, "first_rejected_query needs an audit with bitmaps=True")
        for r in rows:
            r = int(r)
            if 0 <= r < self.n_rows and (self.rejectable_bits[r >> 3] >> (r & 7)) & 1:
                return r
        return None

    @staticmethod
    def _from_c(a, vbits, rbits) -> "AirAudit":
        fams = {name: {"cells": int(f.cells), "rows": int(f.rows), "first_row": int(f.first_row),
                       "first_tape": int(f.first_tape), "first_value": int(f.first_value)}
                for name, f in zip(AIR_FAMILIES, a.fam)}
        return AirAudit(int(a.n_rows), int(a.tau), fams, int(a.rows_violating), int(a.first_violating),
                        int(a.rows_rejectable), int(a.first_rejectable), vbits, rbits)


@dataclass
class VerifyResult:
    """One proof's verdict from verify_batch: the code and message
    sezkp_stark_v1_verify gives for the same bytes, root and tau."""
    ok: bool
    code: int
    message: str


def _verify_batch(call, proofs, manifest_roots, taus) -> list:
    """call(refs, n, out, err, 1024) -> rc over sezkp_proof_ref[n]."""
    proofs = list(proofs)
    n = len(proofs)
    roots = list(manifest_roots) if manifest_roots is not None else [None] * n
    taus = list(taus) if taus is not None else [0] * n
    if len(roots) != n or len(taus) != n:
        raise SezkpError(-1, "verify_batch: manifest_roots and taus must have one entry per proof")
    refs, out, keep = (ProofRef * n)(), (VerifyResultC * n)(), []
    for i, p in enumerate(proofs):
        raw = bytes(p.proof_bytes if isinstance(p, ProofArtifact) else p)  # read in place: no copy of a bytes object
        keep.append(raw)
        refs[i].bytes, refs[i].len = C.cast(C.c_char_p(raw), C.c_void_p).value, len(raw)
        if roots[i] is not None:
            if len(roots[i]) != 32:
                raise SezkpError(-1, "manifest_root must be 32 bytes")
            rb = bytes(roots[i])
            keep.append(rb)
            refs[i].manifest_root = C.cast(C.c_char_p(rb), C.c_void_p).value
        refs[i].tau = int(taus[i] or 0)
    err = C.create_string_buffer(1024)
    check(call(refs, n, out, err, 1024), err)
    return [VerifyResult(o.code == 0, int(o.code), o.msg.decode(errors="replace")) for o in out]


def _head(major: int, v: int) -> bytes:
    if v < 24:
        return bytes([(major << 5) | v])
    for nb, ai in ((1, 24), (2, 25), (4, 26), (8, 27)):
        if v < 1 << (8 * nb):
            return bytes([(major << 5) | ai]) + v.to_bytes(nb, "big")
    raise ValueError(v)


def _meta(proof: bytes, tau: int, streaming: bool) -> dict:
    m = {"proto": "stark-v1", "domain_n": struct.unpack_from("<Q", proof, 0)[0], "tau": tau}
    if streaming:
        m["mode"] = "streaming"
    return m


class StarkV1:
    """`impl ProvingBackend for StarkV1` on MI355X (stateless associated functions)."""

    @staticmethod
    def prove(blocks: BlockSoA, manifest_root: bytes) -> ProofArtifact:
        return StarkV1._prove(blocks, manifest_root, False)

    @staticmethod
    def prove_streaming(blocks: BlockSoA, manifest_root: bytes) -> ProofArtifact:
        """StarkV1::prove_streaming (lib.rs:170-190): same bytes, meta gains mode=streaming."""
        return StarkV1._prove(blocks, manifest_root, True)

    @staticmethod
    def _prove(blocks: BlockSoA, manifest_root: bytes, streaming: bool) -> ProofArtifact:
        if len(manifest_root) != 32:
            raise SezkpError(-1, "manifest_root must be 32 bytes")
        blocks.check_shape()
        pb, mb = Buf(), Buf()
        err = C.create_string_buffer(1024)
        rc = lib.sezkp_stark_v1_prove(C.byref(blocks.view()), bytes(manifest_root),
                                      SEZKP_FLAG_STREAMING if streaming else 0, C.byref(pb), C.byref(mb), err, 1024)
        check(rc, err)
        proof = take_buf(pb)
        meta = json.loads(take_buf(mb).decode())
        return ProofArtifact("stark", bytes(manifest_root), proof, meta)

    @staticmethod
    def prove_trace(input_mv, mv, has_write, wsym, b: int, streaming: bool = False) -> ProofArtifact:
        """StarkV1::prove for a caller that holds the movement log: the device
        partitions it into blocks of b steps (partition.rs:43-150), commits
        the manifest and proves (sezkp_stark_v1_prove_trace). The artifact's
        manifest_root is the computed one."""
        v, _keep = trace_view(input_mv, mv, has_write, wsym, b)
        pb = Buf()
        root = C.create_string_buffer(32)
        err = C.create_string_buffer(1024)
        check(lib.sezkp_stark_v1_prove_trace(C.byref(v), SEZKP_FLAG_STREAMING if streaming else 0, C.byref(pb), root,
                                             err, 1024), err)
        proof = take_buf(pb)
        return ProofArtifact("stark", root.raw, proof, _meta(proof, int(v.tau), streaming))

    @staticmethod
    def prove_trace_cbor(data, b: int, streaming: bool = False) -> ProofArtifact:
        """prove_trace from a TraceFile's CBOR bytes, decoded on the device
        (sezkp_stark_v1_prove_trace_cbor)."""
        p, n, _keep = cbor_bytes(data)
        if not 0 <= int(b) < 1 << 32:
            raise SezkpError(-1, "trace: b must fit 32 bits")
        pb = Buf()
        root = C.create_string_buffer(32)
        err = C.create_string_buffer(1024)
        check(lib.sezkp_stark_v1_prove_trace_cbor(p, n, int(b), SEZKP_FLAG_STREAMING if streaming else 0, C.byref(pb),
                                                  root, err, 1024), err)
        proof = take_buf(pb)
        tau = int.from_bytes(proof[8:16], "little")  # the proof's header: domain_n, tau
        return ProofArtifact("stark", root.raw, proof, _meta(proof, tau, streaming))

    @staticmethod
    def prove_blocks_cbor(data, manifest_root: bytes, streaming: bool = False) -> ProofArtifact:
        """StarkV1::prove from the CBOR bytes of a block file (blocks.cbor),
        decoded on the device (sezkp_stark_v1_prove_blocks_cbor)."""
        p, n, _keep = cbor_bytes(data)
        root = bytes(manifest_root)
        if len(root) != 32:
            raise SezkpError(-1, "manifest_root must be 32 bytes")
        pb = Buf()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_stark_v1_prove_blocks_cbor(p, n, root, SEZKP_FLAG_STREAMING if streaming else 0, C.byref(pb),
                                                   err, 1024), err)
        proof = take_buf(pb)
        tau = int.from_bytes(proof[8:16], "little")  # the proof's header: domain_n, tau
        return ProofArtifact("stark", root, proof, _meta(proof, tau, streaming))

    @staticmethod
    def verify(artifact: ProofArtifact, blocks: BlockSoA, manifest_root: bytes) -> None:
        """StarkV1::verify (lib.rs:144-162 -> v1/verify.rs:60-196), host CPU."""
        if artifact.backend != "stark":
            raise SezkpError(-5, "backend kind mismatch: expected STARK")
        if bytes(artifact.manifest_root) != bytes(manifest_root):
            raise SezkpError(-5, "manifest root mismatch")
        blocks.check_shape()
        err = C.create_string_buffer(1024)
        rc = lib.sezkp_stark_v1_verify(artifact.proof_bytes, len(artifact.proof_bytes), C.byref(blocks.view()),
                                       bytes(manifest_root), err, 1024)
        check(rc, err)

    @staticmethod
    def verify_batch(proofs, manifest_roots=None, taus=None) -> list:
        """Verify a batch of proofs on device 0 (sezkp_stark_v1_verify_batch):
        one VerifyResult per proof. `proofs`: bytes or ProofArtifacts;
        manifest_roots: per proof 32 bytes or None; taus: per proof, 0 = not
        checked."""
        return _verify_batch(lib.sezkp_stark_v1_verify_batch, proofs, manifest_roots, taus)

    @staticmethod
    def air_audit(blocks: BlockSoA, bitmaps: bool = False) -> AirAudit:
        """Full-trace AIR audit on device 0 (sezkp_stark_v1_air_audit); the
        reference has no counterpart."""
        blocks.check_shape()
        a, vb, rb = AirAuditC(), Buf(), Buf()
        err = C.create_string_buffer(1024)
        rc = lib.sezkp_stark_v1_air_audit(C.byref(blocks.view()), C.byref(a), C.byref(vb) if bitmaps else None,
                                          C.byref(rb) if bitmaps else None, err, 1024)
        check(rc, err)
        return AirAudit._from_c(a, take_buf(vb) if bitmaps else None, take_buf(rb) if bitmaps else None)


class ProverContext:
    """Resident-input prover: upload once (trace image in HBM), prove many times."""

    def __init__(self, device: int = 0):
        err = C.create_string_buffer(1024)
        self._h = lib.sezkp_ctx_create(device, err, 1024)
        if not self._h:
            raise SezkpError(-2, err.value.decode())
        self.tau = 0
        self.n_rows = 0  # rows of the uploaded trace
        self.n_blocks = 0
        self.device = device
        self.rank, self.world = 0, 1

    def upload(self, blocks: BlockSoA) -> None:
        blocks.check_shape()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_upload(self._h, C.byref(blocks.view()), err, 1024), err)
        self.tau = blocks.tau
        self.n_rows = int(blocks.step_start[-1])
        self.n_blocks = blocks.n_blocks

    def upload_trace(self, input_mv, mv, has_write, wsym, b: int) -> None:
        """Upload a raw movement log (step-major numpy arrays, or contiguous
        torch tensors on this context's device): the device partitions it into
        blocks of b steps and commits the manifest (sezkp_ctx_upload_trace);
        prove() then needs no root, and manifest_root() / blocks() report what
        the device computed."""
        v, keep = trace_view(input_mv, mv, has_write, wsym, b, getattr(self, "device", None))
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_upload_trace(self._h, C.byref(v), err, 1024), err)
        self.tau, self.n_rows = int(v.tau), int(v.t)
        self.n_blocks = -(-int(v.t) // int(v.b))
        del keep  # the call is synchronous

    def upload_trace_cbor(self, data, b: int) -> None:
        """Upload a TraceFile from its CBOR bytes: the device decodes a
        canonical file (a declined one goes through the host decoder, with the
        same result), then partitions it as upload_trace does
        (sezkp_ctx_upload_trace_cbor). `data`: see trace.cbor_bytes."""
        p, n, keep = cbor_bytes(data)
        if not 0 <= int(b) < 1 << 32:
            raise SezkpError(-1, "trace: b must fit 32 bits")
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_upload_trace_cbor(self._h, p, n, int(b), err, 1024), err)
        st = self.trace_ingest_stats()
        self.tau, self.n_rows = st["tau"], st["t"]
        self.n_blocks = -(-st["t"] // int(b))
        del keep  # the call is synchronous

    def decode_trace_cbor(self, data) -> Trace:
        """The decode of upload_trace_cbor alone, read back into a Trace
        (sezkp_ctx_decode_trace_cbor); the context's trace image is untouched."""
        p, n, keep = cbor_bytes(data)
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_decode_trace_cbor(self._h, p, n, C.byref(h), err, 1024), err)
        del keep
        return Trace._take(h)

    def trace_ingest_stats(self) -> dict:
        """What the last upload_trace_cbor / decode_trace_cbor call did
        (sezkp_ctx_trace_ingest_stats): path "device" or "host", the reason the
        device path declined ("none" when it did not) with the step index of
        "step" / "chain", bytes, t, tau, candidates, and the times ms_h2d,
        ms_decode (HIP events) and ms_host."""
        i = TraceIngestInfo()
        rc = lib.sezkp_ctx_trace_ingest_stats(self._h, C.byref(i))
        if rc != 0:
            raise SezkpError(rc, "trace_ingest_stats: no decode call on this context yet, or a proof is in flight")
        return {"path": INGEST_PATHS[i.path], "reason": INGEST_REASONS[i.reason], "index": int(i.index),
                "bytes": int(i.bytes), "t": int(i.t), "tau": int(i.tau), "candidates": int(i.candidates),
                "ms_h2d": i.ms_h2d, "ms_decode": i.ms_decode, "ms_host": i.ms_host}

    def _note_ingested(self) -> None:
        st = self.blocks_ingest_stats()
        self.tau, self.n_rows, self.n_blocks = st["tau"], st["t"], st["n_blocks"]

    def ingest_blocks_cbor(self, data) -> BlockSoA:
        """Decode a block file (blocks.cbor) from its CBOR bytes and keep the
        step arrays in the context: on the device for a canonical file (a
        declined one goes through the host decoder, with the same result).
        Returns the blocks' fields and step counts without the step arrays
        (enough for manifest_root()); upload_ingested() then uploads
        (sezkp_ctx_ingest_blocks_cbor). `data`: see trace.cbor_bytes."""
        p, n, keep = cbor_bytes(data)
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_ingest_blocks_cbor(self._h, p, n, C.byref(h), err, 1024), err)
        del keep  # the call is synchronous
        return BlockSoA._take(h, meta=True)

    def upload_ingested(self) -> None:
        """upload() of the pending ingest (sezkp_ctx_upload_ingested)."""
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_upload_ingested(self._h, err, 1024), err)
        self._note_ingested()

    def upload_blocks_cbor(self, data) -> None:
        """ingest_blocks_cbor and upload_ingested in one call
        (sezkp_ctx_upload_blocks_cbor)."""
        p, n, keep = cbor_bytes(data)
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_upload_blocks_cbor(self._h, p, n, err, 1024), err)
        del keep
        self._note_ingested()

    def decode_blocks_cbor(self, data) -> BlockSoA:
        """The decode of upload_blocks_cbor alone, read back into a BlockSoA
        (sezkp_ctx_decode_blocks_cbor); the context's trace image is untouched."""
        p, n, keep = cbor_bytes(data)
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_decode_blocks_cbor(self._h, p, n, C.byref(h), err, 1024), err)
        del keep
        return BlockSoA._take(h)

    def blocks_ingest_stats(self) -> dict:
        """What the last ingest_blocks_cbor / upload_blocks_cbor /
        decode_blocks_cbor call did (sezkp_ctx_blocks_ingest_stats): path
        "device" or "host", the reason the device path declined ("none" when it
        did not) with the block or step index that goes with it, bytes,
        n_blocks, t, tau, the candidate counts, and the times ms_h2d, ms_decode
        (HIP events) and ms_host."""
        i = BlocksIngestInfo()
        rc = lib.sezkp_ctx_blocks_ingest_stats(self._h, C.byref(i))
        if rc != 0:
            raise SezkpError(rc, "blocks_ingest_stats: no decode call on this context yet, or a proof is in flight")
        return {"path": INGEST_PATHS[i.path], "reason": BLOCKS_INGEST_REASONS[i.reason], "index": int(i.index),
                "bytes": int(i.bytes), "n_blocks": int(i.n_blocks), "t": int(i.t), "tau": int(i.tau),
                "block_candidates": int(i.block_candidates), "step_candidates": int(i.step_candidates),
                "ms_h2d": i.ms_h2d, "ms_decode": i.ms_decode, "ms_host": i.ms_host}

    def upload_trace_rows(self, input_mv, mv, has_write, wsym, b: int, t: int, row0: int) -> None:
        """upload_trace from arrays that hold only rows [row0, row0 + len) of a
        trace of t steps (sezkp_ctx_upload_trace_rows): a sharded rank's slice,
        which must contain the rows of `trace_shard_rows(t, b, rank, world)`;
        a single-device context needs the whole trace."""
        if row0 < 0 or t < 0:
            raise SezkpError(-1, "row0 and t must be non-negative")
        v, keep = trace_view(input_mv, mv, has_write, wsym, b, getattr(self, "device", None), t=t)
        nrows = len(keep[0])
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_upload_trace_rows(self._h, C.byref(v), row0, nrows, err, 1024), err)
        self.tau, self.n_rows = int(v.tau), int(v.t)
        self.n_blocks = -(-int(v.t) // int(v.b))
        del keep  # the call is synchronous

    def stage_trace(self, input_mv, mv, has_write, wsym, b: int) -> None:
        """stage() for a raw movement log of the uploaded shape
        (sezkp_ctx_stage_trace); the arrays must stay unchanged until the
        prove that takes them has completed."""
        v, keep = trace_view(input_mv, mv, has_write, wsym, b, getattr(self, "device", None))
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_stage_trace(self._h, C.byref(v), err, 1024), err)
        self._staged = keep  # keep the arrays alive

    def manifest_root(self, frontier: bool = False) -> bytes:
        """The manifest root of the trace image the proofs read, as the device
        computed it (sezkp_ctx_manifest_root): commit_blocks' batch root, or
        the Frontier root of .jsonl block files."""
        out = C.create_string_buffer(32)
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_manifest_root(self._h, 1 if frontier else 0, out, err, 1024), err)
        return out.raw

    def manifest_leaves(self) -> bytes:
        """The manifest leaf hash of every block of the trace image, 32 bytes
        each (sezkp_ctx_manifest_leaves)."""
        nb = max(1, int(getattr(self, "n_blocks", 0)))
        out = C.create_string_buffer(32 * nb)
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_manifest_leaves(self._h, out, nb, err, 1024), err)
        return out.raw[:32 * int(self.n_blocks)]

    def blocks(self) -> BlockSoA:
        """The blocks partition_trace gives for the trace image, with the
        metadata the device computed and the step arrays read back from it
        (sezkp_ctx_trace_blocks)."""
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_trace_blocks(self._h, None, C.byref(h), err, 1024), err)
        return BlockSoA._take(h)

    def blocks_cbor(self) -> bytes:
        """The blocks file (blocks.cbor) of the trace image, written on the
        device (sezkp_ctx_encode_trace_blocks_cbor): the bytes of
        `blocks().to_cbor()`, with no step array read back to the host."""
        b = Buf()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_encode_trace_blocks_cbor(self._h, C.byref(b), err, 1024), err)
        return take_buf(b)

    def encode_blocks_cbor(self, blocks: BlockSoA, steps=None) -> bytes:
        """`blocks.to_cbor()` written on the device (sezkp_ctx_encode_blocks_cbor).
        steps: (input_mv, mv, has_write, wsym) to take in place of the step
        arrays of `blocks`, numpy arrays or contiguous torch tensors on this
        context's device (see trace.trace_view); `blocks` may then be a
        metadata-only BlockSoA. Needs no uploaded trace."""
        v = blocks.view()
        keep = None
        if steps is None:
            blocks.check_shape()
        else:
            blocks.check_shape(int(blocks.input_mv.size))  # its own step arrays are not read
            tv, keep = trace_view(*steps, b=0, device=getattr(self, "device", None))
            if int(tv.tau) != blocks.tau or int(tv.t) != int(blocks.step_start[-1] if blocks.n_blocks else 0):
                raise SezkpError(-1, "encode_blocks_cbor: the step arrays given are of another shape than the blocks")
            for f, _t in VIEW_FIELDS[-4:]:
                setattr(v, f, C.cast(C.c_void_p(getattr(tv, f)), type(getattr(v, f))))
        b = Buf()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_encode_blocks_cbor(self._h, C.byref(v), C.byref(b), err, 1024), err)
        del keep  # the call is synchronous
        return take_buf(b)

    def trace_cbor(self, trace=None) -> bytes:
        """A TraceFile (version 1, no meta) written on the device
        (sezkp_ctx_encode_trace_cbor): of the trace image when `trace` is None,
        else of a Trace or of (input_mv, mv, has_write, wsym), numpy arrays or
        contiguous torch tensors on this context's device. The bytes of
        `Trace.to_cbor()`."""
        b = Buf()
        err = C.create_string_buffer(1024)
        if trace is None:
            check(lib.sezkp_ctx_encode_trace_cbor(self._h, None, C.byref(b), err, 1024), err)
            return take_buf(b)
        arrs = trace.arrays() if isinstance(trace, Trace) else tuple(trace)
        v, keep = trace_view(*arrs, b=0, device=getattr(self, "device", None))
        check(lib.sezkp_ctx_encode_trace_cbor(self._h, C.byref(v), C.byref(b), err, 1024), err)
        del keep  # the call is synchronous
        return take_buf(b)

    def encode_stats(self) -> dict:
        """What the last blocks_cbor / encode_blocks_cbor / trace_cbor call did
        (sezkp_ctx_encode_stats): path "device" or "host", the reason the host
        wrote the file ("none" when it did not), bytes, t, tau, n_blocks, and
        the times ms_kernels, ms_d2h (HIP events) and ms_host."""
        i = EncodeInfo()
        rc = lib.sezkp_ctx_encode_stats(self._h, C.byref(i))
        if rc != 0:
            raise SezkpError(rc, "encode_stats: no encode call on this context yet, or a proof is in flight")
        return {"path": INGEST_PATHS[i.path], "reason": ENCODE_REASONS[i.reason], "bytes": int(i.bytes), "t": int(i.t),
                "tau": int(i.tau), "n_blocks": int(i.n_blocks), "ms_kernels": i.ms_kernels, "ms_d2h": i.ms_d2h,
                "ms_host": i.ms_host}

    def upload_rows(self, blocks: BlockSoA, row0: int, nrows: int) -> None:
        """Upload from a view whose step arrays hold only rows [row0, row0 +
        nrows) (a sharded rank's slice, sezkp_ctx_upload_rows)."""
        if row0 < 0 or nrows < 0:
            raise SezkpError(-1, "row0 and nrows must be non-negative")
        blocks.check_shape(nrows)
        if blocks.step_start[-1] < row0 + nrows:
            raise SezkpError(-1, "rows [row0, row0 + nrows) exceed the trace")
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_upload_rows(self._h, C.byref(blocks.view()), row0, nrows, err, 1024), err)
        self.tau = blocks.tau
        self.n_rows = int(blocks.step_start[-1])

    def stage(self, blocks: BlockSoA) -> None:
        """Pipelined upload of the next trace (same shape as the uploaded one):
        async H2D into the spare trace image, allowed while a proof is in
        flight; the next prove uses it (sezkp_ctx_stage). `blocks` must stay
        alive and unchanged until that prove has started."""
        blocks.check_shape()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_stage(self._h, C.byref(blocks.view()), err, 1024), err)
        self._staged = blocks  # keep the arrays alive

    def prove(self, manifest_root: bytes | None = None, streaming: bool = False) -> ProofArtifact:
        """manifest_root=None: the root of the trace image, computed on the
        device (SEZKP_FLAG_ROOT_FROM_TRACE; needs upload_trace / stage_trace)."""
        pb = Buf()
        err = C.create_string_buffer(1024)
        flags = SEZKP_FLAG_STREAMING if streaming else 0
        if manifest_root is None:
            check(lib.sezkp_ctx_prove(self._h, None, flags | SEZKP_FLAG_ROOT_FROM_TRACE, C.byref(pb), err, 1024), err)
            manifest_root = self.manifest_root()
        else:
            check(lib.sezkp_ctx_prove(self._h, bytes(manifest_root), flags, C.byref(pb), err, 1024), err)
        proof = take_buf(pb)
        return ProofArtifact("stark", bytes(manifest_root), proof, _meta(proof, self.tau, streaming))

    def air_audit(self, bitmaps: bool = False) -> AirAudit:
        """Audit the resident trace against the AIR on every row
        (sezkp_ctx_air_audit); bitmaps=True also fetches the two row bitmaps."""
        a = AirAuditC()
        nbytes = (self.n_rows + 7) // 8
        vb = C.create_string_buffer(nbytes) if bitmaps else None
        rb = C.create_string_buffer(nbytes) if bitmaps else None
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_air_audit(self._h, C.byref(a), vb, rb, err, 1024), err)
        return AirAudit._from_c(a, vb.raw if bitmaps else None, rb.raw if bitmaps else None)

    def verify_batch(self, proofs, manifest_roots=None, taus=None) -> list:
        """Verify a batch of proofs with the Merkle chains hashed on this
        context's device (sezkp_ctx_verify_batch): one VerifyResult per proof,
        equal to the host verifier's verdict. Needs no uploaded trace."""
        return _verify_batch(lambda *a: lib.sezkp_ctx_verify_batch(self._h, *a), proofs, manifest_roots, taus)

    def verify(self, artifact: ProofArtifact, blocks: BlockSoA, manifest_root: bytes) -> None:
        """StarkV1.verify with the hashing on this context's device: same
        checks in the same order, same SezkpError."""
        if artifact.backend != "stark":
            raise SezkpError(-5, "backend kind mismatch: expected STARK")
        if bytes(artifact.manifest_root) != bytes(manifest_root):
            raise SezkpError(-5, "manifest root mismatch")
        blocks.check_shape()
        if blocks.n_blocks and blocks.tau == 0:
            # sezkp_proof_ref cannot ask for a tau of 0 to be checked (0 = unchecked): the host verifier can
            return StarkV1.verify(artifact, blocks, manifest_root)
        # the host call checks tau only for a non-empty block list
        r = self.verify_batch([artifact.proof_bytes], [bytes(manifest_root)], [blocks.tau if blocks.n_blocks else 0])[0]
        if not r.ok:
            raise SezkpError(r.code, r.message)

    def verify_times(self) -> dict:
        """Where the last verify_batch spent its time (sezkp_ctx_verify_times)."""
        buf = (C.c_double * len(VERIFY_TIMES))()
        n = lib.sezkp_ctx_verify_times(self._h, buf, len(VERIFY_TIMES))
        return {VERIFY_TIMES[i]: buf[i] for i in range(n)}

    def prove_view(self, manifest_root: bytes | None = None) -> memoryview:
        """The proof bytes as a read-only view of the context's pinned host
        buffer (no copy); valid until the next prove/upload/close.
        manifest_root=None: the trace image's own root, as prove()."""
        ptr = C.POINTER(C.c_uint8)()
        n = C.c_size_t()
        err = C.create_string_buffer(1024)
        root = None if manifest_root is None else bytes(manifest_root)
        flags = SEZKP_FLAG_ROOT_FROM_TRACE if manifest_root is None else 0
        check(lib.sezkp_ctx_prove_borrow(self._h, root, flags, C.byref(ptr), C.byref(n), err, 1024), err)
        return memoryview((C.c_uint8 * n.value).from_address(C.addressof(ptr.contents))).cast("B").toreadonly()

    def prove_async(self, manifest_root: bytes | None = None) -> None:
        """Start a proof on the context's worker thread (sezkp_ctx_prove_async);
        manifest_root=None: the trace image's own root, as prove()."""
        err = C.create_string_buffer(1024)
        if manifest_root is None:
            check(lib.sezkp_ctx_prove_async(self._h, None, SEZKP_FLAG_ROOT_FROM_TRACE, err, 1024), err)
        else:
            check(lib.sezkp_ctx_prove_async(self._h, bytes(manifest_root), 0, err, 1024), err)

    def wait_view(self) -> memoryview:
        """Wait for the proof started by prove_async; a borrowed view as prove_view."""
        ptr = C.POINTER(C.c_uint8)()
        n = C.c_size_t()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_wait(self._h, C.byref(ptr), C.byref(n), err, 1024), err)
        return memoryview((C.c_uint8 * n.value).from_address(C.addressof(ptr.contents))).cast("B").toreadonly()

    def stage_times_ms(self) -> dict:
        buf = (C.c_double * 32)()
        n = lib.sezkp_ctx_stage_times(self._h, buf, 32)
        return {STAGES[i]: buf[i] for i in range(min(n, len(STAGES)))}

    def comm_stats(self) -> list:
        """Per-collective stats of the last sharded prove: [{name, bytes, ms,
        GBs}] (sezkp_ctx_comm_stats; bytes = what this rank sent over links)."""
        from ._lib import CommStat
        buf = (CommStat * 64)()
        n = lib.sezkp_ctx_comm_stats(self._h, buf, 64)
        out = []
        for i in range(n):
            b, ms = int(buf[i].bytes), float(buf[i].ms)
            out.append({"name": buf[i].name.decode(), "bytes": b, "ms": ms,
                        "GBs": (b / ms / 1e6) if ms > 0 else None})
        return out

    def dict_plans(self) -> list:
        """The dictionary commitment's plan of the last prove, one dict per
        dictionary column: {col, kind, tape, K, a, delta, R, dR, min}
        (sezkp_ctx_dict_plans; empty with SEZKP_NO_DICT=1 or below 1024 rows)."""
        from ._lib import DictPlanInfo
        cap = 1 + 4 * self.tau  # input_mv and, per tape, mv / write flag / wsym / head
        buf = (DictPlanInfo * cap)()
        n = lib.sezkp_ctx_dict_plans(self._h, buf, cap)
        if n < 0:
            why = {-1: "a proof is in flight on this context (or the context is closed)",
                   -2: "copying the plans from the device failed"}.get(n, "unexpected return code")
            raise SezkpError(n, f"dict_plans: {why}")
        return [{f: int(getattr(buf[i], f)) for f, _ in DictPlanInfo._fields_} for i in range(n)]

    def dict_cache_stats(self) -> dict:
        """The dictionary table reuse of the last completed prove:
        {cols_rebuilt, cols_reused, entries_rebuilt} (sezkp_ctx_dict_cache_stats;
        all 0 before the first prove of an upload and with SEZKP_NO_DICT=1)."""
        rebuilt, reused, entries = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        rc = lib.sezkp_ctx_dict_cache_stats(self._h, C.byref(rebuilt), C.byref(reused), C.byref(entries))
        if rc < 0:
            raise SezkpError(rc, "dict_cache_stats: a proof is in flight on this context (or the context is closed)")
        return {"cols_rebuilt": rebuilt.value, "cols_reused": reused.value, "entries_rebuilt": entries.value}

    def head_wide_stats(self) -> list:
        """The wide head ladder in the last completed prove, one dict per head
        dictionary column: {col, tape, origin, span, dR, R, entries_built,
        groups_wide, groups_fallback, groups_out_of_span, table_bytes}
        (sezkp_ctx_head_wide_stats; empty before the first prove of an upload)."""
        from ._lib import HeadWideInfo
        cap = max(1, self.tau)
        buf = (HeadWideInfo * cap)()
        n = lib.sezkp_ctx_head_wide_stats(self._h, buf, cap)
        if n < 0:
            raise SezkpError(n, "head_wide_stats: a proof is in flight on this context (or the context is closed)")
        return [{f: int(getattr(buf[i], f)) for f, _ in HeadWideInfo._fields_} for i in range(n)]

    def pw_table_stats(self) -> dict:
        """The per-block piecewise columns' table form in the last completed
        prove: {cols_by_value, cols_by_block, units_built}
        (sezkp_ctx_pw_table_stats; all 0 before the first prove of an upload)."""
        by_value, by_block, units = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        rc = lib.sezkp_ctx_pw_table_stats(self._h, C.byref(by_value), C.byref(by_block), C.byref(units))
        if rc < 0:
            raise SezkpError(rc, "pw_table_stats: a proof is in flight on this context (or the context is closed)")
        return {"cols_by_value": by_value.value, "cols_by_block": by_block.value, "units_built": units.value}

    def lde_closed_stages(self) -> int:
        """The butterfly stages the last completed prove's first LDE pass formed
        in closed form (sezkp_ctx_lde_closed_stages): 1..3, or 0 for the
        point-by-point load (SEZKP_DP_CLOSED=0, a rank evaluating as many
        points as the trace has rows) and the per-point DEEP division."""
        b = C.c_int32(0)
        rc = lib.sezkp_ctx_lde_closed_stages(self._h, C.byref(b))
        if rc != 0:
            raise SezkpError(rc, "lde_closed_stages: a proof is in flight on this context (or the context is closed)")
        return b.value

    def dist_ntt(self, local, scratch=None, inverse: bool = False, sync: bool = True):
        """Distributed four-step NTT of n = world * local.numel() points, in
        place on `local` (a device u64/i64 tensor; layouts in sezkp_stark.h,
        sezkp_ctx_dist_ntt). Every rank calls it together."""
        import torch
        if local.dtype not in (torch.int64, torch.uint64) or not local.is_cuda or not local.is_contiguous():
            raise SezkpError(-1, "local must be a contiguous 64-bit device tensor")
        m = local.numel()
        if m & (m - 1):
            raise SezkpError(-1, "local length must be a power of two")
        if scratch is None:
            scratch = torch.empty_like(local)
        log_n = (m * self.world).bit_length() - 1
        if sync:
            torch.cuda.current_stream(local.device).synchronize()
        err = C.create_string_buffer(1024)
        check(lib.sezkp_ctx_dist_ntt(self._h, local.data_ptr(), scratch.data_ptr(), log_n, -1 if inverse else 1,
                                     err, 1024), err)
        if sync:
            torch.cuda.ExternalStream(self.stream, device=local.device).synchronize()
        return local

    @property
    def stream(self) -> int:
        return lib.sezkp_ctx_stream(self._h) or 0

    def close(self):
        if self._h:
            lib.sezkp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedProverContext(ProverContext):
    """One STARK v1 proof over `world` GPUs (one process per GPU).

    Every rank uploads the same blocks and calls prove() with the same root;
    every rank gets the identical proof bytes. comm="rccl": the exchanges run
    over RCCL (xGMI) inside the library; the communicator id is created on
    rank 0 and broadcast over the torch.distributed `group`. comm="host":
    the exchanges are staged through host memory and run over the (gloo)
    `group` by `sezkp_amd.dist.HostCollectives` — for tests on one GPU.
    comm="solo": this rank alone on `device` with its own contributions only
    (no group): the per-rank cost model; timings real, proof bytes not.

    From a raw movement log: every rank calls upload_trace (the whole trace;
    the rank copies only its rows) or upload_trace_rows (its slice,
    `trace_shard_rows`), then prove() without a root. The first proof of the
    image partitions each rank's blocks on its GPU and exchanges the input-head
    offsets and the manifest leaves (collectives trace_in_head and
    manifest_leaves in comm_stats()); manifest_root() and manifest_leaves()
    report once a proof has completed, blocks() is not available.
    """

    def __init__(self, rank: int, world: int, device: int = 0, comm: str = "rccl", group=None):
        import torch.distributed as dist
        err = C.create_string_buffer(1024)
        self.tau = 0
        self.n_rows = 0
        self.n_blocks = 0
        self.device = device
        self.rank, self.world = rank, world
        self._hc = None
        if comm == "rccl":
            uid = C.create_string_buffer(128)
            if rank == 0:
                check(lib.sezkp_comm_unique_id(uid, err, 1024), err)
            obj = [bytes(uid.raw)]
            if world > 1:
                dist.broadcast_object_list(obj, src=0, group=group)
            self._h = lib.sezkp_ctx_create_sharded(device, rank, world, obj[0], err, 1024)
        elif comm == "solo":
            self._h = lib.sezkp_ctx_create_sharded_solo(device, rank, world, err, 1024)
        elif comm == "host":
            from .dist import HostCollectives
            self._coll = HostCollectives(group)
            self._hc = self._coll.c_struct()
            self._h = lib.sezkp_ctx_create_sharded_host(device, rank, world, C.byref(self._hc), err, 1024)
        else:
            raise ValueError(f"unknown comm {comm!r}")
        if not self._h:
            raise SezkpError(-2, err.value.decode())
