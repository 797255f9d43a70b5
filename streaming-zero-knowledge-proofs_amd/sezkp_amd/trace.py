"""Movement logs (`TraceFile`, crates/sezkp-trace/src/format.rs:59-68) as
step-major arrays, the input of `ProverContext.upload_trace` /
`StarkV1.prove_trace`: the device partitions them and commits the manifest
(sezkp_ctx_upload_trace), so no BlockSoA is built on the host.

The four arrays are input_mv[t] (i8), mv[t, tau] (i8), has_write[t, tau] (u8)
and wsym[t, tau] (u16), as `simulate()` / `reference_trace()` return them:
numpy arrays, or contiguous torch tensors on the context's device (a trace
produced by a simulator on the GPU goes over without a trip through the host).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Buf, SezkpError, TraceView, lib, take_buf

_NP_TYPES = (np.int8, np.int8, np.uint8, np.uint16)
_NAMES = ("input_mv", "mv", "has_write", "wsym")


def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def trace_shard_rows(t: int, b: int, rank: int, world: int) -> tuple:
    """(row0, nrows): the rows rank `rank` of a `world`-GPU sharded prove reads
    of a trace of t steps cut into blocks of b (sezkp_trace_shard_rows)."""
    row0, nrows = C.c_uint64(), C.c_uint64()
    if not (0 <= t < 1 << 64 and 0 <= b < 1 << 32):
        raise SezkpError(-1, "trace_shard_rows: t or b out of range")
    rc = lib.sezkp_trace_shard_rows(t, b, rank, world, C.byref(row0), C.byref(nrows))
    if rc != 0:
        raise SezkpError(rc, f"trace_shard_rows: invalid shape (t={t}, b={b}, rank={rank}, world={world})")
    return row0.value, nrows.value


def trace_shard_blocks(t: int, b: int, rank: int, world: int) -> dict:
    """{blk_lo, blk_cnt, own_lo, own_cnt}: the blocks the rank reads and the
    blocks it owns (sezkp_trace_shard_blocks)."""
    w = [C.c_uint32() for _ in range(4)]
    if not (0 <= t < 1 << 64 and 0 <= b < 1 << 32):
        raise SezkpError(-1, "trace_shard_blocks: t or b out of range")
    rc = lib.sezkp_trace_shard_blocks(t, b, rank, world, *[C.byref(x) for x in w])
    if rc != 0:
        raise SezkpError(rc, f"trace_shard_blocks: invalid shape (t={t}, b={b}, rank={rank}, world={world})")
    return dict(zip(("blk_lo", "blk_cnt", "own_lo", "own_cnt"), (x.value for x in w)))


def trace_view(input_mv, mv, has_write, wsym, b: int, device: int | None = None, t: int | None = None):
    """(TraceView, keep): the sezkp_trace_view of the four arrays with block
    size b, and the objects that must stay alive while the view is used.
    Torch tensors must be contiguous, of the right width and (when `device` is
    given) on that device; the current torch stream of their device is
    synchronised, so the library's own stream reads finished data.
    t: the steps of the whole trace when the arrays hold only a slice of its
    rows (sezkp_ctx_upload_trace_rows)."""
    arrs = [input_mv, mv, has_write, wsym]
    keep, ptrs, shapes = [], [], []
    for name, a, npt in zip(_NAMES, arrs, _NP_TYPES):
        if _is_torch(a):
            import torch
            width = {torch.int8: 1, torch.uint8: 1, torch.int16: 2, getattr(torch, "uint16", torch.int16): 2}.get(a.dtype)
            if width != np.dtype(npt).itemsize:
                raise SezkpError(-1, f"trace.{name}: tensor dtype {a.dtype} is not {np.dtype(npt).itemsize} byte(s) wide")
            if not a.is_contiguous():
                raise SezkpError(-1, f"trace.{name}: tensor must be contiguous")
            if a.is_cuda:
                if device is not None and a.device.index != device:
                    raise SezkpError(-1, f"trace.{name}: tensor is on {a.device}, the context on device {device}")
                torch.cuda.current_stream(a.device).synchronize()
            keep.append(a)
            ptrs.append(a.data_ptr() if a.numel() else 0)
            shapes.append(tuple(a.shape))
        else:
            a = np.ascontiguousarray(a, dtype=npt)
            keep.append(a)
            ptrs.append(a.ctypes.data if a.size else 0)
            shapes.append(a.shape)
    rows = int(shapes[0][0]) if len(shapes[0]) == 1 else -1
    if rows < 0 or len(shapes[1]) != 2 or shapes[1][0] != rows:
        raise SezkpError(-1, "trace: input_mv must be [t] and mv [t, tau]")
    tau = int(shapes[1][1])
    for name, sh in zip(_NAMES[2:], shapes[2:]):
        if tuple(sh) != (rows, tau):
            raise SezkpError(-1, f"trace.{name} has shape {tuple(sh)}, expected {(rows, tau)}")
    if not 0 <= int(b) < 1 << 32:
        raise SezkpError(-1, "trace: b must fit 32 bits")
    if t is not None and not rows <= int(t) < 1 << 64:
        raise SezkpError(-1, "trace: t must be at least the rows the arrays hold")
    v = TraceView()
    v.t, v.tau, v.b = rows if t is None else int(t), tau, int(b)
    v.input_mv, v.mv, v.has_write, v.wsym = [p or None for p in ptrs]
    return v, keep


class Trace:
    """A TraceFile held as the four step-major numpy arrays."""

    def __init__(self, input_mv, mv, has_write, wsym):
        self.input_mv = np.ascontiguousarray(input_mv, dtype=np.int8)
        self.mv = np.ascontiguousarray(mv, dtype=np.int8)
        self.has_write = np.ascontiguousarray(has_write, dtype=np.uint8)
        self.wsym = np.ascontiguousarray(wsym, dtype=np.uint16)
        if self.mv.ndim != 2 or self.mv.shape[0] != self.input_mv.size:
            raise SezkpError(-1, "trace: input_mv must be [t] and mv [t, tau]")

    @property
    def t(self) -> int:
        return int(self.input_mv.size)

    @property
    def tau(self) -> int:
        return int(self.mv.shape[1])

    def arrays(self) -> tuple:
        return self.input_mv, self.mv, self.has_write, self.wsym

    @classmethod
    def from_cbor(cls, data: bytes) -> "Trace":
        """Decode a TraceFile written as CBOR (sezkp_trace_decode_cbor)."""
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = lib.sezkp_trace_decode_cbor(data, len(data), C.byref(h), err, 512)
        if rc != 0:
            raise SezkpError(rc, err.value.decode())
        return cls._take(h)

    @classmethod
    def _take(cls, h) -> "Trace":
        """The arrays of a sezkp_trace handle, which is freed."""
        try:
            v = lib.sezkp_trace_view_of(h).contents
            t, tau = int(v.t), int(v.tau)

            def arr(p, n, dt):
                if not n:
                    return np.zeros(0, dt)
                return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy()
            return cls(arr(v.input_mv, t, np.int8), arr(v.mv, t * tau, np.int8).reshape(t, tau),
                       arr(v.has_write, t * tau, np.uint8).reshape(t, tau), arr(v.wsym, t * tau, np.uint16).reshape(t, tau))
        finally:
            lib.sezkp_trace_free(h)

    def to_cbor(self) -> bytes:
        """The TraceFile as the reference writes it (sezkp_trace_encode_cbor)."""
        v, _keep = trace_view(*self.arrays(), b=0)
        b = Buf()
        rc = lib.sezkp_trace_encode_cbor(C.byref(v), C.byref(b))
        if rc != 0:
            raise SezkpError(rc, "encode trace cbor")
        return take_buf(b)


def cbor_bytes(data):
    """(address, length, keep) of a TraceFile's CBOR bytes for the C ABI: bytes
    / bytearray / memoryview / a numpy uint8 array, or a CPU torch uint8
    tensor (a pinned one is copied to the device without staging)."""
    if _is_torch(data):
        if data.is_cuda or data.element_size() != 1 or not data.is_contiguous():
            raise SezkpError(-1, "trace bytes: a contiguous CPU uint8 tensor is needed")
        return (data.data_ptr() if data.numel() else None), int(data.numel()), data
    if isinstance(data, (bytes, bytearray, memoryview)):
        a = np.frombuffer(data, dtype=np.uint8)
    else:
        a = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    # an empty file is still a file: a non-null address, so that it is the
    # decoder that answers
    keep = a if a.size else np.zeros(1, np.uint8)
    return keep.ctypes.data, int(a.size), keep


def trace_cbor_head(data):
    """(t, tau, steps_off) when the bytes start with the canonical TraceFile
    head the device decoder takes, else None (sezkp_trace_cbor_head)."""
    p, n, _keep = cbor_bytes(data)
    t, tau, off = C.c_uint64(), C.c_uint32(), C.c_uint64()
    if not lib.sezkp_trace_cbor_head(p, n, C.byref(t), C.byref(tau), C.byref(off)):
        return None
    return t.value, tau.value, off.value


def blocks_cbor_head(data):
    """(n_blocks, tau, first_off) when the bytes start with the canonical head
    of a block file the device decoder takes, else None (sezkp_blocks_cbor_head)."""
    p, n, _keep = cbor_bytes(data)
    nb, tau, off = C.c_uint32(), C.c_uint32(), C.c_uint64()
    if not lib.sezkp_blocks_cbor_head(p, n, C.byref(nb), C.byref(tau), C.byref(off)):
        return None
    return nb.value, tau.value, off.value
