"""Views for the CBOR encoder's tests: tests/test_cbor_encode_host.py feeds
them as records to tools/cbor_encode_check.cpp (the passes index by index,
under the sanitizers), tests/test_gpu_cbor_encode.py to the device encoder.
The expected bytes are always the host encoder's. A view is a dict: tau,
step_start, the twelve block fields and the four step arrays (mv, has_write,
wsym as [t, tau])."""
import struct

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
WSYM = (0, 23, 24, 255, 256, 65535)
MOVES = (-128, -25, -24, -1, 0, 23, 24, 127)
EDGES = (0, 23, 24, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32)  # both sides of 24, 2^8, 2^16, 2^32
U16 = [v for v in EDGES if v < 1 << 16]
U32 = [v for v in EDGES if v < 1 << 32]
U64 = list(EDGES) + [(1 << 64) - 1]
I64 = list(EDGES) + [-1, -24, -25, -(1 << 8) - 1, -(1 << 16) - 1, -(1 << 32) - 1, I64_MIN, I64_MAX]

# the steps per tile by tape count (cbor_emit_tile_steps): 256 up to 11 tapes,
# halved behind 11, 24, 49, 101 and 203
TILE_EDGES = (11, 12, 24, 25, 49, 50, 101, 102, 203, 204)
TAUS = (0, 1, 8, 23, 24, 40, 41, 255) + TILE_EDGES


def tile_steps(tau):
    h = 1 if tau < 24 else 2
    s = 256
    while s > 1 and s * (18 + h + 15 * tau) > 48 << 10:
        s >>= 1
    return s


def steps(t, tau, seed):
    """Random step arrays that use every integer width."""
    r = np.random.default_rng(seed)
    return dict(input_mv=r.choice(MOVES, t).astype(np.int8), mv=r.choice(MOVES, (t, tau)).astype(np.int8),
                has_write=r.integers(0, 2, (t, tau)).astype(np.uint8),
                wsym=r.choice(WSYM + (7, 1000), (t, tau)).astype(np.uint16))


def view(nks, tau, seed=1, **over):
    """Blocks of nks[k] steps with small random fields; `over` replaces arrays."""
    r = np.random.default_rng(seed)
    B, ss = len(nks), np.concatenate([[0], np.cumsum(nks)]).astype(np.uint64)
    t = int(ss[-1])
    v = dict(tau=tau, step_start=ss, version=np.ones(B, np.uint16), block_id=np.arange(1, B + 1, dtype=np.uint32),
             step_lo=(ss[:-1] + np.uint64(1)).astype(np.uint64), step_hi=ss[1:].astype(np.uint64),
             ctrl_in=r.integers(0, 40, B).astype(np.uint16), ctrl_out=r.integers(0, 40, B).astype(np.uint16),
             in_head_in=r.integers(-300, 300, B).astype(np.int64), in_head_out=r.integers(-300, 300, B).astype(np.int64),
             win_left=r.integers(-70000, 30, B * tau).astype(np.int64),
             win_right=r.integers(-30, 70000, B * tau).astype(np.int64),
             off_in=r.integers(0, 300, B * tau).astype(np.uint32), off_out=r.integers(0, 70000, B * tau).astype(np.uint32))
    v.update(steps(t, tau, seed + 1000))
    v.update(over)
    return v


def widths_view():
    """Every write form (wsym edge x has_write, a non-zero wsym without a
    write included) against every move edge, in both tapes and input_mv."""
    cells = [(w, h, m) for w in WSYM for h in (0, 1) for m in MOVES]
    t = len(cells)
    ws = np.array([[c[0], cells[(i * 7 + 3) % t][0]] for i, c in enumerate(cells)], np.uint16)
    hw = np.array([[c[1], cells[(i * 5 + 1) % t][1]] for i, c in enumerate(cells)], np.uint8)
    mv = np.array([[c[2], cells[(i * 3 + 2) % t][2]] for i, c in enumerate(cells)], np.int8)
    imv = np.array([MOVES[(i // 3) % len(MOVES)] for i in range(t)], np.int8)
    return view([40, t - 40], 2, input_mv=imv, mv=mv, has_write=hw, wsym=ws)


def heads_view():
    """One block per edge value: every head field takes every edge of its type."""
    B, tau = len(I64), 2
    pick = lambda vals, dt, n, skew=0: np.array([vals[(i + skew) % len(vals)] for i in range(n)], dtype=dt)
    return view([1] * B, tau, version=pick(U16, np.uint16, B), ctrl_in=pick(U16, np.uint16, B, 1),
                ctrl_out=pick(U16, np.uint16, B, 2), block_id=pick(U32, np.uint32, B),
                step_lo=pick(U64, np.uint64, B), step_hi=pick(U64, np.uint64, B, 3),
                in_head_in=pick(I64, np.int64, B), in_head_out=pick(I64, np.int64, B, 5),
                win_left=pick(I64, np.int64, B * tau, 7), win_right=pick(I64, np.int64, B * tau, 2),
                off_in=pick(U32, np.uint32, B * tau), off_out=pick(U32, np.uint32, B * tau, 4))


def block_views():
    """(name, view): everything but the one case that crosses the scan's pass."""
    out = [("widths", widths_view()), ("heads", heads_view())]
    out += [(f"B{B}", view([1] * B, 1, seed=B)) for B in (1, 23, 24, 255, 256)]
    out += [(f"n{n}", view([n], 2, seed=n)) for n in (0, 1, 23, 24, 255, 256, 257)]
    out.append(("empties", view([0, 1, 23, 0, 0, 24, 255, 256, 257, 0], 2, seed=5)))
    out.append(("all_empty", view([0, 0, 0], 3, seed=6)))
    for tau in TAUS:  # two tiles, a block boundary inside the first
        out.append((f"tau{tau}", view([3, tile_steps(tau) - 1], tau, seed=tau)))
    out += [(f"tile{t}", view([t], 8, seed=t)) for t in (255, 256, 257)]
    out.append(("b1", view([1] * 300, 8, seed=7)))
    # boundaries before, on and behind the tile edges 256 and 512
    out.append(("edges", view([255, 1, 1, 254, 2, 100], 8, seed=8)))
    out.append(("edges2", view([256, 256, 1, 0, 255], 8, seed=9)))
    for seed, tau in ((11, 2), (12, 8), (13, 2), (14, 8)):
        r = np.random.default_rng(seed)
        out.append((f"random{seed}", view(list(r.integers(0, 90, int(r.integers(1, 40)))), tau, seed=seed)))
    return out


def scan_pass_view():
    """More than 1024 tiles of steps: t = 2^18 + 1 at one tape."""
    t = (1 << 18) + 1
    nks = [1000] * (t // 1000) + [t % 1000]
    return view(nks, 1, seed=21)


def trace_cases():
    """(name, steps dict, tau)"""
    out = [(f"trace_t{t}_tau{tau}", steps(t, tau, t + tau), tau)
           for t, tau in ((0, 0), (0, 3), (1, 1), (23, 2), (24, 2), (255, 8), (256, 8), (257, 8), (700, 8), (65537, 0),
                          (9, 255), (40, 24), (5, 23))]
    return out


def uniform_cases():
    """(name, t, b, view): partitioned traces (block fields but the metadata synthesised)."""
    out = []
    for t, b, tau in ((1000, 64, 2), (513, 512, 8), (300, 1, 8), (512, 512, 8), (7, 100, 3)):
        nb = -(-t // b)
        nks = [min(b, t - k * b) for k in range(nb)]
        v = view(nks, tau, seed=t + b)
        v["ctrl_in"][:] = 0
        v["ctrl_out"][:] = 0
        out.append((f"uniform_t{t}_b{b}", t, b, v))
    return out


def _flat(v, names):
    return b"".join(np.ascontiguousarray(v[n]).tobytes() for n in names)


STEP_ARRAYS = ("input_mv", "mv", "has_write", "wsym")
SCALARS = ("step_start", "version", "block_id", "step_lo", "step_hi", "ctrl_in", "ctrl_out")
META = ("in_head_in", "in_head_out", "win_left", "win_right", "off_in", "off_out")


def block_record(v):
    B, t = len(v["version"]), int(v["step_start"][-1])
    return struct.pack("<IIIIQ", 0, v["tau"], B, 0, t) + _flat(v, SCALARS + META + STEP_ARRAYS)


def uniform_record(v, t, b):
    return struct.pack("<IIIIQ", 2, v["tau"], len(v["version"]), b, t) + _flat(v, META + STEP_ARRAYS)


def trace_record(s, tau):
    return struct.pack("<IIIIQ", 1, tau, 1, 0, len(s["input_mv"])) + _flat(s, STEP_ARRAYS)


def to_blocks(product, v):
    f = {k: (a.reshape(-1) if isinstance(a, np.ndarray) else a) for k, a in v.items() if k != "tau"}
    return product.BlockSoA(v["tau"], **f)
