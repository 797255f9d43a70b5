"""Corpora for the TraceFile CBOR decoder (tests/test_trace_cbor_host.py on
the CPU, tests/test_gpu_trace_cbor.py on the device): a small encoder of the
canonical form with hooks for the ways a file can leave it.

A: canonical files, which the device path must take and decode as the host
   decoder does;
B: files the host decoder may accept but the device path declines;
C: files the host decoder refuses.
Every entry is (name, bytes); B adds whether the path is pinned to the host.
"""
import os
import random
import re

import numpy as np

from conftest import GOLDEN, PKG

MOVES = [-128, -25, -24, -1, 0, 23, 24, 127]
SYMS = [None, 0, 23, 24, 255, 256, 0xA268, 65535]  # 0xA268 spells the first two bytes of the signature
SIG = b"\xa2\x68input_mv"


def tiling():
    """{tile, lane_bytes, threads, scan_pass} as csrc/trace_cbor_plan.h defines them."""
    src = open(os.path.join(PKG, "csrc", "trace_cbor_plan.h")).read()
    thr = int(re.search(r"TRACE_CBOR_THREADS = (\d+);", src).group(1))
    lane = int(re.search(r"TRACE_CBOR_LANE_BYTES = (\d+);", src).group(1))
    assert re.search(r"TRACE_CBOR_TILE = TRACE_CBOR_THREADS \* TRACE_CBOR_LANE_BYTES;", src)
    per = int(re.search(r"TRACE_CBOR_SCAN_PASS = TRACE_CBOR_THREADS \* (\d+);", src).group(1))
    return {"tile": thr * lane, "lane_bytes": lane, "threads": thr, "scan_pass": thr * per}


# ------------------------------------------------------------------ encoder
def head(major, v, nbytes=None):
    """An item head; nbytes forces a (non-minimal) argument length."""
    if nbytes is None:
        nbytes = 0 if v < 24 else 1 if v < 1 << 8 else 2 if v < 1 << 16 else 4 if v < 1 << 32 else 8
    if nbytes == 0:
        return bytes([major << 5 | v])
    return bytes([major << 5 | {1: 24, 2: 25, 4: 26, 8: 27}[nbytes]]) + v.to_bytes(nbytes, "big")


def sint(x, nbytes=None):
    return head(0, x, nbytes) if x >= 0 else head(1, -1 - x, nbytes)


def text(s):
    b = s.encode() if isinstance(s, str) else s
    return head(3, len(b)) + b


def enc_tape(sym, mv):
    return b"\xa2" + text("write") + (b"\xf6" if sym is None else head(0, sym)) + text("mv") + sint(mv)


def enc_step(imv, tapes, ntapes=None):
    """tapes: [(sym or None, mv)]; ntapes overrides the array head's count."""
    n = len(tapes) if ntapes is None else ntapes
    return SIG + sint(imv) + text("tapes") + head(4, n) + b"".join(enc_tape(s, m) for s, m in tapes)


def enc_file(steps, tau, t=None, meta=b"\xf6", version=1):
    """steps: encoded step records. Returns (bytes, the offset of each step)."""
    out = bytearray(b"\xa4" + text("version") + head(0, version) + text("tau") + head(0, tau) + text("steps") +
                    head(4, len(steps) if t is None else t))
    offs = []
    for s in steps:
        offs.append(len(out))
        out += s
    out += text("meta") + meta
    return bytes(out), offs


def designed_steps(t, tau, phase=0):
    """(imv, tapes) per step, cycling MOVES and SYMS so that every value meets
    every position."""
    out = []
    for i in range(t):
        tapes = [(SYMS[(3 * i + 5 * r + phase) % 8], MOVES[(i + 3 * r + i // 8 + phase) % 8]) for r in range(tau)]
        out.append((MOVES[(i + phase) % 8], tapes))
    return out


def designed_file(t, tau, phase=0, **kw):
    return enc_file([enc_step(m, tp) for m, tp in designed_steps(t, tau, phase)], tau, **kw)[0]


def np_trace(product, t, tau, seed):
    """A Trace over the whole value ranges, from numpy's generator."""
    g = np.random.default_rng(seed)
    hw = g.integers(0, 2, (t, tau), dtype=np.uint8)
    ws = g.integers(0, 65536, (t, tau)).astype(np.uint16) * hw
    # half of the symbols small, so that all three head lengths occur
    ws = np.where(g.integers(0, 2, (t, tau)) == 1, ws % 300, ws).astype(np.uint16)
    return product.Trace(g.integers(-128, 128, t).astype(np.int8), g.integers(-128, 128, (t, tau)).astype(np.int8), hw,
                         ws)


STRADDLE_SEED, STRADDLE_T = 0, 12000


def straddle_file():
    """(bytes, step offsets) of the seeded tau = 1 file whose steps start at
    tile offsets 0 and tile - 1 and straddle a tile boundary with their
    signature (asserted by the tests that use it)."""
    rnd = random.Random(STRADDLE_SEED)
    steps = [enc_step(rnd.choice(MOVES), [(rnd.choice(SYMS), rnd.choice(MOVES))]) for _ in range(STRADDLE_T)]
    return enc_file(steps, 1)


def straddle_facts(offs, tile):
    """(steps whose signature crosses a tile boundary, the tile offsets hit)."""
    rel = {o % tile for o in offs}
    crossing = [o for o in offs if o % tile > tile - len(SIG)]
    return crossing, rel


def corpus_a_small():
    """The designed grid: tau x t over the head-length thresholds."""
    out = []
    for tau in (0, 1, 23, 24, 255):
        for t in (1, 23, 24, 255, 256):
            out.append((f"grid_tau{tau}_t{t}", designed_file(t, tau, phase=tau + t)))
    return out


def corpus_a_extremes():
    t, tau = 300, 3
    lo = [enc_step(MOVES[2 + i % 4], [(None, MOVES[2 + (i + r) % 4]) for r in range(tau)]) for i in range(t)]
    hi = [enc_step(-128 if i % 2 else 127, [(SYMS[5 + (i + r) % 3], 127 if r % 2 else -25) for r in range(tau)])
          for i in range(t)]
    fixture = open(os.path.join(GOLDEN, "riscv_trace.cbor"), "rb").read()
    return [("fixture", fixture), ("min_length_steps", enc_file(lo, tau)[0]), ("max_length_steps", enc_file(hi, tau)[0]),
            ("zero_steps", enc_file([], 2)[0]), ("meta_number", designed_file(40, 2, meta=head(0, 1000))),
            ("meta_bytes", designed_file(40, 2, meta=head(2, 3) + b"abc"))]


def corpus_a_encoded(product):
    """Files Trace.to_cbor writes: around 2^16 steps, around the compaction
    tile, and one whose tile counts need more than one scan pass."""
    tl = tiling()
    out = [(f"t{t}_tau1", np_trace(product, t, 1, t).to_cbor()) for t in (65535, 65536, 65537)]
    out += [(f"tile_t{t}_tau2", np_trace(product, t, 2, t).to_cbor())
            for t in (tl["tile"] - 1, tl["tile"], tl["tile"] + 1, 2 * tl["tile"] + 3)]
    big = np_trace(product, 70000, 4, 9).to_cbor()
    assert len(big) > tl["scan_pass"] * tl["tile"], "the scan's second pass is not reached"
    out.append(("two_scan_passes_t70000_tau4", big))
    return out


# ------------------------------------------------------------------ corpus B
def corpus_b():
    """(name, bytes, pinned to the host path)."""
    t, tau = 40, 2
    st = designed_steps(t, tau, 1)
    enc = [enc_step(m, tp) for m, tp in st]
    out = []
    m, tp = st[20]
    swapped = list(enc)
    swapped[20] = (b"\xa2" + text("tapes") + head(4, tau) + b"".join(enc_tape(s, v) for s, v in tp) + text("input_mv") +
                   sint(m))
    out.append(("tapes_before_input_mv", enc_file(swapped, tau)[0], True))
    wide = list(enc)
    wide[7] = SIG + sint(5, 1) + text("tapes") + head(4, tau) + b"".join(enc_tape(s, v) for s, v in st[7][1])
    out.append(("non_minimal_int", enc_file(wide, tau)[0], True))
    body = b"".join(enc)
    out.append(("indefinite_steps", b"\xa4" + text("version") + head(0, 1) + text("tau") + head(0, tau) + text("steps") +
                b"\x9f" + body + b"\xff" + text("meta") + b"\xf6", True))
    unk = list(enc)
    s0, v0 = st[9][1][0]
    unk[9] = (SIG + sint(st[9][0]) + text("tapes") + head(4, tau) + b"\xa3" + text("write") +
              (b"\xf6" if s0 is None else head(0, s0)) + text("mv") + sint(v0) + text("x") + head(0, 0) +
              enc_tape(*st[9][1][1]))
    out.append(("unknown_tape_key", enc_file(unk, tau)[0], True))
    out.append(("top_level_key_order", b"\xa4" + text("tau") + head(0, tau) + text("version") + head(0, 1) +
                text("steps") + head(4, t) + body + text("meta") + b"\xf6", True))
    out.append(("meta_map", enc_file(enc, tau, meta=b"\xa1" + text("k") + head(0, 1))[0], True))
    out.append(("meta_text_with_signature", enc_file(enc, tau, meta=text(b"vm " + SIG + b" id"))[0], False))
    return out


# ------------------------------------------------------------------ corpus C
def corpus_c():
    t, tau = 40, 2
    st = designed_steps(t, tau, 2)
    enc = [enc_step(m, tp) for m, tp in st]
    good, offs = enc_file(enc, tau)
    out = [("cut_in_signature", good[:offs[30] + 4]), ("cut_in_value", good[:offs[31] + len(SIG) + 1]),
           ("cut_after_last_step", good[:-6]), ("trailing_byte", good + b"\x00")]

    def with_step(i, rec):
        e = list(enc)
        e[i] = rec
        return enc_file(e, tau)[0]
    m, tp = st[12]
    out.append(("mv_128", with_step(12, enc_step(m, [(tp[0][0], 128), tp[1]]))))
    out.append(("input_mv_-129", with_step(12, enc_step(-129, tp))))
    out.append(("wsym_65536", with_step(12, enc_step(m, [(65536, tp[0][1]), tp[1]]))))
    out.append(("step_with_tau-1_tapes", with_step(12, enc_step(m, tp[:1]))))
    out.append(("step_with_tau+1_tapes", with_step(12, enc_step(m, tp + [(None, 0)]))))
    out.append(("steps_head_t+1", enc_file(enc, tau, t=t + 1)[0]))
    out.append(("steps_head_t-1", enc_file(enc, tau, t=t - 1)[0]))
    out.append(("no_tau", b"\xa3" + text("version") + head(0, 1) + text("steps") + head(4, t) + b"".join(enc) +
                text("meta") + b"\xf6"))
    out.append(("empty", b""))
    return out


def corpus_flips():
    """One changed byte at 64 seeded positions of a t = 300 file (the host
    decoder may accept some: equality is what counts)."""
    base = designed_file(300, 2, 3)
    rnd = random.Random(20)
    out = []
    for _ in range(64):
        p, x = rnd.randrange(len(base)), rnd.randrange(1, 256)
        out.append((f"flip_at_{p}_xor_{x:02x}", base[:p] + bytes([base[p] ^ x]) + base[p + 1:]))
    return out


def host_decode(product, raw):
    """("ok", arrays) or ("err", code, message) of sezkp_trace_decode_cbor."""
    try:
        return ("ok", product.Trace.from_cbor(raw).arrays())
    except product.SezkpError as e:
        return ("err", e.code, str(e))
