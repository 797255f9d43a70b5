"""Corpora for the block-file CBOR decoder (tests/test_blocks_cbor_host.py on
the CPU, tests/test_gpu_blocks_cbor.py on the device): a small encoder of the
canonical Vec<BlockSummary> form with hooks for the ways a file can leave it.

A: canonical files, which the device path must take and decode as the host
   decoder does;
B: files the host decoder accepts but the device path declines (or, where
   not pinned, may take if it decodes them alike);
C: files the host decoder refuses.
Every entry is (name, bytes); B adds what the device path must answer:
None (not pinned to a path), or (reason, index or None).
"""
import functools
import os
import random

import numpy as np

from conftest import GOLDEN
from trace_cbor_corpus import MOVES, SYMS, designed_steps, enc_step, enc_tape, head, sint, text, tiling  # noqa: F401

BLOCK_SIG = b"\xae\x67version"
STEP_SIG = b"\xa2\x68input_mv"
U16 = [0, 23, 24, 255, 256, 65535]
U32 = U16 + [65536, (1 << 32) - 1]
U64 = U32 + [1 << 32, (1 << 64) - 1]
I64 = U32 + [1 << 32, (1 << 63) - 1, -1, -24, -25, -256, -257, -65537, -(1 << 32) - 1, -(1 << 63)]
TAG_BYTES = [0, 23, 24, 255]
ARRAYS = ("version", "block_id", "step_lo", "step_hi", "ctrl_in", "ctrl_out", "in_head_in", "in_head_out", "win_left",
          "win_right", "off_in", "off_out", "step_start", "input_mv", "mv", "has_write", "wsym")


# ------------------------------------------------------------------ encoder
def enc_tags(tags, as_bytes=False):
    """tags: per tape 16 byte values (array of uints, as serde writes [u8; 16])."""
    if as_bytes:
        return head(4, len(tags)) + b"".join(head(2, 16) + bytes(t) for t in tags)
    return head(4, len(tags)) + b"".join(b"\x90" + b"".join(head(0, x) for x in t) for t in tags)


def block_items(b, raw=None):
    """[(key, encoded value)] of one block in serde's field order. b: a dict
    with the scalar fields, windows [(left, right)], off_in, off_out, steps
    (encoded records), pre / post (tags; default zero). raw: encoded values
    that replace a field's (a non-minimal integer, say)."""
    raw = raw or {}
    tau = len(b["windows"])
    zero = [[0] * 16] * tau

    def val(k, enc):
        return raw[k] if k in raw else enc()
    it = [(k, val(k, lambda k=k: head(0, b[k]))) for k in ("version", "block_id", "step_lo", "step_hi", "ctrl_in",
                                                         "ctrl_out")]
    it += [(k, val(k, lambda k=k: sint(b[k]))) for k in ("in_head_in", "in_head_out")]
    it.append(("windows", val("windows", lambda: head(4, tau) + b"".join(
        b"\xa2" + text("left") + sint(l) + text("right") + sint(r) for l, r in b["windows"]))))
    it.append(("head_in_offsets", val("head_in_offsets", lambda: head(4, len(b["off_in"])) + b"".join(
        head(0, x) for x in b["off_in"]))))
    it.append(("head_out_offsets", val("head_out_offsets", lambda: head(4, len(b["off_out"])) + b"".join(
        head(0, x) for x in b["off_out"]))))
    it.append(("movement_log", val("movement_log", lambda: b"\xa1" + text("steps") + head(4, len(b["steps"])) +
                                   b"".join(b["steps"]))))
    it.append(("pre_tags", val("pre_tags", lambda: enc_tags(b.get("pre", zero)))))
    it.append(("post_tags", val("post_tags", lambda: enc_tags(b.get("post", zero)))))
    return it


def enc_block(b, raw=None, mutate=None):
    """mutate: [(key, value)] -> [(key, value)], for another key order or count."""
    it = block_items(b, raw)
    if mutate:
        it = mutate(it)
    return head(5, len(it)) + b"".join(text(k) + v for k, v in it)


def enc_blocks_file(blocks, count=None, indefinite=False):
    """blocks: encoded blocks. Returns (bytes, the offset of each block)."""
    out = bytearray(b"\x9f" if indefinite else head(4, len(blocks) if count is None else count))
    offs = []
    for blk in blocks:
        offs.append(len(out))
        out += blk
    if indefinite:
        out += b"\xff"
    return bytes(out), offs


@functools.lru_cache(maxsize=None)
def _steps64(tau, phase):
    return [enc_step(m, tp) for m, tp in designed_steps(64, tau, phase)]


def cached_step(i, tau, phase=0):
    """designed_steps' record i, encoded (the records repeat with period 64)."""
    return _steps64(tau, phase)[i % 64]


def designed_blocks(counts, tau, phase=0, walk=False, tags=False):
    """Block dicts over consistent step ranges. walk: every field cycles its
    type's extremes instead (for the decode-only entry: upload would refuse
    the ranges). tags: tag bytes over every head length."""
    out, s = [], 0
    for k, n in enumerate(counts):
        b = dict(version=1, block_id=k + 1, step_lo=s + 1, step_hi=s + n, ctrl_in=k % 3, ctrl_out=(k + 1) % 3,
                 in_head_in=k - 3, in_head_out=k - 2,
                 windows=[(-(k + r) % 40 - (30 if r % 2 else 0), (k * r) % 50) for r in range(tau)],
                 off_in=[(k + 2 * r) % 300 for r in range(tau)], off_out=[(3 * k + r) % 70000 for r in range(tau)],
                 steps=[cached_step(s + i, tau, phase) for i in range(n)])
        if walk:
            b.update(version=U16[k % 6], block_id=U32[(k + 1) % 8], step_lo=U64[(k + 2) % 10], step_hi=U64[(k + 3) % 10],
                     ctrl_in=U16[(k + 4) % 6], ctrl_out=U16[(k + 5) % 6], in_head_in=I64[k % 18],
                     in_head_out=I64[(k + 7) % 18],
                     windows=[(I64[(k + r) % 18], I64[(k + 5 * r + 9) % 18]) for r in range(tau)],
                     off_in=[U32[(k + r) % 8] for r in range(tau)], off_out=[U32[(k + 3 * r + 4) % 8] for r in range(tau)])
        if tags:
            b["pre"] = [[TAG_BYTES[(k + r + j) % 4] for j in range(16)] for r in range(tau)]
            b["post"] = [[TAG_BYTES[(k + 2 * r + 3 * j + 1) % 4] for j in range(16)] for r in range(tau)]
        out.append(b)
        s += n
    return out


def designed_file(counts, tau, phase=0, **kw):
    return enc_blocks_file([enc_block(b) for b in designed_blocks(counts, tau, phase, **kw)])[0]


# ------------------------------------------------------------------ corpus A
COUNT_CYCLE = [1, 2, 23, 24, 255, 256, 300]


@functools.lru_cache(maxsize=None)
def corpus_a_grid():
    """tau x B over the head-length thresholds; the step counts cycle, so that
    step_start is a real scan and every array-head length occurs (tau = 255:
    one or two steps per block)."""
    out = []
    for tau in (0, 1, 23, 24, 255):
        for B in (1, 23, 24, 255, 256):
            cyc = [1, 2] if tau == 255 else COUNT_CYCLE
            counts = [cyc[(k + B) % len(cyc)] for k in range(B)]
            out.append((f"grid_tau{tau}_B{B}", designed_file(counts, tau, phase=tau + B)))
    return out


@functools.lru_cache(maxsize=None)
def corpus_a_extremes():
    out = [(n, open(os.path.join(GOLDEN, n + ".cbor"), "rb").read()) for n in ("ref_blocks", "riscv_blocks")]
    out.append(("field_walk", designed_file([1 + k % 3 for k in range(36)], 2, 1, walk=True)))
    out.append(("tag_bytes", designed_file([2, 1, 3, 1, 24, 5], 3, 2, tags=True)))
    out += [(f"one_block_of_{n}_steps", designed_file([n], 1, n)) for n in (65535, 65536, 65537)]
    tl = tiling()
    out += [(f"B{B}_tau0", designed_file([1] * B, 0, B)) for B in (tl["scan_pass"] - 1, tl["scan_pass"],
                                                                    tl["scan_pass"] + 1)]
    big = designed_file([1100] * 64, 4, 5)
    assert len(big) > tl["scan_pass"] * tl["tile"], "the scan's second pass is not reached"
    out.append(("two_scan_passes", big))
    return out


STRADDLE_SEED, STRADDLE_B = 3, 14000


@functools.lru_cache(maxsize=None)
def straddle_file(seed=STRADDLE_SEED, nblocks=STRADDLE_B):
    """(bytes, block offsets, step offsets) of the seeded tau = 1 file whose
    signatures cross tile boundaries and whose blocks start at tile offsets 0
    and tile - 1 (asserted by the tests that use it)."""
    rnd = random.Random(seed)
    counts = [rnd.randint(1, 3) for _ in range(nblocks)]
    blocks = designed_blocks(counts, 1)
    for b in blocks:
        b["steps"] = [enc_step(rnd.choice(MOVES), [(rnd.choice(SYMS), rnd.choice(MOVES))]) for _ in b["steps"]]
        b["in_head_in"] = rnd.choice(I64)
    raw, offs = enc_blocks_file([enc_block(b) for b in blocks])
    soffs, p = [], raw.find(STEP_SIG)
    while p >= 0:
        soffs.append(p)
        p = raw.find(STEP_SIG, p + 1)
    return raw, offs, soffs


def straddle_facts(offs, soffs, tile):
    """(blocks and steps whose signature crosses a tile boundary, the tile offsets blocks start at)."""
    return ([o for o in offs if o % tile > tile - len(BLOCK_SIG)], [o for o in soffs if o % tile > tile - len(STEP_SIG)],
            {o % tile for o in offs})


# ------------------------------------------------------------------ corpus B
B_COUNTS, B_TAU = [3, 1, 4, 1, 5, 9, 2, 6], 2


def _with(k, **kw):
    """The B / C base file with block k encoded through enc_block(**kw)."""
    blocks = designed_blocks(B_COUNTS, B_TAU, 1)
    return enc_blocks_file([enc_block(b, **(kw if i == k else {})) for i, b in enumerate(blocks)])[0]


def _edit(k, **fields):
    blocks = designed_blocks(B_COUNTS, B_TAU, 1)
    blocks[k].update(fields)
    return enc_blocks_file([enc_block(b) for b in blocks])[0]


@functools.lru_cache(maxsize=None)
def corpus_b():
    """(name, bytes, None or (reason, index or None))."""
    blocks = designed_blocks(B_COUNTS, B_TAU, 1)
    out = []

    def swap(it):
        it = list(it)
        it[4], it[5] = it[5], it[4]  # ctrl_out before ctrl_in
        return it
    out.append(("key_order_swapped", _with(3, mutate=swap), ("block_head", 3)))
    out.append(("map15_unknown_trailing_key", _with(2, mutate=lambda it: it + [("extra", head(0, 7))]),
                ("block_candidates", None)))
    spell = text(b"x " + BLOCK_SIG + b" y " + STEP_SIG + b" z")
    out.append(("unknown_key_spelling_both_signatures", _with(2, mutate=lambda it: it[:1] + [("note", spell)] + it[1:]),
                None))
    zero = [[0] * 16] * B_TAU
    out.append(("byte_string_tags", _with(1, raw={"pre_tags": enc_tags(zero, as_bytes=True)}), ("block_tail", 1)))
    out.append(("map13_without_post_tags", _with(6, mutate=lambda it: it[:-1]), ("block_candidates", None)))
    out.append(("non_minimal_head_int", _with(4, raw={"block_id": head(0, 5, 2)}), ("block_head", 4)))
    wide = b"\x82" + (b"\x90" + head(0, 0, 1) + b"\x00" * 15) + (b"\x90" + b"\x00" * 16)
    out.append(("non_minimal_tag_int", _with(2, raw={"post_tags": wide}), ("block_tail", 2)))
    out.append(("indefinite_outer_array", enc_blocks_file([enc_block(b) for b in blocks], indefinite=True)[0],
                ("head", None)))
    out.append(("zero_step_block", _edit(5, steps=[]), ("block_head", 5)))
    out.append(("version_65536", _edit(1, version=65536), ("block_head", 1)))
    out.append(("block_id_2^32", _edit(7, block_id=1 << 32), ("block_head", 7)))
    out.append(("ctrl_in_65536", _edit(2, ctrl_in=65536), ("block_head", 2)))
    # block 4 starts at step 3 + 1 + 4 + 1 = 9: its second step is step 10 of the file
    st = list(blocks[4]["steps"])
    m, tp = designed_steps(11, B_TAU, 1)[10]
    assert -24 <= m < 24 and st[1] == enc_step(m, tp)
    st[1] = STEP_SIG + sint(m, 1) + text("tapes") + head(4, B_TAU) + b"".join(enc_tape(sy, v) for sy, v in tp)
    out.append(("non_minimal_step_int", _edit(4, steps=st), ("step", 10)))
    return out


# ------------------------------------------------------------------ corpus C
@functools.lru_cache(maxsize=None)
def corpus_c():
    blocks = designed_blocks([2] * 30, B_TAU, 2)
    enc = [enc_block(b) for b in blocks]
    good, offs = enc_blocks_file(enc)
    assert good[0] == 0x98  # a two-byte array head
    o = offs[20]
    key_at = good.index(text("in_head_in"), o)
    step_at = good.index(STEP_SIG, o)
    tag_at = good.index(text("pre_tags"), o) + 9 + 1 + 5
    wide = designed_blocks([2] * 30, B_TAU, 2)
    wide[20]["step_lo"] = 1 << 40
    wide_raw, wide_offs = enc_blocks_file([enc_block(b) for b in wide])
    value_at = wide_raw.index(text("step_lo"), wide_offs[20]) + 8
    out = [("cut_in_array_head", good[:1]), ("cut_in_key", good[:key_at + 4]), ("cut_in_head_value", wide_raw[:value_at + 4]),
           ("cut_in_step", good[:step_at + len(STEP_SIG) + 1 + 3]), ("cut_in_tag", good[:tag_at]),
           ("trailing_byte", good + b"\x00"), ("outer_count_B+1", enc_blocks_file(enc, count=31)[0]),
           ("outer_count_B-1", enc_blocks_file(enc, count=29)[0])]
    w = blocks[2]["windows"]
    out.append(("windows_tau+1", _edit(2, windows=designed_blocks(B_COUNTS, B_TAU + 1, 1)[2]["windows"])))
    out.append(("windows_tau-1", _edit(2, windows=w[:1])))
    out.append(("offset_2^32", _edit(2, off_in=[5, 1 << 32])))
    m, tp = designed_steps(3, B_TAU, 1)[2]
    for name, rec in (("step_with_tau-1_tapes", enc_step(m, tp[:1])), ("step_with_tau+1_tapes", enc_step(
            m, tp + [(None, 0)])), ("mv_128", enc_step(m, [(tp[0][0], 128), tp[1]]))):
        st = list(designed_blocks(B_COUNTS, B_TAU, 1)[2]["steps"])
        st[2] = rec
        out.append((name, _edit(2, steps=st)))
    out.append(("empty", b""))
    return out


@functools.lru_cache(maxsize=None)
def corpus_flips():
    """One changed byte at 64 seeded positions of a B = 6, tau = 2 file (the
    host decoder may accept some: equality is what counts)."""
    base = designed_file([4, 1, 7, 2, 3, 5], 2, 3)
    rnd = random.Random(21)
    out = []
    for _ in range(64):
        p, x = rnd.randrange(len(base)), rnd.randrange(1, 256)
        out.append((f"flip_at_{p}_xor_{x:02x}", base[:p] + bytes([base[p] ^ x]) + base[p + 1:]))
    return out


def arrays_of(blocks):
    """The arrays of a BlockSoA in ARRAYS' order, step_start without its last entry."""
    return {f: (np.asarray(getattr(blocks, f))[:-1] if f == "step_start" else np.asarray(getattr(blocks, f)))
            for f in ARRAYS}


def host_decode(product, raw):
    """("ok", BlockSoA) or ("err", code, message) of sezkp_blocks_decode_cbor."""
    try:
        return ("ok", product.BlockSoA.from_cbor(bytes(raw)))
    except product.SezkpError as e:
        return ("err", e.code, str(e))
