"""Block-file CBOR decoded on the device, the host side (CPU only).

* the seven new entry points are exported, bound and in the header, ABI still
  4, the new info struct's size pinned; null arguments are SEZKP_E_INVALID and
  a file the host decoder refuses is SEZKP_E_DECODE with its message, all
  without a device;
* sezkp_blocks_cbor_head on both reference fixtures and on heads that leave
  the canonical form;
* csrc/blocks_cbor_plan.h through the stand-alone tools/cbor_check.cpp (mode
  `blocks`), built with the address and undefined-behaviour sanitizers (nothing
  is loaded into Python): the device decoder's own mark, compact, heads, steps
  and chain passes, index by index, over corpora A, B and C
  (tests/blocks_cbor_corpus.py) and over every prefix of a small file. The tool
  never takes a file the host decoder refuses, decodes what it takes as the
  host decoder does, takes every file of A, and the sanitizers stay silent:
  this is the out-of-bounds check of every read and write a lane makes."""
import ctypes as C
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import blocks_cbor_corpus as K
from conftest import GOLDEN, PKG, ROOT

NEW_SYMBOLS = ["sezkp_ctx_ingest_blocks_cbor", "sezkp_ctx_upload_ingested", "sezkp_ctx_upload_blocks_cbor",
               "sezkp_ctx_decode_blocks_cbor", "sezkp_stark_v1_prove_blocks_cbor", "sezkp_blocks_cbor_head",
               "sezkp_ctx_blocks_ingest_stats"]
REF = open(os.path.join(GOLDEN, "ref_blocks.cbor"), "rb").read()
RISCV = open(os.path.join(GOLDEN, "riscv_blocks.cbor"), "rb").read()


def test_blocks_cbor_entry_points_are_exported(product):
    lib = C.CDLL(product.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "sezkp_stark.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in product._lib.EXPORTS and s + "(" in hdr, s
    assert lib.sezkp_abi_version() == 4
    assert C.sizeof(product._lib.BlocksIngestInfo) == 80
    assert C.sizeof(product._lib.TraceIngestInfo) == 72  # the sibling's stays as it is
    for name in ("ProverContext.ingest_blocks_cbor", "ProverContext.upload_ingested", "ProverContext.upload_blocks_cbor",
                 "ProverContext.decode_blocks_cbor", "ProverContext.blocks_ingest_stats",
                 "ShardedProverContext.upload_blocks_cbor", "StarkV1.prove_blocks_cbor"):
        cls, meth = name.split(".")
        assert callable(getattr(getattr(product, cls), meth)), name
    assert callable(product.blocks_cbor_head)


def test_bad_arguments_are_answered_without_a_device(product):
    lib = product.lib
    err = C.create_string_buffer(512)
    buf = C.create_string_buffer(REF, len(REF))
    p = C.addressof(buf)
    h = C.c_void_p()
    root = b"\x00" * 32
    # no context: null argument, whatever else is given
    assert lib.sezkp_ctx_ingest_blocks_cbor(None, p, len(REF), C.byref(h), err, 512) == -1 and not h.value
    assert err.value == b"null argument"
    assert lib.sezkp_ctx_upload_ingested(None, err, 512) == -1
    assert lib.sezkp_ctx_upload_blocks_cbor(None, p, len(REF), err, 512) == -1
    assert lib.sezkp_ctx_upload_blocks_cbor(None, None, 0, err, 512) == -1
    assert lib.sezkp_ctx_decode_blocks_cbor(None, p, len(REF), C.byref(h), err, 512) == -1 and not h.value
    assert lib.sezkp_ctx_blocks_ingest_stats(None, C.byref(product._lib.BlocksIngestInfo())) == -1
    # the stateless form: every argument check comes before sezkp_ctx_create
    pb = product._lib.Buf()

    def stateless(data, n, rt=root, out=pb):
        rc = lib.sezkp_stark_v1_prove_blocks_cbor(data, n, rt, 0, C.byref(out) if out is not None else None, err, 512)
        assert pb.len == 0 and not pb.data
        return rc, err.value.decode()
    assert stateless(None, 0) == (-1, "null argument")
    assert stateless(None, len(REF)) == (-1, "null argument")
    assert stateless(p, len(REF), out=None) == (-1, "null argument")
    assert stateless(p, len(REF), rt=None) == (-1, "null argument")
    # bytes the host decoder refuses: its code and message, no device needed
    # (an empty file at a non-null address is such a file)
    for raw in (b"", b"\xa0", REF[:7], b"\x81\xa0\x00"):
        keep = C.create_string_buffer(raw, max(1, len(raw)))
        want = K.host_decode(product, raw)
        rc, msg = stateless(C.addressof(keep), len(raw))
        assert want[0] == "err" and (rc, f"[{rc}] {msg}") == want[1:], raw


def test_blocks_cbor_head(product):
    # each fixture: 88 AE 67 "version", 8 blocks of tau = 2
    assert REF[:3] == RISCV[:3] == b"\x88\xae\x67"
    assert REF.count(K.BLOCK_SIG) == RISCV.count(K.BLOCK_SIG) == 8
    assert (REF.count(K.STEP_SIG), RISCV.count(K.STEP_SIG)) == (64, 32)
    assert product.blocks_cbor_head(REF) == (8, 2, 1) and product.blocks_cbor_head(RISCV) == (8, 2, 1)
    blocks = K.designed_blocks([2] * 30, 3)
    enc = [K.enc_block(b) for b in blocks]
    good = K.enc_blocks_file(enc)[0]
    assert product.blocks_cbor_head(good) == (30, 3, 2)
    assert product.blocks_cbor_head(K.enc_blocks_file(enc, count=29)[0]) == (29, 3, 2)  # the head alone
    assert product.blocks_cbor_head(K.designed_file([1], 255)) == (1, 255, 1)
    assert product.blocks_cbor_head(K.designed_file([1], 0)) == (1, 0, 1)

    def first(**kw):
        return K.enc_blocks_file([K.enc_block(blocks[0], **kw)] + enc[1:])[0]
    for name, raw in [("empty", b""), ("empty array", b"\x80"), ("a map", b"\xa0"), ("cut in block 0", good[:60]),
                      ("indefinite", K.enc_blocks_file(enc, indefinite=True)[0]),
                      ("non-minimal count", K.head(4, 30, 2) + good[2:]),
                      ("more blocks than bytes", K.head(4, 1 << 30) + good[2:]),
                      ("one block too many for the bytes", K.head(4, len(good) // 220 + 1) + good[2:]),
                      ("non-minimal version", first(raw={"version": K.head(0, 1, 1)})),
                      ("version 65536", first(raw={"version": K.head(0, 65536)})),
                      ("negative block_id", first(raw={"block_id": K.sint(-1)})),
                      ("text step_lo", first(raw={"step_lo": K.text("1")})),
                      ("key order", first(mutate=lambda it: [it[1], it[0]] + it[2:])),
                      ("fifteen keys", first(mutate=lambda it: it + [("x", b"\x00")])),
                      ("zero steps", K.enc_blocks_file([K.enc_block(dict(blocks[0], steps=[]))] + enc[1:])[0]),
                      ("tau 256", K.designed_file([1], 256))]:
        assert product.blocks_cbor_head(raw) is None, name
    for name, raw, pin in K.corpus_b():
        want = None if name == "indefinite_outer_array" else (8, 2, 1)
        assert product.blocks_cbor_head(raw) == want, name
    # null arguments: 0
    nb, ta, fo = C.c_uint32(), C.c_uint32(), C.c_uint64()
    assert product.lib.sezkp_blocks_cbor_head(None, 0, C.byref(nb), C.byref(ta), C.byref(fo)) == 0
    assert product.lib.sezkp_blocks_cbor_head(REF, len(REF), None, C.byref(ta), C.byref(fo)) == 0


# ------------------------------------------------------------ the check tool
@pytest.fixture(scope="module")
def check_tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cbor_check") / "cbor_check")
    csrc = os.path.join(PKG, "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "cbor_check.cpp"),
                    os.path.join(csrc, "codec.cpp"), os.path.join(csrc, "host_crypto.cpp"), "-pthread"], check=True)
    return exe


def run_tool(exe, files):
    """One verdict per file: ("decline", reason) or ("device", {array: (count, crc32)})."""
    feed = b"".join(struct.pack("<Q", len(f)) + f for f in files)
    r = subprocess.run([exe, "blocks", "batch"], input=feed, capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stderr == b"", r.stderr[-2000:]  # a sanitizer report
    lines = r.stdout.decode().splitlines()
    out, i = [], 0
    while i < len(lines):
        w = lines[i].split()
        if w[0] == "decline":
            out.append(("decline", " ".join(w[1:])))
            i += 1
            continue
        assert w[0] == "device", lines[i][:80]
        arrs = {}
        for k, name in enumerate(K.ARRAYS):
            f = lines[i + 1 + k].split()
            assert f[0] == name
            arrs[name] = (int(f[1]), int(f[2]))
        out.append(("device", arrs))
        i += 1 + len(K.ARRAYS)
    assert len(out) == len(files)
    return out


def check_against_host(product, name, verdict, raw, must_take=False, pin=None):
    want = K.host_decode(product, raw)
    if must_take:
        assert verdict[0] == "device", (name, verdict)
    if want[0] == "err":
        # never a file the host decoder refuses
        assert verdict[0] == "decline", (name, want[1:])
    if pin is not None:
        reason, index = pin
        assert verdict == ("decline", reason if index is None else f"{reason} {index}"), name
    if verdict[0] == "device":
        assert want[0] == "ok", name
        for f, a in K.arrays_of(want[1]).items():
            assert verdict[1][f] == (a.size, zlib.crc32(a.tobytes())), f"{name}: {f}"


def test_tool_reports_the_bounds(check_tool):
    r = subprocess.run([check_tool, "blocks", "tiling"], capture_output=True, text=True, check=True)
    tl = json.loads(r.stdout)
    assert tl["tile"] == K.tiling()["tile"] and (tl["block_sig_len"], tl["step_sig_len"]) == (9, 10)
    # the shortest canonical block of each tau is exactly the bound B is checked against
    for tau, want in zip((0, 8, 24), tl["block_min"]):
        b = dict(version=0, block_id=0, step_lo=0, step_hi=0, ctrl_in=0, ctrl_out=0, in_head_in=0, in_head_out=0,
                 windows=[(0, 0)] * tau, off_in=[0] * tau, off_out=[0] * tau,
                 steps=[K.enc_step(0, [(None, 0)] * tau)])
        assert len(K.enc_block(b)) == want, tau


@pytest.mark.parametrize("tau", [0, 1, 23, 24, 255])
def test_corpus_a_grid_is_taken_and_decoded_as_the_host_does(product, check_tool, tau):
    files = [(n, f) for n, f in K.corpus_a_grid() if n.startswith(f"grid_tau{tau}_")]
    assert len(files) == 5
    for (name, raw), v in zip(files, run_tool(check_tool, [f for _, f in files])):
        check_against_host(product, name, v, raw, must_take=True)


def test_corpus_a_extremes_are_taken_and_decoded_as_the_host_does(product, check_tool):
    files = K.corpus_a_extremes()
    for (name, raw), v in zip(files, run_tool(check_tool, [f for _, f in files])):
        check_against_host(product, name, v, raw, must_take=True)


def test_corpus_a_straddle_file_is_taken_and_decoded_as_the_host_does(product, check_tool):
    raw_s, offs, soffs = K.straddle_file()
    tile = K.tiling()["tile"]
    bcross, scross, rel = K.straddle_facts(offs, soffs, tile)
    assert bcross and scross and 0 in rel and tile - 1 in rel
    (v,) = run_tool(check_tool, [raw_s])
    check_against_host(product, "straddle", v, raw_s, must_take=True)


def test_corpus_b_is_declined_or_decoded_alike(product, check_tool):
    files = K.corpus_b()
    for (name, raw, pin), v in zip(files, run_tool(check_tool, [f for _, f, _ in files])):
        assert K.host_decode(product, raw)[0] == "ok", name  # B: files the host decoder accepts
        check_against_host(product, name, v, raw, pin=pin)


def test_corpus_c_is_never_taken(product, check_tool):
    files = K.corpus_c()
    for (name, raw), v in zip(files, run_tool(check_tool, [f for _, f in files])):
        assert K.host_decode(product, raw)[0] == "err", name  # C: files the host decoder refuses
        check_against_host(product, name, v, raw)
    flips = K.corpus_flips()
    for (name, raw), v in zip(flips, run_tool(check_tool, [f for _, f in flips])):
        check_against_host(product, name, v, raw)


def test_every_prefix_of_a_small_file_is_declined_without_a_stray_read(product, check_tool):
    whole = K.designed_file([2, 1, 3], 2, 4, tags=True)
    cuts = [whole[:n] for n in range(len(whole))]
    for n, v in enumerate(run_tool(check_tool, cuts)):
        assert v[0] == "decline", n
        check_against_host(product, f"prefix {n}", v, cuts[n])
    (v,) = run_tool(check_tool, [whole])
    check_against_host(product, "whole", v, whole, must_take=True)
