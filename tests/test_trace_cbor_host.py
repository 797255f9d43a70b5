"""TraceFile CBOR decoded on the device, the host side (CPU only).

* the new entry points are exported and bound, ABI still 4; null arguments
  and b = 0 are SEZKP_E_INVALID, and a file the host decoder refuses is
  SEZKP_E_DECODE with its message, all without a device;
* sezkp_trace_cbor_head on the fixture and on heads that leave the canonical
  form;
* csrc/trace_cbor_plan.h through the stand-alone tools/cbor_check.cpp (mode
  `trace`), built with the address and undefined-behaviour sanitizers (nothing
  is loaded into Python): the device decoder's own mark, compact and parse
  passes, index by index, over corpora A, B and C (tests/trace_cbor_corpus.py)
  and over every prefix of a small file. The tool never takes a file the host
  decoder refuses, decodes what it takes as the host decoder does, takes every
  file of A, declines the pinned files of B for the reason the product gives
  (they share trace_cbor_decide), and the sanitizers stay silent: this is the
  out-of-bounds check of every read and write a lane makes."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import trace_cbor_corpus as K
from conftest import GOLDEN, PKG, ROOT

NEW_SYMBOLS = ["sezkp_ctx_upload_trace_cbor", "sezkp_ctx_decode_trace_cbor", "sezkp_stark_v1_prove_trace_cbor",
               "sezkp_trace_cbor_head", "sezkp_ctx_trace_ingest_stats"]
FIXTURE = open(os.path.join(GOLDEN, "riscv_trace.cbor"), "rb").read()


def test_trace_cbor_entry_points_are_exported(product):
    lib = C.CDLL(product.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "sezkp_stark.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in product._lib.EXPORTS and s + "(" in hdr, s
    assert lib.sezkp_abi_version() == 4
    assert C.sizeof(product._lib.TraceIngestInfo) == 72
    for name in ("ProverContext.upload_trace_cbor", "ProverContext.decode_trace_cbor",
                 "ProverContext.trace_ingest_stats", "StarkV1.prove_trace_cbor"):
        cls, meth = name.split(".")
        assert callable(getattr(getattr(product, cls), meth)), name


def test_bad_arguments_are_answered_without_a_device(product):
    lib = product.lib
    err = C.create_string_buffer(512)
    buf = C.create_string_buffer(FIXTURE, len(FIXTURE))
    p = C.addressof(buf)
    h = C.c_void_p()
    # no context: null argument, whatever else is given
    assert lib.sezkp_ctx_upload_trace_cbor(None, p, len(FIXTURE), 4, err, 512) == -1 and err.value == b"null argument"
    assert lib.sezkp_ctx_upload_trace_cbor(None, None, 0, 4, err, 512) == -1
    assert lib.sezkp_ctx_upload_trace_cbor(None, p, len(FIXTURE), 0, err, 512) == -1
    assert lib.sezkp_ctx_decode_trace_cbor(None, p, len(FIXTURE), C.byref(h), err, 512) == -1 and not h.value
    assert lib.sezkp_ctx_trace_ingest_stats(None, C.byref(product._lib.TraceIngestInfo())) == -1
    # the stateless form: every argument check comes before sezkp_ctx_create
    pb = product._lib.Buf()
    root = C.create_string_buffer(32)

    def stateless(data, n, b, out=pb):
        rc = lib.sezkp_stark_v1_prove_trace_cbor(data, n, b, 0, C.byref(out) if out is not None else None, root, err,
                                                 512)
        assert pb.len == 0 and not pb.data
        return rc, err.value.decode()
    assert stateless(None, 0, 4) == (-1, "null argument")
    assert stateless(None, len(FIXTURE), 4) == (-1, "null argument")
    assert stateless(p, len(FIXTURE), 4, out=None) == (-1, "null argument")
    assert stateless(p, len(FIXTURE), 0) == (-1, "trace view: b (steps per block) must be at least 1")
    # bytes the host decoder refuses: its code and message, no device needed
    # (an empty file at a non-null address is such a file)
    for raw in (b"", b"\xa0", FIXTURE[:7]):
        keep = C.create_string_buffer(raw, max(1, len(raw)))
        want = K.host_decode(product, raw)
        rc, msg = stateless(C.addressof(keep), len(raw), 4)
        assert want[0] == "err" and (rc, f"[{rc}] {msg}") == want[1:], raw


def test_trace_cbor_head(product):
    assert product.trace_cbor_head(FIXTURE) == (32, 2, 23)
    tau = 2
    body = b"".join(K.enc_step(m, tp) for m, tp in K.designed_steps(5, tau))
    pre = b"\xa4" + K.text("version")

    def file(version=K.head(0, 1), tau_item=K.head(0, tau), steps=K.head(4, 5), keys=("tau", "steps")):
        return pre + version + K.text(keys[0]) + tau_item + K.text(keys[1]) + steps + body + K.text("meta") + b"\xf6"
    off = len(file()) - len(body) - 6
    assert product.trace_cbor_head(file()) == (5, tau, off)
    assert product.trace_cbor_head(file(version=K.head(0, 1000))) == (5, tau, off + 2)
    assert product.trace_cbor_head(file(steps=K.head(4, 4))) == (4, tau, off)  # the head alone: the body is not read
    assert product.trace_cbor_head(file(tau_item=K.head(0, 255), steps=K.head(4, 0))) == (0, 255, off + 1)
    for name, raw in [("empty", b""), ("a0", b"\xa0"), ("head only, cut", file()[:off - 1]),
                      ("indefinite steps", file(steps=b"\x9f")), ("tau 256", file(tau_item=K.head(0, 256))),
                      ("non-minimal tau", file(tau_item=K.head(0, tau, 1))),
                      ("non-minimal count", file(steps=K.head(4, 5, 2))),
                      ("negative tau", file(tau_item=K.sint(-1))), ("text version", file(version=K.text("1"))),
                      ("more steps than bytes", file(steps=K.head(4, 1 << 40))),
                      ("one step too many for the bytes", file(steps=K.head(4, (len(body) + 6) // 42 + 1))),
                      ("other key", file(keys=("tau", "stepz"))), ("three keys", b"\xa3" + file()[1:]),
                      ("key order", b"\xa4" + K.text("tau") + K.head(0, tau) + file()[9:])]:
        assert product.trace_cbor_head(raw) is None, name
    for name, raw, _pin in K.corpus_b():
        want = None if name in ("indefinite_steps", "top_level_key_order") else (40, 2, 23)
        assert product.trace_cbor_head(raw) == want, name
    # null arguments: 0
    t, ta, so = C.c_uint64(), C.c_uint32(), C.c_uint64()
    assert product.lib.sezkp_trace_cbor_head(None, 0, C.byref(t), C.byref(ta), C.byref(so)) == 0
    assert product.lib.sezkp_trace_cbor_head(FIXTURE, len(FIXTURE), None, C.byref(ta), C.byref(so)) == 0


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
    """One verdict per file: ("decline", reason) or ("device", arrays)."""
    feed = b"".join(struct.pack("<Q", len(f)) + f for f in files)
    r = subprocess.run([exe, "trace", "batch"], input=feed, capture_output=True)
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
        t, tau = int(w[1][2:]), int(w[2][4:])
        arrs = []
        for k, (name, dt) in enumerate((("input_mv", np.int8), ("mv", np.int8), ("has_write", np.uint8),
                                        ("wsym", np.uint16))):
            f = lines[i + 1 + k].split()
            assert f[0] == name
            a = np.array(f[1:], dtype=np.int64).astype(dt)
            arrs.append(a if k == 0 else a.reshape(t, tau))
        out.append(("device", tuple(arrs)))
        i += 5
    assert len(out) == len(files)
    return out


def check_against_host(product, name, verdict, raw, must_take=False, must_decline=False):
    want = K.host_decode(product, raw)
    if must_take:
        assert verdict[0] == "device", (name, verdict)
    if must_decline or want[0] == "err":
        # never a file the host decoder refuses
        assert verdict[0] == "decline", (name, want[1:] if want[0] == "err" else "pinned to the host")
    if verdict[0] == "device":
        assert want[0] == "ok", name
        for got, ref, arr in zip(verdict[1], want[1], ("input_mv", "mv", "has_write", "wsym")):
            np.testing.assert_array_equal(got, ref, err_msg=f"{name}: {arr}")


def test_tool_reports_the_tiling(check_tool):
    import json
    r = subprocess.run([check_tool, "trace", "tiling"], capture_output=True, text=True, check=True)
    tl = json.loads(r.stdout)
    assert {k: tl[k] for k in K.tiling()} == K.tiling()
    assert (tl["step_min"], tl["step_max"]) == ([18, 114, 307], [19, 139, 380])  # 17 + h + 12 tau, 18 + h + 15 tau


def test_corpus_a_is_taken_and_decoded_as_the_host_does(product, check_tool):
    raw_s, offs = K.straddle_file()
    tile = K.tiling()["tile"]
    crossing, rel = K.straddle_facts(offs, tile)
    assert crossing and 0 in rel and tile - 1 in rel
    files = K.corpus_a_small() + K.corpus_a_extremes() + [("straddle", raw_s)] + K.corpus_a_encoded(product)
    for (name, raw), v in zip(files, run_tool(check_tool, [f for _, f in files])):
        check_against_host(product, name, v, raw, must_take=True)


def test_corpus_b_is_declined_or_decoded_alike(product, check_tool):
    files = K.corpus_b()
    verdicts = run_tool(check_tool, [f for _, f, _ in files])
    for (name, raw, pinned), v in zip(files, verdicts):
        assert K.host_decode(product, raw)[0] == "ok", name  # B: files the host decoder accepts
        check_against_host(product, name, v, raw, must_decline=pinned)
    # the reasons tests/test_gpu_trace_cbor.py pins on the device: the tool decides through
    # trace_cbor_decide, as the product does
    got = {name: v for (name, _, _), v in zip(files, verdicts)}
    assert got["non_minimal_int"] == ("decline", "step 7")
    assert got["unknown_tape_key"] == ("decline", "step 9")
    assert got["indefinite_steps"] == got["top_level_key_order"] == ("decline", "head")
    assert got["meta_map"] == ("decline", "tail")
    assert got["tapes_before_input_mv"][0] == "decline"
    assert got["tapes_before_input_mv"][1].split()[0] in ("candidates", "step", "chain")


def test_corpus_c_is_never_taken(product, check_tool):
    files = K.corpus_c()
    for (name, raw), v in zip(files, run_tool(check_tool, [f for _, f in files])):
        assert K.host_decode(product, raw)[0] == "err", name  # C: files the host decoder refuses
        check_against_host(product, name, v, raw)
    flips = K.corpus_flips()
    for (name, raw), v in zip(flips, run_tool(check_tool, [f for _, f in flips])):
        check_against_host(product, name, v, raw)


def test_every_prefix_of_a_small_file_is_declined_without_a_stray_read(product, check_tool):
    whole = K.designed_file(3, 2, 4)
    cuts = [whole[:n] for n in range(len(whole))]
    for n, v in enumerate(run_tool(check_tool, cuts)):
        check_against_host(product, f"prefix {n}", v, cuts[n], must_decline=True)
    (v,) = run_tool(check_tool, [whole])
    check_against_host(product, "whole", v, whole, must_take=True)
