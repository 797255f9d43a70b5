"""Block files and TraceFiles encoded on the device, the host side (CPU only).

* the four new entry points are exported, bound and in the header, ABI still
  4, the info struct's size pinned; null arguments are SEZKP_E_INVALID without
  a device;
* csrc/cbor_emit_plan.h through the stand-alone tools/cbor_encode_check.cpp,
  built with the address and undefined-behaviour sanitizers (nothing is loaded
  into Python): the device encoder's own length, step and block passes, index
  by index, into a file of exactly the scanned length, over the corpus of
  tests/cbor_encode_corpus.py (the one tests/test_gpu_cbor_encode.py feeds the
  device). Every byte is written exactly once, the file is the host encoder's
  (encode_blocks_cbor / encode_trace_cbor), and the sanitizers stay silent:
  this is the out-of-bounds check of every read and write a lane makes."""
import ctypes as C
import json
import os
import subprocess

import pytest

import cbor_encode_corpus as K
from conftest import PKG, ROOT

NEW_SYMBOLS = ["sezkp_ctx_encode_trace_blocks_cbor", "sezkp_ctx_encode_blocks_cbor", "sezkp_ctx_encode_trace_cbor",
               "sezkp_ctx_encode_stats"]


def test_encode_entry_points_are_exported(product):
    lib = C.CDLL(product.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "sezkp_stark.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in product._lib.EXPORTS and s + "(" in hdr, s
    assert lib.sezkp_abi_version() == 4
    assert C.sizeof(product._lib.EncodeInfo) == 56
    for meth in ("blocks_cbor", "encode_blocks_cbor", "trace_cbor", "encode_stats"):
        assert callable(getattr(product.ProverContext, meth)), meth


def test_null_arguments_are_answered_without_a_device(product):
    lib = product.lib
    err = C.create_string_buffer(512)
    buf = product._lib.Buf()
    view = K.to_blocks(product, K.view([2, 1], 2)).view()
    assert lib.sezkp_ctx_encode_trace_blocks_cbor(None, C.byref(buf), err, 512) == -1
    assert err.value == b"null argument"
    assert lib.sezkp_ctx_encode_blocks_cbor(None, C.byref(view), C.byref(buf), err, 512) == -1
    assert lib.sezkp_ctx_encode_trace_cbor(None, None, C.byref(buf), err, 512) == -1
    assert lib.sezkp_ctx_encode_stats(None, C.byref(product._lib.EncodeInfo())) == -1
    assert buf.len == 0 and not buf.data


@pytest.fixture(scope="module")
def check_tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cbor_encode_check") / "cbor_encode_check")
    csrc = os.path.join(PKG, "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "cbor_encode_check.cpp"),
                    os.path.join(csrc, "codec.cpp"), os.path.join(csrc, "host_crypto.cpp"), "-pthread"], check=True)
    return exe


def run_tool(exe, names, records):
    r = subprocess.run([exe], input=b"".join(records), capture_output=True)
    lines = r.stdout.decode().splitlines()
    assert r.stderr == b"", r.stderr[-2000:]  # a sanitizer report
    assert r.returncode == 0 and len(lines) == len(names), (r.returncode, lines[-3:])
    for name, line in zip(names, lines):
        assert line.startswith("ok "), (name, line)
    return [int(line.split()[1]) for line in lines]


def test_tool_reports_the_tiling(check_tool):
    r = subprocess.run([check_tool, "tiling"], capture_output=True, text=True, check=True)
    tl = json.loads(r.stdout)
    assert (tl["threads"], tl["lds"]) == (256, 48 << 10) and tl["step_max"] == [19, 139, 3845]
    steps = {int(k): v for k, v in tl["tile_steps"].items()}
    assert all(steps[tau] == K.tile_steps(tau) for tau in range(256))
    # the corpus has both sides of every tape count at which the steps per tile change
    changes = [tau for tau in range(1, 256) if steps[tau] != steps[tau - 1]]
    assert changes and all(tau in K.TAUS and tau - 1 in K.TAUS for tau in changes)
    assert all(steps[tau] * (18 + (1 if tau < 24 else 2) + 15 * tau) <= tl["lds"] for tau in range(256))


def test_block_views_are_written_as_the_host_encoder_writes_them(product, check_tool):
    cases = K.block_views()
    lens = run_tool(check_tool, [n for n, _ in cases], [K.block_record(v) for _, v in cases])
    for (name, v), n in zip(cases, lens):
        assert n == len(K.to_blocks(product, v).to_cbor()), name


def test_the_case_that_crosses_the_scan_pass(check_tool):
    v = K.scan_pass_view()
    assert -(-int(v["step_start"][-1]) // K.tile_steps(1)) > 1024
    run_tool(check_tool, ["scan_pass"], [K.block_record(v)])


def test_traces_are_written_as_the_host_encoder_writes_them(product, check_tool):
    cases = K.trace_cases()
    lens = run_tool(check_tool, [n for n, _, _ in cases], [K.trace_record(s, tau) for _, s, tau in cases])
    for (name, s, tau), n in zip(cases, lens):
        assert n == len(product.Trace(s["input_mv"], s["mv"], s["has_write"], s["wsym"]).to_cbor()), name


def test_partitioned_traces_are_written_with_the_fields_of_partition_trace(check_tool):
    cases = K.uniform_cases()
    run_tool(check_tool, [n for n, _, _, _ in cases], [K.uniform_record(v, t, b) for _, t, b, v in cases])
