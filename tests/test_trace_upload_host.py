"""Proving from a raw trace, the host side (CPU only, no device call).

* the trace entry points are exported and bound, ABI still 4;
* sezkp_stark_v1_prove_trace answers bad arguments and shapes before any
  device is touched, with the texts of the block upload;
* TraceFile CBOR: the reference's riscv_trace.cbor decodes to its own
  generate_trace(32, 2) and encodes back byte for byte;
* `sezkp-cli prove --trace` usage errors;
* csrc/trace_plan.h through the stand-alone tools/trace_plan_check.cpp, built
  with the address and undefined-behaviour sanitizers (nothing is loaded into
  Python): the manifest leaf message hashes to BlockSoA.leaf_hashes() on both
  sides of the one-chunk condition, and the scan tiling tiles [0, nblk)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT

NEW_SYMBOLS = ["sezkp_ctx_upload_trace", "sezkp_ctx_stage_trace", "sezkp_ctx_manifest_root",
               "sezkp_ctx_manifest_leaves", "sezkp_ctx_trace_blocks", "sezkp_stark_v1_prove_trace",
               "sezkp_trace_decode_cbor", "sezkp_trace_encode_cbor", "sezkp_trace_view_of", "sezkp_trace_free"]
CLI = os.path.join(PKG, "bin", "sezkp-cli")


def test_trace_entry_points_are_exported(product):
    lib = C.CDLL(product.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "sezkp_stark.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in product._lib.EXPORTS and s + "(" in hdr, s
    assert "#define SEZKP_FLAG_ROOT_FROM_TRACE 2u" in hdr
    assert product._lib.SEZKP_FLAG_ROOT_FROM_TRACE == 2
    assert lib.sezkp_abi_version() == 4


# ------------------------------------------------------------ argument checks
def _prove_trace(product, view):
    pb = product._lib.Buf()
    root = C.create_string_buffer(32)
    err = C.create_string_buffer(512)
    rc = product.lib.sezkp_stark_v1_prove_trace(view, 0, C.byref(pb), root, err, 512)
    assert pb.len == 0 and not pb.data
    return rc, err.value.decode()


def _view(product, t, tau, b, null=None):
    tr = product.simulate(t, tau, 3)
    v, keep = product.trace.trace_view(*tr, b=b)
    if null:
        setattr(v, null, None)
    return v, keep


@pytest.mark.parametrize("case,text", [
    ("null_view", "null argument"),
    ("null_array", "trace view: null step array"),
    ("b0", "trace view: b (steps per block) must be at least 1"),
    ("tau256", "trace view: tau must be at most 255 (got 256)"),
    ("t3000", "n_base must be a power of two (got 3000)"),
    ("t0", "n_base must be a power of two (got 0)"),
])
def test_prove_trace_rejects_bad_input_before_any_device(product, case, text):
    """No device is needed for these: an environment that hides every GPU
    still gets the same answers (the child sees no HIP device at all)."""
    if case == "null_view":
        rc, msg = _prove_trace(product, None)
    else:
        t, tau, b, null = {"null_array": (16, 2, 4, "has_write"), "b0": (16, 2, 0, None), "tau256": (4, 256, 2, None),
                           "t3000": (3000, 2, 8, None), "t0": (0, 2, 8, None)}[case]
        v, _keep = _view(product, t, tau, b, null)
        rc, msg = _prove_trace(product, C.byref(v))
    assert rc == -1 and msg == text


# ------------------------------------------------------------ trace CBOR
def test_trace_cbor_decodes_to_the_reference_generator(product):
    raw = open(os.path.join(GOLDEN, "riscv_trace.cbor"), "rb").read()
    tr = product.Trace.from_cbor(raw)
    assert (tr.t, tr.tau) == (32, 2)
    for got, want, name in zip(tr.arrays(), product.reference_trace(32, 2), ("input_mv", "mv", "has_write", "wsym")):
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert got.dtype == want.dtype
    assert tr.to_cbor() == raw


def test_trace_cbor_round_trips_wide_values(product):
    """Moves over the whole i8 range and symbols over the whole u16 range."""
    t, tau = 40, 3
    imv = np.array([-128, 127, -1, 0, 23, -24, 24, -25] * 5, np.int8)
    mv = (np.arange(t * tau, dtype=np.int64).reshape(t, tau) * 37 % 256 - 128).astype(np.int8)
    hw = (np.arange(t * tau).reshape(t, tau) % 3 == 0).astype(np.uint8)
    ws = ((np.arange(t * tau, dtype=np.int64).reshape(t, tau) * 4099) % 65536).astype(np.uint16) * hw
    tr = product.Trace(imv, mv, hw, ws)
    back = product.Trace.from_cbor(tr.to_cbor())
    for got, want in zip(back.arrays(), tr.arrays()):
        np.testing.assert_array_equal(got, want)
    assert product.Trace(imv[:0], mv[:0], hw[:0], ws[:0]).to_cbor() == bytes.fromhex(
        "a46776657273696f6e016374617503657374657073806" "46d657461f6")


def test_trace_cbor_decode_errors_are_reported(product):
    raw = open(os.path.join(GOLDEN, "riscv_trace.cbor"), "rb").read()
    for bad in (raw[:100], raw[:-1], b"\xa0", b"", raw + b"\x00"):
        with pytest.raises(product.SezkpError):
            product.Trace.from_cbor(bad)


# ------------------------------------------------------------ CLI
@pytest.mark.parametrize("args,text", [
    (["--blocks", "b.cbor", "--trace", "t.cbor", "--b", "4", "--out", "p.cbor"], "mutually exclusive"),
    (["--trace", "t.json", "--b", "4", "--out", "p.cbor"], "--trace reads a .cbor trace file"),
    (["--trace", "t", "--b", "4", "--out", "p.cbor"], "--trace reads a .cbor trace file"),
    (["--trace", "t.cbor", "--out", "p.cbor"], "needs --b and --out"),
    (["--trace", "t.cbor", "--b", "4"], "needs --b and --out"),
    (["--trace", "t.cbor", "--b", "0", "--out", "p.cbor"], "--b must be in"),
    (["--trace", "t.cbor", "--b", "4", "--out", "p.cbor", "--out-blocks", "b.json"], "--out-blocks must end in"),
])
def test_cli_prove_trace_usage_errors(args, text, tmp_path):
    r = subprocess.run([CLI, "prove", "--backend", "stark"] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert text in r.stderr
    assert os.listdir(tmp_path) == []


def test_cli_prove_trace_reports_a_bad_trace_file(tmp_path):
    bad = tmp_path / "t.cbor"
    bad.write_bytes(b"\xa0")
    r = subprocess.run([CLI, "prove", "--backend", "stark", "--trace", str(bad), "--b", "4", "--out",
                        str(tmp_path / "p.cbor")], capture_output=True, text=True)
    assert r.returncode == 1 and "reading trace" in r.stderr and "trace without tau" in r.stderr
    assert not (tmp_path / "p.cbor").exists()


def test_cli_simulate_still_writes_out_blocks(tmp_path):
    """--out-blocks keeps its meaning for simulate (it gained one for prove --trace)."""
    out = tmp_path / "b.cbor"
    r = subprocess.run([CLI, "simulate", "--t", "64", "--b", "8", "--tau", "2", "--out-blocks", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == open(os.path.join(GOLDEN, "ref_blocks.cbor"), "rb").read()


# ------------------------------------------------------------ plan program
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trace_plan") / "trace_plan_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "trace_plan_check.cpp")],
                   check=True)

    def run(*args, stdin=""):
        r = subprocess.run([exe] + [str(a) for a in args], input=stdin, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        assert r.stderr == "", r.stderr[-2000:]  # a sanitizer report
        return r.stdout

    return run


def designed_trace(t, tau, seed):
    """Moves over the whole i8 range (nothing restricts them to -1, 0, 1), so
    windows, offsets and both input-head sums take many-byte values of both signs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    imv = rng.integers(-128, 128, size=t, dtype=np.int8)
    mv = rng.integers(-128, 128, size=(t, tau), dtype=np.int8)
    hw = (rng.random((t, tau)) < 0.4).astype(np.uint8)
    ws = rng.integers(0, 16, size=(t, tau), dtype=np.uint16) * hw
    return imv, mv, hw, ws.astype(np.uint16)


def metadata_text(blocks):
    nb, tau = blocks.n_blocks, blocks.tau
    wl, wr = blocks.win_left.reshape(nb, tau), blocks.win_right.reshape(nb, tau)
    oi, oo = blocks.off_in.reshape(nb, tau), blocks.off_out.reshape(nb, tau)
    lines = []
    for k in range(nb):
        vals = [blocks.in_head_in[k], blocks.in_head_out[k], *wl[k], *wr[k], *oi[k], *oo[k]]
        lines.append(" ".join(str(int(x)) for x in vals))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("tau", [0, 1, 8, 40, 41])
@pytest.mark.parametrize("t,b", [(64, 5), (16, 16)])
def test_leaf_message_hashes_to_the_leaf_hash(plan, product, tau, t, b):
    blocks = product.partition(*designed_trace(t, tau, 11 + tau), b)
    want = blocks.leaf_hashes()
    out = plan("leaves", t, tau, b, stdin=metadata_text(blocks)).split()
    assert len(out) == blocks.n_blocks
    for k, line in enumerate(out):
        msg = bytes.fromhex(line)
        assert len(msg) == 58 + 24 * tau
        h = C.create_string_buffer(32)
        product.lib.sezkp_blake3(msg, len(msg), h, 32)
        assert h.raw == want[32 * k:32 * k + 32], (tau, k)
    dev = json.loads(plan("leafdev", tau))
    assert dev == {"len": 58 + 24 * tau, "on_device": tau <= 40, "max_tau": 40}


def test_leaf_message_takes_large_fields(plan, product):
    """Eight-byte fields with every byte in use: the windows of one long block
    of +127 / -128 moves, an input head near -2^31, offsets near 2^31."""
    t, tau = 1 << 16, 2
    imv = np.full(t, -128, np.int8)
    mv = np.stack([np.full(t, 127, np.int8), np.full(t, -128, np.int8)], axis=1)
    z = np.zeros((t, tau), np.uint8)
    blocks = product.partition(imv, mv, z, z.astype(np.uint16), t // 2)
    assert int(blocks.in_head_out[-1]) == -128 * t and int(blocks.off_in[1]) == 128 * (t // 2)
    want = blocks.leaf_hashes()
    for k, line in enumerate(plan("leaves", t, tau, t // 2, stdin=metadata_text(blocks)).split()):
        h = C.create_string_buffer(32)
        msg = bytes.fromhex(line)
        product.lib.sezkp_blake3(msg, len(msg), h, 32)
        assert h.raw == want[32 * k:32 * k + 32]


def test_scan_tiling_tiles_the_blocks(plan):
    tile = json.loads(plan("tiles", 1))["tile"]
    assert tile >= 256 and tile % 256 == 0
    for nblk in (1, tile - 1, tile, tile + 1, 2 * tile + 3):
        p = json.loads(plan("tiles", nblk))
        assert p["ntiles"] == -(-nblk // tile) == len(p["ranges"])
        at = 0
        for lo, hi in p["ranges"]:
            assert lo == at and lo < hi <= lo + tile
            at = hi
        assert at == nblk


@pytest.mark.parametrize("t,b", [(32, 4), (4096, 333), (1024, 1024), (7, 1), (10, 64)])
def test_uniform_step_start_is_partition_traces(plan, product, t, b):
    p = json.loads(plan("shape", t, b))
    z = np.zeros((t, 1), np.uint8)
    blocks = product.partition(np.zeros(t, np.int8), z.astype(np.int8), z, z.astype(np.uint16), b)
    assert p["nblk"] == blocks.n_blocks
    assert p["step_start"] == [int(x) for x in blocks.step_start]
