"""The host-only part of the C ABI (csrc/abi_host.cpp) on the CPU, under the
sanitizers: the stand-alone tools/host_abi_check.cpp, built with the address
and undefined-behaviour sanitizers and linked with abi_host.cpp, codec.cpp,
host_crypto.cpp and tracegen.cpp (no HIP; nothing is loaded into Python), runs
the codecs, the manifest commitment and the simulator over the fixtures in
tests/golden/: CBOR and JSONL round trips byte for byte, the sliced JSONL
decoder and its line offsets, the committed manifest roots and both roots
again over the leaf hashes, the TraceFile codec, every truncation of a blocks
file and of a trace file refused with SEZKP_E_DECODE and a message, and the
simulator's blocks through the codec and the commitment. tests/test_host_abi.py
asserts the same through ctypes; this run adds the sanitizers."""
import os
import subprocess

from conftest import GOLDEN, PKG, ROOT


def test_host_abi_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_abi_check")
    csrc = os.path.join(PKG, "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "host_abi_check.cpp")] +
                   [os.path.join(csrc, f) for f in ("abi_host.cpp", "codec.cpp", "host_crypto.cpp", "tracegen.cpp")] +
                   ["-pthread"], check=True)
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stderr == "", r.stderr[-2000:]  # a sanitizer report
    out = r.stdout.splitlines()
    assert len(out) == 6 and out[-1].startswith("simulate t=64 b=8 tau=2"), out
    # no prefix of a fixture is itself a file of its kind
    assert [ln for ln in out if "prefixes refused" in ln] == [
        "ref_blocks.cbor: 4844 prefixes refused, 0 decode", "riscv_trace.cbor: 1373 prefixes refused, 0 decode"]
