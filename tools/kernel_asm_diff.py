#!/usr/bin/env python3
"""Compare kernels between two sets of device assembly files (hipcc
--cuda-device-only -S).

    kernel_asm_diff.py --a old1.s [old2.s ...] --b new1.s [new2.s ...]

Per kernel symbol present on both sides: the text from its label to its
.Lfunc_end, comments stripped, local labels .LBB<k>_<n> rewritten to .LBB_<n>,
and the verdict `same` or `differs` with the instruction-line counts.
"""
import argparse
import re
import subprocess


def kernels(paths):
    out = {}
    for p in paths:
        name, body = None, []
        for line in open(p, errors="replace"):
            m = re.match(r"^(_Z\w+):", line)
            if m and name is None and "k_" in m.group(1):
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            line = re.sub(r"\s*;.*$", "", line.rstrip("\n")).rstrip()
            line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
            if line.strip():
                body.append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    args = ap.parse_args()
    a, b = kernels(args.a), kernels(args.b)
    names = sorted(set(a) | set(b))
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    for sym, d in zip(names, dem):
        d = re.sub(r"\(.*$", "", d)
        if sym not in a or sym not in b:
            print(f"{d:48s} only in {'a' if sym in a else 'b'}")
        else:
            print(f"{d:48s} {'same' if a[sym] == b[sym] else 'differs':8s} {len(a[sym])} / {len(b[sym])} lines")


if __name__ == "__main__":
    main()
