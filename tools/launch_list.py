#!/usr/bin/env python3
"""Per call, the ordered (kernel, grid, workgroup) list of a rocprofv3
--kernel-trace csv of a probe that separates its calls by a one-element fill
kernel (a one-element int32 tensor made with torch.zeros, then fill_ before
every call) and writes the calls' labels (a JSON list) in call order.

    launch_list.py run_kernel_trace.csv labels.json

Prints JSON: "kernels", the distinct names of the library's kernels (without
their namespace; the runtime's copy and fill kernels are left out), then
"calls", one line per call: its label and "launches", [index into kernels,
grid in workgroups, workgroup size] in dispatch order. This is the form of
tests/golden/ntt_parent_launches.json, whose NTT pass kernels
tests/test_ntt_plan_host.py pins the planner to.
"""
import argparse
import csv
import json
import re


def short(name):
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, ch in enumerate(name):  # cut the argument list: the first '(' outside the template arguments
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("labels")
    args = ap.parse_args()
    labels = json.load(open(args.labels))
    rows = sorted(csv.DictReader(open(args.trace)), key=lambda r: int(r["Dispatch_Id"]))
    calls, cur = [], None
    for r in rows:
        name = short(r["Kernel_Name"])
        if "FillFunctor<int>" in name and int(r["Grid_Size_X"]) == int(r["Workgroup_Size_X"]):
            cur = []
            calls.append(cur)
        elif cur is not None and name.startswith("sezkp::"):
            wg = int(r["Workgroup_Size_X"])
            cur.append((name[len("sezkp::"):], int(r["Grid_Size_X"]) // wg, wg))
    calls = calls[1:]  # the first fill is the separator's own allocation (torch.zeros)
    assert len(calls) == len(labels), (len(calls), len(labels))
    kernels = sorted({k[0] for ks in calls for k in ks})
    index = {k: i for i, k in enumerate(kernels)}
    lines = [json.dumps(dict(label, launches=[[index[n], g, b] for n, g, b in ks]), separators=(",", ":"))
             for label, ks in zip(labels, calls) if label["call"] != "end"]
    print('{"kernels": [\n' + ",\n".join(json.dumps(k) for k in kernels) + '],\n"calls": [\n' + ",\n".join(lines) + "]}")


if __name__ == "__main__":
    main()
