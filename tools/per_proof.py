#!/usr/bin/env python3
"""Per-proof figures of the dictionary table kernels from a rocprofv3 csv of a
one-proof-at-a-time run. The dispatches are cut into proofs at every k_expand
(the first kernel of a proof).

    python3 tools/per_proof.py pmc <counter_collection.csv>
        wave64 VALU instructions (SQ_INSTS_VALU) per proof, with the share of
        k_dict_level and k_dict_plan and k_dict_level's time per launch
    python3 tools/per_proof.py trace <kernel_trace.csv>
        per proof the summed time of the table kernels (k_dict_level) and
        the span from k_dict_plan's end to
        k_col_commit_dict's start (the dependent chain in front of the commit);
        proofs grouped by launches and by the table kernels' time
"""
import csv
import sys
from statistics import median

from pmc_valu import short as short_inst

TABLE_KERNELS = ("k_dict_level",)


def short(name):
    return short_inst(name).split("<")[0]


def proofs_of(dispatches):
    """dispatches: (start ns, end ns, kernel, value) -> one list per proof."""
    out = []
    for d in sorted(dispatches):
        if d[2] == "k_expand":
            out.append([])
        if out:
            out[-1].append(d)
    return out


def pmc(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] == "SQ_INSTS_VALU":
            rows[int(r["Dispatch_Id"])] = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                                           short(r["Kernel_Name"]), float(r["Counter_Value"]))
    print("proof  valu_insts(wave64)  k_dict_level_insts  k_dict_plan_insts  k_dict_level us per launch")
    for i, p in enumerate(proofs_of(rows.values())):
        lvl = [d for d in p if d[2] == "k_dict_level"]
        print(f"{i:5d}  {sum(d[3] for d in p):18.0f}  {sum(d[3] for d in lvl):18.0f}  "
              f"{sum(d[3] for d in p if d[2] == 'k_dict_plan'):17.0f}  {[round((d[1] - d[0]) / 1e3, 1) for d in lvl]}")


def trace(path):
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), 0)
            for r in csv.DictReader(open(path))]
    proofs = proofs_of(rows)
    print("proofs", len(proofs))
    groups = {}
    for p in proofs:
        plan = [d[1] for d in p if d[2] == "k_dict_plan"]
        commit = [d[0] for d in p if d[2] == "k_col_commit_dict"]
        if not plan or not commit:
            continue
        tab = [d for d in p if d[2] in TABLE_KERNELS]
        tab_us = sum(d[1] - d[0] for d in tab) / 1e3
        lo = 0
        for hi in (10, 30, 60, 100, 200, 1e9):
            if tab_us < hi:
                break
            lo = hi
        cls = f"{lo}-{hi if hi < 1e9 else 'inf'}us"
        span = (max(d[1] for d in p) - p[0][0]) / 1e3
        groups.setdefault((cls, len(tab)), []).append((tab_us, (commit[0] - plan[-1]) / 1e3, span))
    print("class launches  n  median table-kernel us  median plan-end->commit-start us  median device span us")
    for (cls, ln), v in sorted(groups.items()):
        print(f"{cls:12s} {ln:3d} {len(v):4d}  {median(x[0] for x in v):10.1f}  {median(x[1] for x in v):10.1f}  "
              f"{median(x[2] for x in v):10.1f}")


if __name__ == "__main__":
    {"pmc": pmc, "trace": trace}[sys.argv[1]](sys.argv[2])
