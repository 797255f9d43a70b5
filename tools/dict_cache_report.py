#!/usr/bin/env python3
"""Headline A/B table from tools/dict_cache_ab.sh's ab/ directory: per pair
the `value` of the parent, of this tree and of this tree with
SEZKP_DICT_CACHE=0, and the project's bar for a gain: every pair has the new
arm ahead AND the mean gain exceeds the largest difference between two runs
of one arm in the session.

    python3 tools/dict_cache_report.py [--off-label VAR=value] <ab dir>

--off-label names the third arm's switch when the A/B ran with another one
(tools/dict_cache_ab.sh, SEZKP_AB_OFF). Without runs of a third arm
(SEZKP_AB_OFF=none) the table has two arms and the verdict is the equality
rule: the new arm not worse than the parent beyond the same-arm spread.
"""
import glob
import json
import os
import sys


def values(d, arm):
    out = {}
    for f in glob.glob(os.path.join(d, f"{arm}_[0-9]*.json")):
        i = int(os.path.basename(f)[len(arm) + 1:-5])
        lines = [l for l in open(f).read().splitlines() if l.startswith("{")]
        if lines:
            out[i] = json.loads(lines[-1])["value"] / 1e9
    return out


def verdict(name, new, base):
    idx = sorted(set(new) & set(base))
    gains = [new[i] / base[i] - 1 for i in idx]
    mean_gain = sum(new[i] for i in idx) / sum(base[i] for i in idx) - 1
    spread = max((max(a.values()) - min(a.values())) / (sum(a.values()) / len(a)) for a in (new, base))
    every = all(g > 0 for g in gains)
    print(f"{name}: pairs ahead {sum(g > 0 for g in gains)}/{len(idx)}, per pair "
          + " ".join(f"{100 * g:+.2f}%" for g in gains)
          + f"; mean gain {100 * mean_gain:+.2f}%, largest same-arm spread {100 * spread:.2f}% -> "
          + ("a gain by the project's bar" if every and mean_gain > spread else "NOT a gain by the project's bar"))


def equality(new, base):
    """A change without a switch (a refactor): the claim is equality, so the
    new arm must not be below the parent by more than the larger difference
    between two runs of one arm, the rule of the --full views."""
    mean_change = (sum(new.values()) / len(new)) / (sum(base.values()) / len(base)) - 1
    spread = max((max(a.values()) - min(a.values())) / (sum(a.values()) / len(a)) for a in (new, base))
    print(f"new vs parent (equality claimed): mean change {100 * mean_change:+.2f}%, largest same-arm spread "
          f"{100 * spread:.2f}% -> " + ("WORSE beyond the spread" if -mean_change > spread else "not worse beyond the spread"))


def main(d, off_label="SEZKP_DICT_CACHE=0"):
    par, new, off = values(d, "parent"), values(d, "new"), values(d, "new_cache_off")
    print("value, 1e9 field-elements/s (plain `python bench.py`, 200 steps, 3 proofs in flight), runs alternating")
    print("pair   parent      new" + (f"  new, {off_label}" if off else ""))
    for i in sorted(new):
        print(f"{i:4d}  {par.get(i, float('nan')):7.3f}  {new[i]:7.3f}" + (f"  {off[i]:7.3f}" if i in off else ""))
    for name, a in (("parent", par), ("new", new), ("switch off", off)):
        if a:
            print(f"{name:10s} mean {sum(a.values()) / len(a):.3f}  min {min(a.values()):.3f}  max {max(a.values()):.3f}")
    if par and not off:  # tools/dict_cache_ab.sh with SEZKP_AB_OFF=none
        equality(new, par)
    elif par:
        verdict("new vs parent", new, par)
    if off:
        verdict(f"new vs new with {off_label}", new, off)


FULL_VIEWS = (  # name, path in the bench line, higher is better
    ("value 1e9", ("value",), True),
    ("single_proof ms", ("single_proof", "ms_per_proof"), False),
    ("host_to_proof ms/proof", ("host_to_proof", "ms_per_proof"), False),
    ("c3 single ms", ("configs", "c3_prove_2e18", "single_proof_ms"), False),
    ("c3 inflight3 ms", ("configs", "c3_prove_2e18", "inflight3_ms_per_proof"), False),
    ("worst no_dict inflight ms", ("worst_case", "no_dict", "inflight3_ms_per_proof"), False),
    ("worst high_entropy inflight ms", ("worst_case", "high_entropy", "inflight3_ms_per_proof"), False),
    ("sharded_predicted P=2 ms", ("sharded_predicted", "2", "predicted_ms_per_proof"), False),
    ("sharded_predicted P=4 ms", ("sharded_predicted", "4", "predicted_ms_per_proof"), False),
    ("sharded_predicted P=8 ms", ("sharded_predicted", "8", "predicted_ms_per_proof"), False),
)


def lines_of(d, arm):
    out = {}
    for f in glob.glob(os.path.join(d, f"{arm}_[0-9]*.json")):
        lines = [l for l in open(f).read().splitlines() if l.startswith("{")]
        if lines:
            out[int(os.path.basename(f)[len(arm) + 1:-5])] = json.loads(lines[-1])
    return out


def full(d):
    """The other views of alternating `bench.py --full` runs: per view every
    run of both arms, and whether the new arm is worse than the parent by more
    than the larger spread inside one arm."""
    par, new = lines_of(d, "parent"), lines_of(d, "new")

    def get(line, path):
        for k in path:
            line = line.get(k) if isinstance(line, dict) else None
        return line / 1e9 if path == ("value",) and line else line

    print("view: parent runs | new runs | mean parent -> new (change) | same-arm spread | worse beyond the spread?")
    for name, path, up in FULL_VIEWS:
        a = [get(par[i], path) for i in sorted(par)]
        b = [get(new[i], path) for i in sorted(new)]
        if not a or not b or None in a or None in b:
            continue
        ma, mb = sum(a) / len(a), sum(b) / len(b)
        spread = max(max(a) - min(a), max(b) - min(b)) / ma
        change = mb / ma - 1
        worse = (-change if up else change) > spread
        print(f"{name:32s} {' '.join(f'{x:.4g}' for x in a)} | {' '.join(f'{x:.4g}' for x in b)} | "
              f"{ma:.4g} -> {mb:.4g} ({100 * change:+.2f}%) | {100 * spread:.2f}% | {'YES' if worse else 'no'}")


if __name__ == "__main__":
    if sys.argv[1] == "--full":
        full(sys.argv[2])
    elif sys.argv[1] == "--off-label":
        main(sys.argv[3], sys.argv[2])
    else:
        main(sys.argv[1])
