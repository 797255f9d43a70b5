"""The host's decision for the wide head ladder (csrc/prove_plan.h:
head_wide_decide / head_wide_observe) on the CPU: the stand-alone
tools/head_wide_check.cpp, built with the address and undefined-behaviour
sanitizers, replays the proofs of one head column and prints each decision;
nothing is loaded into Python. Checked: when the ladder is built (never by
the first proof of an epoch), its span and sizes, when it is kept, re-spanned
(the union with the old span, or the new range alone when the union does not
fit the cap), dropped and invalidated."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CAP = 1 << 19
M = 8  # HEAD_WIDE_MARGIN


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("head_wide") / "head_wide_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "head_wide_check.cpp")],
                   check=True)

    def run(proofs):
        r = subprocess.run([exe] + [":".join(str(int(x)) for x in p) for p in proofs], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        assert r.stderr == "", r.stderr[-2000:]  # a sanitizer report
        return json.loads(r.stdout)

    return run


def proof(epoch=1, cap=CAP, lo=-70, hi=69, mlo=-1, mhi=1, delta=1, wide=0, fb_start=0, fb_span=0):
    return (epoch, cap, lo, hi, mlo, mhi, delta, wide, fb_start, fb_span)


def sizes(span, dR, dmin):
    sw = span + 7 * (max(dmin + dR - 1, 0) - min(dmin, 0))
    return span * dR ** 7, sw * (1 + dR + dR ** 3)


def test_first_proof_builds_nothing_second_builds_third_reuses(replay):
    a, b, c = replay([proof(), proof(wide=1000), proof(wide=1000)])
    assert (a["use"], a["build"], a["in_place"]) == (0, 0, 0)
    l3, low = sizes(140 + 2 * M, 3, -1)
    assert (b["use"], b["build"], b["in_place"]) == (1, 1, 1)
    assert (b["olo"], b["span"], b["dmin"], b["dR"], b["l3"], b["low"]) == (-70 - M, 140 + 2 * M, -1, 3, l3, low)
    assert l3 == 156 * 2187 and low == (156 + 14) * 31
    assert (c["use"], c["build"], c["olo"], c["span"]) == (1, 0, -70 - M, 140 + 2 * M)


def test_inside_the_margin_is_kept_and_a_few_outside_too(replay):
    out = replay([proof(), proof(wide=32768),
                  proof(lo=-77, hi=77, wide=32768),                      # inside the margin
                  proof(lo=-90, hi=69, wide=32768 - 512, fb_span=512),   # exactly 1/64: kept
                  proof(wide=32768)])
    assert [o["build"] for o in out] == [0, 1, 0, 0, 0]
    assert [o["respan"] for o in out] == [0, 0, 0, 0, 0]
    assert all(o["span"] == 156 and o["olo"] == -78 for o in out[1:])


def test_respan_to_the_union_above_the_threshold(replay):
    out = replay([proof(), proof(wide=32768),
                  proof(lo=-60, hi=100, wide=32768 - 513, fb_span=513),  # above 1/64
                  proof(lo=-60, hi=100, wide=32768),                     # rebuilt over both ranges
                  proof(wide=32768)])                                    # the first trace again: kept
    assert [o["respan"] for o in out] == [0, 0, 1, 0, 0]
    assert [o["build"] for o in out] == [0, 1, 0, 1, 0]
    assert (out[3]["olo"], out[3]["span"]) == (-78, 108 + 78 + 1)
    assert (out[4]["olo"], out[4]["span"], out[4]["use"]) == (-78, 187, 1)
    assert out[3]["l3"] == 187 * 2187


def test_respan_to_the_new_range_when_the_union_does_not_fit(replay):
    out = replay([proof(), proof(wide=32768),
                  proof(lo=100, hi=239, wide=0, fb_span=32768),
                  proof(lo=100, hi=239, wide=32768)])
    # the union [-78, 247] has 326 values: 326 * 2187 > 2^19
    assert out[3]["build"] == 1 and (out[3]["olo"], out[3]["span"]) == (100 - M, 140 + 2 * M)


def test_block_start_fallbacks_do_not_respan(replay):
    out = replay([proof(), proof(wide=100, fb_start=32668), proof(wide=100, fb_start=32668)])
    assert [o["respan"] for o in out] == [0, 0, 0] and [o["build"] for o in out] == [0, 1, 0]


def test_moves_outside_widen_the_ladder(replay):
    out = replay([proof(mlo=0, mhi=1), proof(mlo=0, mhi=1, wide=32768),
                  proof(wide=0, fb_span=32768), proof(wide=32768)])
    assert (out[1]["dmin"], out[1]["dR"]) == (0, 2) and out[1]["l3"] == 156 * 128
    assert out[1]["low"] == (156 + 7) * (1 + 2 + 8)
    assert out[3]["build"] == 1 and (out[3]["dmin"], out[3]["dR"], out[3]["span"]) == (-1, 3, 156)


def test_epoch_move_invalidates(replay):
    out = replay([proof(), proof(wide=32768), proof(epoch=2, wide=0), proof(epoch=2, wide=32768),
                  proof(epoch=3), proof(epoch=4), proof(epoch=5)])
    assert [o["build"] for o in out] == [0, 1, 0, 1, 0, 0, 0]
    assert [o["in_place"] for o in out] == [0, 1, 0, 1, 0, 0, 0]
    assert [o["use"] for o in out] == [0, 1, 0, 1, 0, 0, 0]


def test_cap_and_plans_that_do_not_qualify(replay):
    # span 156 needs 156 * 2187 = 341172 entries
    out = replay([proof(cap=341171), proof(cap=341171), proof(cap=341172), proof(cap=341171), proof(cap=341172)])
    assert [o["build"] for o in out] == [0, 0, 1, 0, 1]
    assert [o["use"] for o in out] == [0, 0, 1, 0, 1]
    assert [o["in_place"] for o in out] == [0, 0, 1, 0, 1]
    # moves of range 2: 5^7 entries per head value; no delta plan; an empty range
    for p in (proof(mlo=-2, mhi=2), proof(delta=0), proof(lo=0, hi=-1), proof(mlo=0, mhi=-1), proof(mlo=0, mhi=300)):
        out = replay([p, p, p])
        assert [(o["use"], o["build"], o["in_place"]) for o in out] == [(0, 0, 0)] * 3
    # a cap beyond 2^24 is held to 2^24 (the commit indexes L3 in 32 bits)
    wide = proof(lo=0, hi=7671 - 2 * M - 1 + 1, cap=1 << 40)
    out = replay([wide, wide])
    assert out[1]["build"] == 0
    fits = proof(lo=0, hi=7671 - 2 * M - 1, cap=1 << 40)
    out = replay([fits, fits])
    assert out[1]["build"] == 1 and out[1]["l3"] == 7671 * 2187 <= 1 << 24


def test_extreme_heads(replay):
    lo, hi = -(1 << 31), -(1 << 31) + 99
    out = replay([proof(lo=lo, hi=hi), proof(lo=lo, hi=hi)])
    assert (out[1]["olo"], out[1]["span"]) == (lo - M, 100 + 2 * M)
    lo, hi = (1 << 31) - 100, (1 << 31) - 1
    out = replay([proof(lo=lo, hi=hi), proof(lo=lo, hi=hi)])
    assert (out[1]["olo"], out[1]["span"]) == (lo - M, 100 + 2 * M)
