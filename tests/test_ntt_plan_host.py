"""The transforms' pass planner (csrc/ntt_plan.h) on the CPU: the stand-alone
tools/ntt_plan_check.cpp, built with the address and undefined-behaviour
sanitizers, prints the plan of each request as JSON; nothing is loaded into
Python. Checked over every request kind at 2^1..2^28: the passes cover the
stages and tile the points, every pass's kernel form meets the preconditions
of that kernel (restated here from the kernels' static_asserts and their
former launch guards), the buffers chain, the scale and the fused DEEP sit
only where they may. The pass lists the code comments state are pinned
literally, and the planner's launches for the requests of a C-ABI probe are
pinned to the launches recorded from a kernel trace of that probe on the
commit before the planner existed (tests/golden/ntt_parent_launches.json).

The kernel names compared there are the tool's own (kernel_name in
ntt_plan_check.cpp, from a pass's form, M1, M2 and SKIP), not the
form-to-instantiation switches of ntt_pass.hip and ntt_pass512.hip: an edit
of launch_form or launch_split that picks another instantiation does not fail
this test. That switch is covered on the GPU only: by the kernel trace of the
new build equal to the golden file (profiles/ntt_split/launches_new.json) and
by the parity tests of every size."""
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

K, S = 32, 16
LOGNS = range(1, 29)
# the (blow-up, dpoly, deep) the callers make: the kernel-level LDE at blow-ups
# 0..3 with and without the fused DEEP; the prover at blow-up 3 with the DEEP
# polynomial or the fused DEEP; a rank of a sharded proof over 2, 4 or 8 ranks,
# whose LDE of 2^(log N - log P) points loads all 2^log n coefficients: the
# DEEP polynomial at blow-ups 2, 1 and 0 (at blow-up 0 and 2^10..2^12 points
# one X16 pass that loads the polynomial), the fused DEEP likewise
LDE_CASES = [(b, 0, deep) for b in range(4) for deep in (0, 1)] + [(b, 1, 0) for b in range(4)]


def lde_req(logN, b, dpoly, deep, inv=0):
    return "lde:%d:%d:%d:%d:%d" % (logN, inv, logN - b, dpoly, deep)


def all_requests():
    out = []
    for logN in LOGNS:
        for inv in (0, 1):
            for kind in ("dif", "dit", "natural", "natural_dit", "natural_tr", "natural_store"):
                out.append("%s:%d:%d" % (kind, logN, inv))
        out += [lde_req(logN, b, dp, dq) for b, dp, dq in LDE_CASES if b <= logN]
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ntt_plan") / "ntt_plan_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "ntt_plan_check.cpp")],
                   check=True)
    cache = {}

    def run(requests):
        todo = [r for r in dict.fromkeys(requests) if r not in cache]
        if todo:
            r = subprocess.run([exe, "K=%d" % K, "S=%d" % S] + todo, capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
            assert r.stderr == "", r.stderr[-2000:]  # a sanitizer report
            for p in json.loads(r.stdout):
                cache[p["request"]] = p
        return [cache[r] for r in requests]

    run(all_requests())
    return run


def one(plans, request):
    return plans([request])[0]


def ms(plan):
    return [p["m"] for p in plan["passes"]]


def forms(plan):
    return [p["form"] for p in plan["passes"]]


# ------------------------------------------------------- every plan is sound
def check_pass(p, i, plan, logN, inv, src, log_src, dpoly):
    """One pass against its kernel's preconditions."""
    dif, np_, f = plan["dif"], len(plan["passes"]), p["form"]
    first, last = i == 0, i == np_ - 1
    m, sL, logC = p["m"], p["sL"], p["logC"]
    contiguous = f in ("x16", "n12r8")  # a tile of 2^m contiguous points
    assert p["tiles"] << (m if contiguous else m + logC) == 1 << logN
    assert p["grid"] == p["tiles"] and p["block"] == p["threads"] == (512 if f in ("dif9", "w8r8", "n12r8") else 256)
    # the LDE's loads: the first DIT pass only; the skip is the stages replication makes trivial
    assert p["loads_src"] == (src and first) and p["loads_dpoly"] == (dpoly and first)
    assert not (p["loads_src"] and dif)
    assert p["skip"] == (logN - log_src if p["loads_src"] and not dpoly else 0) <= m
    if f == "generic":  # k_ntt_pass: 2^m rows x 2^logC columns in (1 << 8) * 17 words of LDS
        assert m <= 8 and logC == min(4, logN - m)
        assert (p["M1"], p["M2"], p["SKIP"]) == (0, 0, 0)
    elif f in ("wide", "narrow", "x16", "deep"):  # k_ntt4
        assert logC == 4  # 16 columns x 16 row groups = 256 lanes
        assert (p["M1"], p["M2"]) in ((3, 3), (4, 3), (4, 4))
        assert m == p["M1"] + p["M2"] + (4 if f == "x16" else 0)
        assert p["SKIP"] == (p["skip"] if p["loads_src"] else 0) <= 3
        assert not (dif and p["SKIP"])  # the skipping butterflies exist on the DIT side only
        if f == "wide":
            assert sL >= 4 and not p["loads_src"] and not p["nat_out"] and not p["nat_tr"]
        else:
            assert (sL == 0) == (f != "deep")
        if f == "x16":  # static_assert(!X16 || (NARROW && SKIP == 0)); not with the replicated load
            assert p["SKIP"] == 0 and not (p["loads_src"] and not p["loads_dpoly"]) and not p["nat_tr"]
        if f == "deep":  # static_assert(F1 * NTT_CMAX == NTT_THREADS && !INV && !DIF); a wide pass
            assert p["M1"] == 4 and not dif and not inv and sL >= 4 and last and not first and p["SKIP"] == 0
    elif f == "dif9":
        assert dif and m == 9 and sL >= 4 and logC == 4 and not p["nat_out"] and not p["nat_tr"]
    elif f == "w8r8":
        assert dif and m == 8 and sL >= 4 and logC == 4 and not p["nat_out"] and not p["nat_tr"]
    elif f == "n12r8":
        assert dif and m == 12 and sL == 0 and p["nat_out"] and last
    else:
        raise AssertionError(f)
    # the natural-order stores: the narrow DIF pass; the transposed pair: 16 blocks of 2^m <= 2^8 points
    if p["nat_out"]:
        assert dif and last and sL == 0 and f in ("narrow", "x16", "n12r8")
    if p["nat_tr"]:
        assert f == "narrow" and m <= 8 and (last if dif else first)
    # a pass table only where the kernel reads one and its entries are single hi entries
    if p["tw_pass"]:
        assert f in ("wide", "deep") and sL >= 4 and m + sL <= K - S
    elif f in ("wide", "deep"):
        assert m + sL > K - S


def check_plan(plan, logN, inv, natural=False, src=False, log_src=0, dpoly=False, deep=False):
    ps = plan["passes"]
    assert 1 <= len(ps) <= 8
    assert sum(ms(plan)) == logN
    at = logN if plan["dif"] else 0
    for i, p in enumerate(ps):  # sL chains: descending for DIF, ascending for DIT
        if plan["dif"]:
            at -= p["m"]
        assert p["sL"] == at, (i, p["sL"], at)
        if not plan["dif"]:
            at += p["m"]
        check_pass(p, i, plan, logN, inv, src, log_src, dpoly)
    # buffers: the first pass reads a, the last writes a, no pass reads what was not written
    written = {"a"}
    for p in ps:
        assert p["reads"] in written
        written = {p["writes"]} if natural else written | {p["writes"]}
    assert ps[0]["reads"] == "a" and ps[-1]["writes"] == "a"
    if natural:
        assert len(ps) >= 2 and [p["writes"] for p in ps[:-1]] == ["scratch"] * (len(ps) - 1)
        assert any(p["nat_out"] or p["nat_tr"] for p in ps)
    else:
        assert all(p["reads"] == p["writes"] == "a" and not p["nat_out"] and not p["nat_tr"] for p in ps)
    # the scale: the last pass of a natural transform, nowhere else
    assert [p["out_scale"] for p in ps] == [False] * (len(ps) - 1) + [natural]
    # fused DEEP: asked for, the last pass but not the first, forward, 16 wide columns, m of 7 or 8
    last = ps[-1]
    may = deep and len(ps) >= 2 and not inv and last["logC"] == 4 and last["sL"] >= 4 and last["m"] in (7, 8)
    assert plan["deep_fused"] == may == ("deep" in forms(plan))


@pytest.mark.parametrize("logN", LOGNS)
def test_every_plan_is_sound(plans, logN):
    for inv in (0, 1):
        for kind, dif in (("dif", True), ("dit", False)):
            plan = one(plans, "%s:%d:%d" % (kind, logN, inv))
            assert plan["status"] == "ok" and plan["dif"] == dif
            check_plan(plan, logN, inv)
        for kind in ("natural", "natural_dit", "natural_tr", "natural_store"):
            plan = one(plans, "%s:%d:%d" % (kind, logN, inv))
            assert plan["status"] in ("ok", "bitrev")
            if plan["status"] == "ok":
                check_plan(plan, logN, inv, natural=True)
            else:
                assert plan["passes"] == []
    for b, dpoly, deep in LDE_CASES:
        if b <= logN:
            plan = one(plans, lde_req(logN, b, dpoly, deep))
            assert plan["status"] == "ok" and not plan["dif"]
            check_plan(plan, logN, 0, src=True, log_src=logN - b, dpoly=bool(dpoly), deep=bool(deep))


# ---------------------------------------------- the plans the comments state
def test_x16_single_pass(plans):
    for logN in (10, 11, 12):
        for kind in ("dif", "dit"):
            plan = one(plans, "%s:%d:0" % (kind, logN))
            assert ms(plan) == [logN] and forms(plan) == ["x16"]


def test_x16_two_and_three_passes(plans):
    two = {17: [6, 11], 18: [6, 12], 19: [7, 12], 20: [8, 12]}
    three = {25: [7, 6, 12], 26: [7, 7, 12], 27: [8, 7, 12], 28: [8, 8, 12]}
    for logN, want in {**two, **three}.items():
        for inv in (0, 1):
            dif, dit = one(plans, "dif:%d:%d" % (logN, inv)), one(plans, "dit:%d:%d" % (logN, inv))
            assert ms(dif) == want and forms(dif) == ["wide"] * (len(want) - 1) + ["x16"]
            assert ms(dit) == want[::-1][:1] + want[:-1] and forms(dit) == ["x16"] + ["wide"] * (len(want) - 1)
            # the DEEP-polynomial LDE takes the DIT plan; the replicated load does not
            assert ms(one(plans, lde_req(logN, 3, 1, 0))) == ms(dit)
            assert "x16" not in forms(one(plans, lde_req(logN, 3, 0, 1)))


def test_plain_plans(plans):
    assert ms(one(plans, "dif:24:0")) == ms(one(plans, "dit:24:1")) == [8, 8, 8]
    assert forms(one(plans, "dif:24:0")) == ["wide", "wide", "narrow"]
    assert forms(one(plans, "dit:24:1")) == ["narrow", "wide", "wide"]
    assert ms(one(plans, "dif:22:0")) == [8, 7, 7] and ms(one(plans, "dif:13:1")) == [7, 6]
    # below 2^10 and wherever fewer than 16 columns or 6 stages are left: k_ntt_pass
    for logN in range(1, 10):
        assert forms(one(plans, "dif:%d:0" % logN)) == ["generic"] * (1 if logN <= 8 else 2)


def test_dif_2p21_is_dif9_then_x16(plans):
    for inv in (0, 1):
        plan = one(plans, "dif:21:%d" % inv)
        assert ms(plan) == [9, 12] and forms(plan) == ["dif9", "x16"]
        assert [p["kernel"] for p in plan["passes"]] == \
            ["k_ntt_dif9<%s>" % ("false", "true")[inv],
             "k_ntt4<true, %s, 4, 4, 0, false, true, true>" % ("false", "true")[inv]]
    assert ms(one(plans, "dit:21:0")) == [7, 7, 7]  # the DIT keeps three passes
    assert "dif9" not in [f for logN in LOGNS if logN != 21 for f in forms(one(plans, "dif:%d:1" % logN))]


def test_natural_choices_by_size(plans):
    for inv in (0, 1):
        chosen = {}
        for logN in LOGNS:
            plan = one(plans, "natural:%d:%d" % (logN, inv))
            which = [k for k in ("natural_dit", "natural_tr", "natural_store")
                     if one(plans, "%s:%d:%d" % (k, logN, inv))["status"] == "ok"]
            if plan["status"] == "bitrev":
                assert which == []
                continue
            # the first planner that takes the size, in this order
            want = one(plans, "%s:%d:%d" % (which[0], logN, inv))
            assert plan["passes"] == want["passes"] and plan["dif"] == want["dif"]
            chosen[logN] = which[0]
        assert chosen == {19: "natural_store", 20: "natural_store", 21: "natural_dit", 22: "natural_dit",
                          23: "natural_dit", 24: "natural_dit", 25: "natural_tr", 26: "natural_tr"}


def test_natural_dit_gathers_in_its_first_pass(plans):
    for logN, want in {21: [7, 7, 7], 22: [8, 7, 7], 23: [8, 8, 7], 24: [8, 8, 8]}.items():
        plan = one(plans, "natural_dit:%d:1" % logN)
        assert not plan["dif"] and ms(plan) == want and forms(plan) == ["narrow", "wide", "wide"]
        assert [p["nat_tr"] for p in plan["passes"]] == [True, False, False]
    for logN in (20, 25):
        assert one(plans, "natural_dit:%d:0" % logN)["status"] == "bitrev"


def test_natural_transposed_pass(plans):
    want = {23: [8, 7, 8], 24: [8, 8, 8], 25: [9, 8, 8], 26: [9, 9, 8]}
    for logN, m in want.items():
        plan = one(plans, "natural_tr:%d:0" % logN)
        assert plan["dif"] and ms(plan) == m
        assert forms(plan) == [{9: "dif9"}.get(x, "wide") for x in m[:2]] + ["narrow"]
        assert [p["nat_tr"] for p in plan["passes"]] == [False, False, True]
    for logN in (22, 27):
        assert one(plans, "natural_tr:%d:0" % logN)["status"] == "bitrev"


def test_natural_store_and_radix8_at_2p20_only(plans):
    for logN in LOGNS:
        for inv in (0, 1):
            for kind in ("dif", "dit", "natural", "natural_dit", "natural_tr", "natural_store"):
                f = forms(one(plans, "%s:%d:%d" % (kind, logN, inv)))
                assert ("w8r8" in f or "n12r8" in f) == (logN == 20 and kind in ("natural", "natural_store")), (kind, logN)
    plan = one(plans, "natural:20:1")
    assert forms(plan) == ["w8r8", "n12r8"] and ms(plan) == [8, 12]
    assert [(p["kernel"], p["grid"], p["block"]) for p in plan["passes"]] == \
        [("k_ntt_w8r8<true>", 256, 512), ("k_ntt_n12r8<true>", 256, 512)]
    plan = one(plans, "natural:19:0")
    assert forms(plan) == ["wide", "x16"] and ms(plan) == [7, 12] and plan["passes"][1]["nat_out"]
    assert [one(plans, "natural_store:%d:0" % n)["status"] for n in (18, 19, 22, 23)] == ["bitrev", "ok", "ok", "bitrev"]


def test_lde_skip_and_fused_deep(plans):
    # the prover's LDE at blow-up 8: the first pass skips 3 stages; DEEP fused from two passes on
    plan = one(plans, lde_req(15, 3, 0, 1))
    assert ms(plan) == [8, 7] and forms(plan) == ["narrow", "deep"] and plan["deep_fused"]
    assert [p["kernel"] for p in plan["passes"]] == ["k_ntt4<false, false, 4, 4, 3, false, true, false>",
                                                      "k_ntt4<false, false, 4, 3, 0, true, false, false>"]
    assert not one(plans, lde_req(8, 3, 0, 1))["deep_fused"]      # one pass: the last is the first
    assert not one(plans, lde_req(13, 3, 0, 1))["deep_fused"]     # [7, 6]: the last pass has 6 stages
    assert not one(plans, lde_req(15, 3, 0, 1, inv=1))["deep_fused"]
    assert not one(plans, lde_req(15, 3, 1, 0))["deep_fused"]     # not asked for
    # a first pass below 6 stages or 16 columns keeps its skip in k_ntt_pass
    plan = one(plans, lde_req(5, 3, 0, 0))
    assert forms(plan) == ["generic"] and plan["passes"][0]["skip"] == 3


def test_refused_before_any_launch(plans):
    refused = ["lde:20:0:5:0:0",    # the first pass (7 stages) cannot hold the 15 stages replication makes trivial
               "lde:20:0:21:0:0",   # more coefficients than points
               "dif:33:0", "dit:-1:0", "natural:33:1"]
    for r in plans(refused):
        assert r["status"] == "refused" and r["passes"] == [], r["request"]


# ------------------------------------- the launches of the commit before it
def requests_of(call):
    """The transforms a probe call runs, as planner requests, in launch order."""
    n = call["log_n"]
    if call["call"] == "gl_ntt":
        inv = call["inverse"]
        return [("natural:%d:%d" % (n, inv) if call["scratch"] else None, "dif:%d:%d" % (n, inv))]
    if call["call"] == "dist_ntt":  # one rank
        inv = call["inverse"]
        return [("natural:%d:%d" % (n, inv), "dit:%d:1" % n if inv else "dif:%d:0" % n)]
    if call["call"] == "lde_deep":  # the INTT, then the LDE (DEEP fused at the prover's shift)
        N = n + call["log_blowup"]
        return [(None, "dif:%d:1" % n), (None, "lde:%d:0:%d:0:%d" % (N, n, int(call["shift"] == 3)))]
    if call["call"] == "proof":  # the INTT, then the LDE by the DEEP polynomial or with the fused DEEP
        poly = not call["no_deep_poly"]
        return [(None, "dif:%d:1" % n), (None, "lde:%d:0:%d:%d:%d" % (n + 3, n, int(poly), int(not poly)))]
    raise AssertionError(call)


PASS_KERNEL = re.compile(r"k_ntt(_pass|4|_dif9|_w8r8|_n12r8)<")  # the recorded list holds every kernel of a call


def test_launches_match_the_recorded_trace(plans):
    rec = json.load(open(os.path.join(GOLDEN, "ntt_parent_launches.json")))
    calls = rec["calls"]
    assert {c["call"] for c in calls} == {"gl_ntt", "dist_ntt", "lde_deep", "proof"} and len(calls) > 250
    for c in calls:
        got = []
        for natural, plain in requests_of(c):
            plan = one(plans, natural) if natural else None
            if plan is None or plan["status"] == "bitrev":
                plan = one(plans, plain)
            assert plan["status"] == "ok", (c, plan["request"])
            got += [[p["kernel"], p["grid"], p["block"]] for p in plan["passes"]]
        want = [[rec["kernels"][k], grid, block] for k, grid, block in c.pop("launches")
                if PASS_KERNEL.match(rec["kernels"][k])]
        assert got == want, c
