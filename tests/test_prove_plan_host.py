"""The prover's upload plan (csrc/prove_plan.h) on the CPU: the stand-alone
tools/prove_plan_check.cpp, built with the address and undefined-behaviour
sanitizers, prints the plan of a trace shape as JSON; nothing is loaded into
Python. Checked: the planned proof length against the oracle's proofs, the FRI
workspace's regions (inside their buffers, disjoint, tiling the totals), the
forest's workgroup ranges and the upper-job ranges, the shape errors' texts,
the column work lists, the layout of the status words that come home with the
column roots, and the query requests (plan_requests, csrc/proof_host.h) over
the ranks of one world."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

U_LEVELS = 11


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prove_plan") / "prove_plan_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "prove_plan_check.cpp")],
                   check=True)

    def run(tau, step_start, what, rank=0, world=1, sharded=False, use_dict=True, expect_error=False):
        ss = [step_start] if isinstance(step_start, str) else [str(int(x)) for x in step_start]
        r = subprocess.run([exe, str(tau), str(rank), str(world), str(int(sharded)), str(int(use_dict)), what] + ss,
                           capture_output=True, text=True)
        assert r.returncode == (2 if expect_error else 0), (r.returncode, r.stderr[-2000:])
        assert r.stderr == "", r.stderr[-2000:]  # a sanitizer report
        return json.loads(r.stdout)

    return run


def uniform(n, blk):
    return list(range(0, n + 1, blk))


# ------------------------------------------------------------ proof length
@pytest.mark.parametrize("tau", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 2, 16, 1024, 4096])
def test_proof_length_matches_oracle(plan, oracle, product, n, tau):
    blk = min(n, 256)
    blocks = product.synthetic_blocks(n, blk, tau, 7)
    want = oracle.prove_v1(blocks, blocks.manifest_root())
    p = plan(tau, [int(x) for x in blocks.step_start], "proof")["proof"]
    assert p["hdr_bytes"] + p["total"] == len(want)
    # the header is the proof's, up to the column roots it leaves zero
    hdr = bytearray(want[:p["hdr_bytes"]])
    for pos in p["root_pos"]:
        hdr[pos:pos + 32] = bytes(32)
    assert hdr.hex() == p["header_hex"]


@pytest.mark.parametrize("name,blocks_file", [("minimal_riscv", "riscv_blocks.cbor"), ("root_blocks", "ref_blocks.cbor")])
def test_proof_length_matches_golden(plan, name, blocks_file):
    import cbor_min
    blocks = cbor_min.loads(open(os.path.join(GOLDEN, blocks_file), "rb").read())
    gold = json.load(open(os.path.join(GOLDEN, "v1_proofs.json")))[name]
    ss = [0]
    for b in blocks:
        ss.append(ss[-1] + len(b["movement_log"]["steps"]))
    tau = len(blocks[0]["windows"])
    p = plan(tau, ss, "proof")["proof"]
    assert p["hdr_bytes"] + p["total"] == gold["proof_len"]
    first_root = 2 * p["root_pos"][0]  # the golden head goes on into the column roots, which the plan leaves zero
    assert p["header_hex"][:first_root] == gold["head_hex"][:first_root]


# ----------------------------------------------------------- FRI workspace
def stored_nodes(log_len, lstore):
    return (1 << (log_len - lstore + 1)) - 1 if log_len >= lstore else 0


def tiles(regions, total, what):
    """regions (offset, length) are disjoint and cover [0, total) exactly."""
    at = 0
    for off, ln in sorted(r for r in regions if r[1]):
        assert off == at, (what, off, at)
        at = off + ln
    assert at == total, (what, at, total)


FRI_SHAPES = [(logn, 1, False) for logn in (0, 1, 4, 9, 10, 12, 13, 18, 19, 21, 28)] + \
             [(logn, P, True) for P in (1, 2, 4, 8)
              for logn in sorted({12 + P.bit_length() - 1, 13 + P.bit_length() - 1, 18, 19, 21})]


@pytest.mark.parametrize("logn,P,sharded", FRI_SHAPES, ids=lambda v: str(int(v)))
def test_fri_workspace(plan, logn, P, sharded):
    logP = P.bit_length() - 1
    for rank in sorted({0, P - 1}):
        out = plan(1, "logn:%d" % logn, "shape,fri", rank=rank, world=P, sharded=sharded)
        s, f = out["shape"], out["fri"]
        k = logn + 3
        assert (s["logN"], f["k"], len(f["layers"]), f["root_slots"]) == (k, k, k + 1, k + 2)
        assert s["rR"] == (k - 12 - logP if sharded else (k - 12 if k >= 12 else -1))
        assert s["tree_wg_log"] == (10 if s["M"] <= 1 << 21 else 11)
        assert s["full_lde"] == int(sharded and P == 2)
        assert f["lde_vals"] == s["M"] == (8 << logn) >> logP
        # values: each layer inside its buffer, the layers of a buffer tile it
        # (sharded: the replicated buffer starts with the whole layer rR, 4096 P values)
        size = {0: f["lde_vals"], 1: f["run_vals"], 2: f["rep_vals"]}
        vals = {0: [], 1: [], 2: [(0, 4096 << logP)] if sharded else []}
        nodes, roots = [], []
        for r, L in enumerate(f["layers"]):
            assert L["run"] == int(r <= s["rR"])
            assert L["val_len"] == ((8 << logn) >> r) >> (logP if L["run"] else 0)
            assert L["buf"] == (0 if r == 0 else 1 if L["run"] else 2)
            assert L["val_off"] + L["val_len"] <= size[L["buf"]]
            vals[L["buf"]].append((L["val_off"], L["val_len"]))
            assert (1 << L["logLen"]) == L["val_len"] and L["lstore"] == 6
            nodes.append((L["node_off"], stored_nodes(L["logLen"], 6)))
            assert L["has_cap"] == int(sharded and L["run"])
            if L["has_cap"]:
                assert (L["cap_logLen"], L["cap_lstore"]) == (k - r, 12)
                nodes.append((L["cap_off"], stored_nodes(L["cap_logLen"], 12)))
                assert L["gather_nodes"] == (8 << logn) >> r >> 12
                nodes.append((L["gather_off"], L["gather_nodes"]))
                # the local root goes to the dummy slot, the cap's to the layer's
                assert (L["root_slot"], L["cap_root_slot"]) == (k + 1, r)
            else:
                assert (L["cap_off"], L["cap_logLen"], L["cap_lstore"]) == (L["node_off"], L["logLen"], L["lstore"])
                assert L["root_slot"] == L["cap_root_slot"] == r
            roots.append(L["cap_root_slot"])
        for b in (0, 1, 2):
            tiles(vals[b], size[b], "values of buffer %d" % b)
        tiles(nodes, f["total_nodes"], "nodes")
        for off, ln in nodes:
            assert off + ln <= f["total_nodes"]
        assert roots == list(range(k + 1))  # every layer's root in its own slot, all below the dummy
        # a cap of exactly 2^12 leaves (forced-sharded P = 1 at its smallest n) stores one node
        if sharded and P == 1 and logn == 12:
            assert [L["cap_logLen"] for L in f["layers"] if L["has_cap"]][-1] == 12
        # replicated layers of >= 4096 leaves, then the tail
        assert f["rep16"] == [r for r in range(max(s["rR"] + 1, 1), k + 1) if k - r >= 12]
        assert f["tail_first"] == max(s["rR"] + 1, 1) + len(f["rep16"])
        assert f["tailbuf"] == int(not sharded)
        # forest: the replicated layers first, then run layers 1..rR; running sum of workgroups
        assert [e["layer"] for e in f["forest"]] == f["rep16"] + list(range(1, s["rR"] + 1))
        at = 0
        for e in f["forest"]:
            assert e["wg_start"] == at
            assert e["wgs"] == 1 << (f["layers"][e["layer"]]["logLen"] - s["tree_wg_log"]) >= 1
            assert e["stop"] == (s["wg_stop"] if e["layer"] <= s["rR"] else min(12, s["tree_wg_log"]))
            at += e["wgs"]
        assert f["forest_wgs"] == at
        # upper jobs: every range inside the job array, the ranges disjoint and covering it
        ranges = [tuple(p) for key in ("jobs0", "jobsF", "jobsL0", "jobsLR") for p in f[key]]
        for first, count in ranges:
            assert count > 0 and first + count <= f["njobs"]
        tiles(ranges, f["njobs"], "job ranges")
        tiles([(p["first"], p["count"]) for p in f["passes"]], f["njobs"], "job passes")
        for p in f["passes"]:
            L = f["layers"][p["layer"]]
            assert p["logLen"] == (L["cap_logLen"] if p["cap"] else L["logLen"])
            assert p["from"] <= p["logLen"] and (p["to"] == 0 or p["from"] < p["to"] <= p["logLen"])
            assert not p["gath"] or (L["has_cap"] and p["cap"] and p["from"] == 12)
        if not sharded:
            assert not f["jobsL0"] and not f["jobsLR"]
        # sharded: every run layer's cap is built from its gathered roots by exactly one first pass
        if sharded:
            assert sorted(p["layer"] for p in f["passes"] if p["gath"]) == list(range(s["rR"] + 1))


# ------------------------------------------------------------ shape errors
def test_shape_errors(plan):
    """The messages are those of the upload before its arithmetic moved into prove_plan.h."""
    e = plan(1, [0, 3000], "shape", expect_error=True)["error"]
    assert e == "n_base must be a power of two (got 3000)"
    e = plan(1, [0, 0], "shape", expect_error=True)["error"]
    assert e == "n_base must be a power of two (got 0)"
    e = plan(1, [1, 1025], "shape", expect_error=True)["error"]
    assert e == "step_start[0] must be 0"
    e = plan(1, [0, 8192], "shape", world=4, sharded=True, expect_error=True)["error"]
    assert e == "sharded proving needs n >= 4096 * P rows and P <= 8 (n = 8192, P = 4)"
    e = plan(1, [0, 2048], "shape", world=1, sharded=True, expect_error=True)["error"]
    assert e == "sharded proving needs n >= 4096 * P rows and P <= 8 (n = 2048, P = 1)"
    e = plan(1, [0, 1 << 29], "shape", expect_error=True)["error"]
    assert e == "trace too long for one device (n > 2^28)"
    # logN = log n + 3 > FS_MAX_BETAS = 64
    e = plan(1, "logn:62", "shape,fri", expect_error=True)["error"]
    assert e == "LDE domain too large for the challenge record"
    assert plan(1, [0, 4096], "shape", world=1, sharded=True)["shape"]["rR"] == 3


# ------------------------------------------------------------- column plan
def column_cases():
    yield "one_block", 2, uniform(4096, 4096), 1, False
    yield "short_blocks_dense", 2, uniform(4096, 32), 1, False       # 32 blocks per chunk: every chunk dense
    yield "mixed", 1, uniform(2048, 32) + [4096, 8192], 1, False     # two dense chunks, then piecewise ones
    yield "below_one_chunk", 3, uniform(256, 64), 1, False           # n < 1024: one chunk, no dictionary
    yield "sharded_p4", 2, uniform(8192, 32) + [16384], 4, True
    yield "forced_sharded_p1", 1, uniform(4096, 512), 1, True


@pytest.mark.parametrize("use_dict", [True, False])
@pytest.mark.parametrize("case", list(column_cases()), ids=lambda c: c[0])
def test_column_plan(plan, case, use_dict):
    _, tau, ss, P, sharded = case
    n, nblk = ss[-1], len(ss) - 1
    nchunks, chunk_rows = max(n // 1024, 1), min(n, 1024)
    for rank in range(P):
        out = plan(tau, ss, "shape,columns", rank=rank, world=P, sharded=sharded, use_dict=use_dict)
        s, c = out["shape"], out["columns"]
        ncols = 3 + 7 * tau
        assert s["ncols"] == ncols == len(c["cols"])
        lo, hi = nchunks // P * rank, nchunks // P * (rank + 1)
        assert (s["ch_lo"], s["ch_hi"]) == (lo, hi)
        # the blocks over rows [lo * 1024, hi * 1024] (the halo row, but not past the last row)
        r0, r1 = lo * chunk_rows, min(hi * chunk_rows, n - 1)
        blk_of = lambda row: max(b for b in range(nblk + 1) if ss[b] <= row)
        assert (s["blk_lo"], s["blk_lo"] + s["blk_cnt"] - 1) == (blk_of(r0), blk_of(r1))
        # labels and kinds in all_labels order
        names = ["mv", "wflag", "wsym", "head", "winlen", "in_off", "out_off"]
        for i, col in enumerate(c["cols"]):
            want = ["input_mv", "is_first", "is_last"][i] if i < 3 else "%s_%d" % (names[(i - 3) // tau], (i - 3) % tau)
            assert col["label"] == want
            assert col["kind"] == (i if i < 3 else 3 + (i - 3) // tau) and col["tape"] == (0 if i < 3 else (i - 3) % tau)
            assert (col["off"], col["block_len"]) == (12 + len(want), 20 + len(want))
        dict_on = use_dict and n >= 1024
        is_dict = lambda k: dict_on and (k == 0 or 3 <= k <= 6)
        is_pw = lambda k: k in (1, 2) or k >= 7
        kinds = [col["kind"] for col in c["cols"]]
        # dictionary columns, their table slots and the head -> mv links
        assert [d["col"] for d in c["dcols"]] == [i for i in range(ncols) if is_dict(kinds[i])]
        assert [d["tab"] for d in c["dcols"]] == [i * 5 * 65536 for i in range(len(c["dcols"]))]
        assert c["dict_of"] == [[d["col"] for d in c["dcols"]].index(i) if is_dict(kinds[i]) else -1
                                for i in range(ncols)]
        for d in c["dcols"]:
            col = c["cols"][d["col"]]
            if col["kind"] == 6:
                mv = c["cols"][c["dcols"][d["mv"]]["col"]]
                assert (mv["kind"], mv["tape"]) == (3, col["tape"])
            else:
                assert d["mv"] == -1
        # tables: disjoint, tiling tab_nodes
        tabs = []
        for i, col in enumerate(c["cols"]):
            if is_dict(col["kind"]):
                assert col["tab"] == -1 and col["tab_log"] == 0
            elif col["kind"] in (0, 3, 4, 5):
                assert col["tab_log"] == (16 if col["kind"] == 5 else 8)
                tabs.append((col["tab"], 1 << col["tab_log"]))
            elif is_pw(col["kind"]):
                tabs.append((col["tab"], (2 if col["kind"] in (1, 2) else nblk) * U_LEVELS))
            else:  # head without the dictionary: leaves computed
                assert col["kind"] == 6 and col["tab"] == -1
        tiles(tabs, c["tab_nodes"], "tables")
        assert c["tab_cols"] == [i for i, col in enumerate(c["cols"]) if col["tab"] != -1]
        assert c["pw_cols"] == [i for i in range(ncols) if is_pw(kinds[i])]
        # chunks: dense when more than 16 distinct block starts fall inside (c0, c1)
        dense = []
        for ch in range(lo, hi):
            c0 = ch * chunk_rows
            inside = len({x for x in ss[:nblk] if c0 < x < c0 + chunk_rows})
            if inside > 16:
                dense.append(ch)
        assert [ch for ch, d in enumerate(c["dense_chunk"]) if d] == dense
        assert sorted(c["pw_chunks"] + dense) == list(range(lo, hi))
        # work: every non-dictionary column for exactly its chunks
        pairs = list(zip(c["work"][0::2], c["work"][1::2]))
        assert len(set(pairs)) == len(pairs)
        for i in range(ncols):
            got = sorted(ch for col, ch in pairs if col == i)
            if is_dict(kinds[i]):
                assert got == []
            elif is_pw(kinds[i]):
                assert got == dense
            else:
                assert got == list(range(lo, hi))


# ------------------------------------------------------- the one-node cap
def test_one_node_cap_job_smallest_shape(plan):
    """plan_upper_jobs' `gath && from == top` branch (a cap of one node: the
    job copies the gathered run root into the cap and the root slot) exists
    only with one rank, where the last run layer has 4096 values: the tool
    finds the smallest shape that plans it, 2^12 rows (the smallest sharded
    shape), layer 3 of 2^15 / 8. tests/test_gpu_sharded.py proves that shape
    (test_sharded_algorithm_over_rccl_one_rank) against the oracle."""
    c = plan(2, "logn:0", "onecap", world=1, sharded=True)["onecap"]
    assert c["logn"] == 12 and c["count"] == 1
    assert (c["layer"], c["cap"], c["from"], c["to"], c["logLen"], c["lstore"]) == (3, 1, 12, 0, 12, 12)
    assert (c["wg"], c["nrun"], c["logP"]) == (0, 1, 0)
    # the same job in the full plan of that shape, and in every larger one-rank shape's last run layer
    for logn in (12, 13, 18):
        f = plan(2, "logn:%d" % logn, "fri", world=1, sharded=True)["fri"]
        caps = [p for p in f["passes"] if p["gath"] and p["from"] == p["logLen"]]
        assert len(caps) == 1 and caps[0]["count"] == 1 and caps[0]["layer"] == logn + 3 - 12, (logn, caps)
    # no other world, and no unsharded plan, has it
    for world in (2, 4, 8):
        assert plan(2, "logn:0", "onecap", world=world, sharded=True)["onecap"]["logn"] == -1
    assert plan(2, "logn:0", "onecap")["onecap"]["logn"] == -1


# ------------------------------------------------------------ status words
@pytest.mark.parametrize("use_dict", [True, False])
@pytest.mark.parametrize("tau", [1, 2, 8])
def test_status_layout_tiles(plan, tau, use_dict):
    """The small copy that comes home with the column roots (StatusLayout):
    roots, 16 guard words with the trace root at +8, 2 words per dictionary
    column, 1 per column, HW_STAT_WORDS per dictionary column, nothing else."""
    out = plan(tau, uniform(4096, 512), "columns,status", use_dict=use_dict)
    c, s = out["columns"], out["status"]
    ncols, nd = 3 + 7 * tau, len(c["dcols"])
    assert (s["ncols"], s["n_dict"]) == (ncols, nd)
    assert nd == ((1 + 4 * tau) if use_dict else 0)
    assert (s["guard_words"], s["hw_stat_words"]) == (16, 10)
    tiles([(s["roots"], 8 * ncols), (s["guard"], 16), (s["dict"], 2 * nd), (s["pw"], ncols), (s["hw"], 10 * nd)],
          s["total"], "status words")
    assert s["roots"] == 0 and s["trace_root"] == s["guard"] + 8
    assert s["total"] == 8 * ncols + 16 + (2 + 10) * nd + ncols  # the size the four places spelled out by hand


# ---------------------------------------------------------------- requests
REQ_SHAPES = [(logn, 1, False) for logn in (0, 4, 9, 10, 12)] + \
             [(logn, P, True) for P in (1, 2, 4, 8) for logn in (12 + P.bit_length() - 1, 13 + P.bit_length() - 1)]


@pytest.mark.parametrize("tau", [1, 2])
@pytest.mark.parametrize("logn,P,sharded", REQ_SHAPES, ids=lambda v: str(int(v)))
def test_requests_partition_the_proof(plan, logn, P, sharded, tau):
    """plan_requests over the ranks of one world: every FRI path record and
    every column opening of the proof is requested by exactly one rank, the
    one that owns it, within the room the proof plan allots."""
    n, N, k, NQ = 1 << logn, 8 << logn, logn + 3, 30
    seed = 1000 * logn + 10 * P + tau
    fri_ords, open_ords = [], []
    pos = None
    for rank in range(P):
        out = plan(tau, uniform(n, min(n, 256)), "shape,requests:%d" % seed, rank=rank, world=P, sharded=sharded)
        s, r = out["shape"], out["requests"]
        assert (r["max_fri_req"], r["max_open_req"]) == (NQ * 2 * k, NQ * (9 * tau + 3))
        assert r["nf"] <= r["max_fri_req"] and r["no"] <= r["max_open_req"]
        assert (len(r["fri"]), len(r["open"])) == (r["nf"], r["no"])
        assert all(x < n for x in r["rows"]) and all(x < N for x in r["frows"])
        # positions: the same on every rank, pos[q][r + 1] = pos[q][r] mod (N >> (r + 1))
        p = [r["pos"][q * (k + 1):(q + 1) * (k + 1)] for q in range(NQ)]
        assert pos is None or p == pos
        pos = p
        for q in range(NQ):
            assert p[q][0] == r["frows"][q]
            for l in range(k):
                assert p[q][l + 1] == p[q][l] % (N >> (l + 1))
        # FRI records: (layer, index, ordinal), the run owner for layers <= rR, rank 0 above them
        for layer, idx, ordn in r["fri"]:
            q, rem = divmod(ordn, 2 * k)
            assert layer == rem // 2
            assert idx == p[q][layer] ^ ((rem % 2) * (N >> (layer + 1)))
            owner = (idx >> 12) & (P - 1) if sharded and layer <= s["rR"] else 0
            assert owner == rank
            fri_ords.append(ordn)
        # openings: in proof order, by the owner of the row's chunk
        per_q = 9 * tau + 3
        for col, row, ordn, dict_ix in r["open"]:
            ch = row >> 10 if n >= 1024 else 0
            assert s["ch_lo"] <= ch < s["ch_hi"]
            q, j = divmod(ordn, per_q)
            row_q = r["rows"][q]
            nxt = row_q + 1 if row_q + 1 < n else 0
            if j < 9 * tau:
                t, f = divmod(j, 9)
                want_col = 3 + [0, 0, 1, 2, 3, 3, 4, 5, 6][f] * tau + t
                want_row = nxt if f in (1, 5) else row_q
            else:
                want_col, want_row = [1, 2, 0][j - 9 * tau], row_q
            assert (col, row) == (want_col, want_row)
            assert dict_ix == r["dict_of"][col]
            open_ords.append(ordn)
    assert sorted(fri_ords) == list(range(NQ * 2 * k))
    assert sorted(open_ords) == list(range(NQ * (9 * tau + 3)))
