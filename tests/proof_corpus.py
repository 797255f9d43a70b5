"""Proofs for the verifier's differential tests, shared by the CPU module
(test_verifier_differential.py) and the GPU module
(test_gpu_verify_differential.py). A plain helper, no fixtures.

`corpus(oracle)` returns the named cases, built once per session. Each case
carries its proof bytes, the manifest root passed to the verifier (or None),
the tau passed (0: not checked) and `want`, the verdict of the independent
restatement of the reference's verify_v1 (oracle/sezkp_oracle_py.py) computed
with the C oracle's BLAKE3: None for accepted, else the reference's message.

Honest proofs come from the C oracle's prover, forged ones from the hooked
pure-Python prover (sezkp_oracle_py.prove_v1(forge=...)): neither shares code
with the product's verifier.

Families
  a  field walk: every field class of the bincode layout, first / middle /
     last instance, lowest and highest bit
  b  seeded random single-bit flips
  c  re-serialised shapes (the bincode writer below)
  d  forgeries whose Merkle paths all hold: only an algebraic or structural
     check can reject them, and some the reference accepts
  e  shapes whose chains the batch verifier leaves to the host (more than 1024
     siblings, label ids from 2^16 on), and the 1024-sibling boundary

The builder asserts, on the restatement's verdicts alone, that every forged
case does what it declares (so a forgery that is a no-op fails here), that
every message verify_v1 can return is some case's verdict, and that
acceptance occurs in each of a-d.
"""
import ctypes as C
import inspect
import random
import re
import struct
from collections import namedtuple

P = 0xFFFFFFFF00000001
E_INVALID, E_DECODE, E_VERIFY = -1, -4, -5

# shape: (bytes after the ProofV1, FRI roots, domain_n) as the restatement reads them, None if it cannot
Case = namedtuple("Case", "name family proof root tau want shape")
ACCEPTS = None  # a forged case's declaration: the reference accepts it


# ----------------------------------------------------------------- verdicts
def normalise(msg):
    """A verdict without the values only the reference's wording carries:
    'tau mismatch vs. block windows: got 3, expected 2' and 'AIR query count
    mismatch (expected 30, got 31)' lose their tails; the row, layer or column
    a message names stays."""
    for cut in (": got ", " (expected "):
        if cut in msg:
            msg = msg[:msg.index(cut)]
    return msg


def verdict_class(msg):
    """The check that failed: the message up to its first digit or ' @'; every
    failed bincode read is the one class 'parse'; None is acceptance."""
    import sezkp_oracle_py as V
    if msg is None:
        return None
    if msg.startswith(V.DECODE_ERROR):
        return "parse"
    return re.split(r"\d| @", normalise(msg))[0]


def host_verdict(product, proof, root=None, tau=0):
    """(code, message) of sezkp_stark_v1_verify; tau != 0: checked against the
    blocks' tau (the call reads n_blocks and tau of the view, nothing else)."""
    from sezkp_amd._lib import BlockView
    view = BlockView()
    view.n_blocks, view.tau = (1, tau) if tau else (0, 0)
    err = C.create_string_buffer(1024)
    buf = C.create_string_buffer(bytes(proof), len(proof)) if len(proof) else C.create_string_buffer(1)
    rc = product.lib.sezkp_stark_v1_verify(C.cast(buf, C.c_char_p), len(proof), C.byref(view),
                                           bytes(root) if root is not None else None, err, 1024)
    return rc, (err.value.decode(errors="replace") if rc else "")


# Where the product's verifier departs from the reference on purpose
# (include/sezkp_stark.h): entry -> the product's (code, message)
# wherever divergence(case) names that entry, whatever the reference says
# there. Every other case must agree. The wording of a decode error differs
# too ('bad length prefix', 'truncated proof bytes', ... against bincode's):
# all failed reads are one class.
DIVERGENCES = {
    # The reference compares the root it is given with the artifact envelope's (lib.rs:154-157) and
    # never with the proof's own copy, which only enters the transcript. The C ABI has no envelope:
    # it compares the root it is given with the proof's last 32 bytes, before anything else.
    "root argument": (E_VERIFY, "manifest root mismatch"),
    # bincode 1.3's top-level deserialize ignores bytes after the value (lib.rs:159); a verifier
    # library should not accept two encodings of one proof. Checked when the walk ends.
    "trailing bytes": (E_VERIFY, "trailing bytes in proof"),
    # The layer count comes from the untrusted proof and sizes a shift: the product wants
    # log2(domain_n) + 1 layers before FRI starts; the reference goes on with what it is given.
    "layer count": (E_VERIFY, "FRI layer count does not match domain_n"),
}
_FRI_STAGE = (None, "final FRI value mismatch with last root", "positions length mismatch", "pairs length mismatch",
              "FRI Merkle path failed at layer ", "FRI index propagation failed at layer ",
              "FRI fold mismatch at layer ", "final FRI value mismatch")


def divergence(case):
    """The entry of DIVERGENCES that governs this case, or None. Decided from
    the bytes as the restatement reads them and from its verdict, in the
    order in which the product makes these checks."""
    if case.root is not None and len(case.proof) >= 40 and case.proof[-32:] != case.root:
        return "root argument"
    if case.shape is None:  # not a ProofV1: a decode error on both sides
        return None
    trailing, n_layers, domain_n = case.shape
    if trailing:
        return "trailing bytes"
    if n_layers and (n_layers > 64 or 1 << (n_layers - 1) != domain_n) and verdict_class(case.want) in _FRI_STAGE:
        return "layer count"  # the reference got as far as fri_verify's layers
    return None


def agrees(case, host):
    """None when the product's (code, message) matches the restatement's
    verdict for this case under the rules above, else what differs."""
    code, msg = host
    d = divergence(case)
    if d is not None:
        return None if host == DIVERGENCES[d] else f"{d}: restatement {case.want!r}, product {host!r}"
    if (code == 0) != (case.want is None):
        return f"restatement {case.want!r}, product {host!r}"
    if case.want is None:
        return None
    if verdict_class(case.want) == "parse" or code == E_DECODE:
        ok = verdict_class(case.want) == "parse" and code == E_DECODE
    else:
        ok = code == E_VERIFY and normalise(case.want) == msg
    return None if ok else f"restatement {case.want!r}, product {host!r}"


# ------------------------------------------------------------------ layout
def _layout(b):
    """Byte offsets of a bincode ProofV1 (proof.rs:80-98), the arithmetic of
    test_verifier.py made a walk: openings as dicts of field offsets."""
    u64 = lambda o: struct.unpack_from("<Q", b, o)[0]
    L = {"cols": [], "rows": [], "fq": []}
    p = 16
    ncols = u64(p); L["ncols_at"] = p; p += 8
    for _ in range(ncols):
        ll = u64(p)
        L["cols"].append({"len_at": p, "label": p + 8, "label_len": ll, "root": p + 8 + ll})
        p += 8 + ll + 32
    L["hdr"] = p

    def opening(p):
        a = u64(p + 64)
        bq = u64(p + 72 + 32 * a)
        o = {"value": p, "index": p + 8, "chunk_index": p + 16, "index_in_chunk": p + 24, "chunk_root": p + 32,
             "n_in_at": p + 64, "path_in": p + 72, "n_in": a, "n_to_at": p + 72 + 32 * a,
             "path_to": p + 80 + 32 * a, "n_to": bq}
        return o, p + 80 + 32 * (a + bq)
    L["nq_at"] = p
    nq = u64(p); p += 8
    for _ in range(nq):
        row = {"row": p, "nt_at": p + 8, "opens": []}
        nt = u64(p + 8); p += 16
        for _ in range(9 * nt + 3):
            o, p = opening(p)
            row["opens"].append(o)
        L["rows"].append(row)
    L["nroots_at"] = p
    nr = u64(p); p += 8
    L["roots"] = p; p += 32 * nr
    L["nroots"] = nr
    L["nfq_at"] = p
    nfq = u64(p); p += 8
    for _ in range(nfq):
        q = {"npos_at": p, "pos": p + 8, "pairs": []}
        npos = u64(p); p += 8 + 8 * npos
        q["npos"] = npos
        q["npairs_at"] = p
        npairs = u64(p); p += 8
        for _ in range(npairs):
            a = u64(p + 8)
            c = u64(p + 16 + 32 * a + 8)
            q["pairs"].append({"vi": p, "path_i": p + 16, "n_i": a, "vj": p + 16 + 32 * a,
                               "path_j": p + 32 + 32 * a, "n_j": c})
            p += 32 + 32 * (a + c)
        L["fq"].append(q)
    L["final"] = p
    L["mroot"] = p + 8
    assert p + 40 == len(b)
    return L


def _flip(proof, at, bit=0):
    b = bytearray(proof)
    b[at] ^= 1 << bit
    return bytes(b)


# ------------------------------------------------------------- bincode writer
def _write_proof(pf):
    """bincode 1.3 fixint LE writer over sezkp_oracle_py.parse_proof_v1's
    output (a label may be given as bytes, to write one that is not UTF-8)."""
    u64 = lambda x: struct.pack("<Q", x)
    vec32 = lambda v: u64(len(v)) + b"".join(v)

    def opening(o):
        return (o["value_le"] + u64(o["index"]) + u64(o["chunk_index"]) + u64(o["index_in_chunk"]) + o["chunk_root"] +
                vec32(o["path_in_chunk"]) + vec32(o["path_to_chunk"]))
    out = [u64(pf["domain_n"]), u64(pf["tau"]), u64(len(pf["col_roots"]))]
    for lab, r in pf["col_roots"]:
        lb = lab if isinstance(lab, bytes) else lab.encode()
        out += [u64(len(lb)), lb, r]
    out.append(u64(len(pf["queries"])))
    for q in pf["queries"]:
        out += [u64(q["row"]), u64(len(q["per_tape"]))]
        for t in q["per_tape"]:
            out += [opening(t[k]) for k in ("mv", "next_mv", "write_flag", "write_sym", "head", "next_head", "win_len",
                                            "in_off", "out_off")]
        out += [opening(q[k]) for k in ("is_first", "is_last", "input_mv")]
    out.append(vec32(pf["fri_roots"]))
    out.append(u64(len(pf["fri_queries"])))
    for f in pf["fri_queries"]:
        out += [u64(len(f["positions"]))] + [u64(x) for x in f["positions"]] + [u64(len(f["pairs"]))]
        for vi, pi, vj, pj in f["pairs"]:
            out += [vi, vec32(pi), vj, vec32(pj)]
    out += [pf["fri_final_value_le"], pf["manifest_root"]]
    return b"".join(out)


# ------------------------------------------------------------------- traces
def _blocks(T, B, tau, mv=lambda j, r, k: 0, write=lambda j, r, k: None):
    """T rows in blocks of B as the block file's dicts. mv(j, r, k) and
    write(j, r, k): the move and the written symbol (or None) of row j of block
    k on tape r. Heads start at 0 in every block, so in_off = 0 and out_off =
    the block's last head satisfy the boundary terms."""
    out = []
    for k in range(T // B):
        steps, heads = [], [0] * tau
        for j in range(B):
            ops = []
            for r in range(tau):
                heads[r] += mv(j, r, k)
                assert 0 <= heads[r] <= 3
                ops.append({"mv": mv(j, r, k), "write": write(j, r, k)})
            steps.append({"input_mv": 0, "tapes": ops})
        out.append({"version": 1, "block_id": k + 1, "step_lo": k * B + 1, "step_hi": (k + 1) * B, "ctrl_in": 0,
                    "ctrl_out": 0, "in_head_in": 0, "in_head_out": 0,
                    "windows": [{"left": 0, "right": 3} for _ in range(tau)], "head_in_offsets": [0] * tau,
                    "head_out_offsets": list(heads), "movement_log": {"steps": steps}})
    return out


_MOVES = ((1, 1, -1, 0), (1, 0, 1, -1), (0, 1, 1, 0), (1, -1, 1, 1))  # heads stay in 0..2, end at 1, 1, 2, 2


def _varied():
    """16 rows, blocks of 4, tau = 2, a valid AIR with non-zero moves, writes
    and last heads: on it a forged term multiplies something other than 0."""
    return _blocks(16, 4, 2, mv=lambda j, r, k: _MOVES[(k + r) % 4][j],
                   write=lambda j, r, k: (j + k) % 16 if (j + k + r) % 3 == 0 else None)


BASES = {  # name -> (blocks, tau); all but `varied` are still traces (no moves, no writes)
    "n16_t2": lambda: (_blocks(16, 4, 2), 2),
    "varied": lambda: (_varied(), 2),
    "n2048_t1": lambda: (_blocks(2048, 256, 1), 1),  # two column chunks: path_to_chunk has one sibling
    "n1_t1": lambda: (_blocks(1, 1, 1), 1),          # N = 8, first == last row, next row = row 0
    "n16_t0": lambda: (_blocks(16, 4, 0), 0),
    "n16_t11": lambda: (_blocks(16, 4, 11), 11),     # tapes 10 and over: two-digit labels
    "n16_b1_t2": lambda: (_blocks(16, 1, 2), 2),     # one-row blocks: every row is first and last
}


# ------------------------------------------------------------------ builder
class _Builder:
    def __init__(self, oracle):
        import sezkp_oracle_py as V
        self.V, self.oracle = V, oracle
        self.cases = []
        self.blocks, self.root, self.honest = {}, {}, {}
        for name, make in BASES.items():
            blocks, _tau = make()
            self.blocks[name] = blocks
            ob = oracle.Blocks(blocks)
            self.root[name] = oracle.manifest_root(ob)
            self.honest[name] = oracle.prove_v1(ob, self.root[name])

    def tau(self, base):
        return len(self.blocks[base][0]["windows"])

    def verdict(self, proof, tau):
        return self.V.verify_v1(proof, tau or None, blake3=self.oracle.blake3)

    def add(self, family, name, proof, root=None, tau=0):
        try:
            pf = self.V.parse_proof_v1(proof)
            shape = (pf["trailing"], len(pf["fri_roots"]), pf["domain_n"])
        except ValueError:
            shape = None
        c = Case(f"{family}/{name}", family, bytes(proof), root, tau, self.verdict(proof, tau), shape)
        if shape and shape[0]:  # the reference does not see the bytes after the proof
            assert c.want == self.verdict(proof[:len(proof) - shape[0]], tau)
        self.cases.append(c)
        return c

    def parsed(self, base):
        return self.V.parse_proof_v1(self.honest[base])

    # --------------------------------------------------------------- honest
    def honest_cases(self):
        for base, p in self.honest.items():
            c = self.add("h", base, p, self.root[base], self.tau(base))
            assert c.want is None, (base, c.want)  # every base trace satisfies the AIR
        # the hooked prover without hooks writes the C prover's bytes
        for base in ("n16_t2", "varied", "n1_t1", "n16_t0"):
            assert self.V.prove_v1(self.blocks[base], self.root[base], blake3=self.oracle.blake3) == self.honest[base]

    # ----------------------------------------------------------- a: field walk
    def field_walk(self, base):
        p, tau = self.honest[base], self.tau(base)
        L = _layout(p)
        pick3 = lambda xs: [xs[i] for i in sorted({0, len(xs) // 2, len(xs) - 1})]
        fields = [("domain_n", [0], 8), ("tau", [8], 8), ("ncols", [L["ncols_at"]], 8)]
        cols = pick3(L["cols"])
        fields.append(("label length", [c["len_at"] for c in cols], 8))
        fields += [("label byte", [c["label"]], c["label_len"]) for c in cols]
        fields.append(("column root", [c["root"] for c in cols], 32))
        fields.append(("nq", [L["nq_at"]], 8))
        rows = pick3(L["rows"])
        fields.append(("row", [r["row"] for r in rows], 8))
        fields.append(("nt", [r["nt_at"] for r in rows], 8))
        opens = pick3([o for r in L["rows"] for o in r["opens"]])
        for f, w in (("value", 8), ("index", 8), ("chunk_index", 8), ("index_in_chunk", 8), ("chunk_root", 32),
                     ("n_in_at", 8), ("n_to_at", 8)):
            fields.append((f"opening {f}", [o[f] for o in opens], w))
        fields.append(("path_in sibling", [o["path_in"] + 32 * (o["n_in"] // 2) for o in opens if o["n_in"]], 32))
        fields.append(("path_to sibling", [o["path_to"] + 32 * (o["n_to"] // 2) for o in opens if o["n_to"]], 32))
        k = L["nroots"] - 1
        fields.append(("nroots", [L["nroots_at"]], 8))
        fields.append(("FRI root", [L["roots"] + 32 * i for i in sorted({0, k // 2, k})], 32))
        fields.append(("nfq", [L["nfq_at"]], 8))
        fqs = pick3(L["fq"])
        fields.append(("npos", [q["npos_at"] for q in fqs], 8))
        fields.append(("position", [q["pos"] + 8 * i for q, i in zip(fqs, (0, k // 2, k))], 8))
        fields.append(("npairs", [q["npairs_at"] for q in fqs], 8))
        pairs = [q["pairs"][i] for q, i in zip(fqs, (0, k // 2, k - 1))]
        fields.append(("vi", [x["vi"] for x in pairs], 8))
        fields.append(("vj", [x["vj"] for x in pairs], 8))
        fields.append(("path_i sibling", [x["path_i"] + 32 * (x["n_i"] // 2) for x in pairs], 32))
        fields.append(("path_j sibling", [x["path_j"] + 32 * (x["n_j"] // 2) for x in pairs], 32))
        fields.append(("final value", [L["final"]], 8))
        fields.append(("manifest root", [L["mroot"]], 32))
        for what, ats, width in fields:
            if what in ("path_to sibling",) and not ats:
                continue  # a one-chunk column has no sibling above its chunk root
            for at in ats:
                for nm, (a, bit) in (("low", (at, 0)), ("high", (at + width - 1, 7))):
                    self.add("a", f"{base} {what} @{at} {nm} bit", _flip(p, a, bit), None, tau)
        self.add("a", f"{base} manifest root, root passed", _flip(p, L["mroot"] + 31), self.root[base], tau)

    # ------------------------------------------------------- b: random flips
    def random_flips(self, base, count, seed):
        p, rng = self.honest[base], random.Random(seed)
        for i in range(count):
            at, bit = rng.randrange(len(p)), rng.randrange(8)
            self.add("b", f"{base} flip {i:03d} byte {at} bit {bit}", _flip(p, at, bit), None, self.tau(base))

    # ------------------------------------------------------- c: re-serialised
    def reserialised(self):
        base = "n16_t2"
        p = self.honest[base]
        assert _write_proof(self.parsed(base)) == p

        def edited(name, edit, tau=0):
            pf = self.parsed(base)
            edit(pf)
            return self.add("c", name, _write_proof(pf), None, tau)

        def f(pf):
            pf["queries"][4]["per_tape"][1]["head"]["path_in_chunk"] = []
        edited("empty path_in", f)

        def f(pf):
            vi, pi, vj, pj = pf["fri_queries"][7]["pairs"][2]
            pf["fri_queries"][7]["pairs"][2] = (vi, pi + [bytes([i]) * 32 for i in range(70 - len(pi))], vj, pj)
        edited("70 FRI siblings", f)

        def f(pf):
            for q in pf["queries"]:
                q["per_tape"] = []
        edited("0 tapes per row", f)  # the three row columns hold and the AIR sum is empty: accepted

        def f(pf):
            pf["fri_roots"] = pf["fri_roots"][:-1]
        edited("one layer fewer", f)

        def f(pf):
            pf["fri_roots"] = pf["fri_roots"] + [pf["fri_roots"][-1]]
        edited("one layer more", f)
        for n in (0, 1, 39, 40, len(p) - 1):
            self.add("c", f"truncated to {n}", p[:n])

        def f(pf):
            pf["fri_queries"][3]["positions"].pop()
        edited("position dropped", f)

        def f(pf):
            pf["fri_queries"][3]["pairs"].pop()
        edited("pair dropped", f)

        def f(pf):
            pf["queries"].append(pf["queries"][-1])
        edited("31st row query", f)

        def f(pf):
            pf["queries"].pop()
        edited("29th row query is the last", f)

        def f(pf):
            lab, r = pf["col_roots"][5]
            pf["col_roots"][5] = (b"\xff" + lab.encode()[1:], r)
        edited("label not UTF-8", f)

        def f(pf):
            lab, r = pf["col_roots"][5]
            pf["col_roots"][5] = (b"\xed\xa0\x80" + lab.encode(), r)  # a surrogate: UTF-8 in form, not a Rust str
        edited("label with a surrogate", f)

        def f(pf):
            lab, r = pf["col_roots"][3]
            pf["col_roots"].append((lab, bytes(32)))  # the later root wins in the reference's map
        edited("column root listed twice", f)
        self.add("c", "one trailing byte", p + b"\0")
        for dn in (0, 12, 24):
            def f(pf):
                pf["domain_n"] = dn
            edited(f"domain_n = {dn}", f)
        self.add("c", "honest, tau not checked", p)

    # ---------------------------------------------------------- d: forgeries
    def forged(self, name, base, forge, expect, tau=None):
        """A proof from the hooked prover. `expect`: the class of the verdict
        the restatement must give, or ACCEPTS. Either way the bytes must differ
        from the honest proof's."""
        p = self.V.prove_v1(self.blocks[base], self.root[base], forge=forge, blake3=self.oracle.blake3)
        assert p != self.honest[base], f"{name}: the forgery changed nothing"
        c = self.add("d", name, p, self.root[base], self.tau(base) if tau is None else tau)
        assert verdict_class(c.want) == expect, f"{name}: declared {expect!r}, restatement says {c.want!r}"
        return c

    def forgeries(self):
        AIR = "AIR composition non-zero at row "
        k = 7  # n = 16: N = 128, layers 0..7

        def every_row(**cols):
            def hook(rows, tau):
                for i, r in enumerate(rows):
                    for lab, v in cols.items():
                        r[lab] = v(i, r) if callable(v) else v
                return rows
            return {"rows": hook}
        for r in (1, 4, k - 1):
            self.forged(f"layer {r} + 1", "varied", {"layer": lambda rr, v, r=r: [x + 1 for x in v] if rr == r else v},
                        "FRI fold mismatch at layer ")
        self.forged(f"layer {k} + 1 (the final value)", "varied",
                    {"layer": lambda rr, v: [x + 1 for x in v] if rr == k else v}, "final FRI value mismatch")
        self.forged("wflag = 2", "varied", every_row(wflag_0=2), AIR)            # bool_flag
        self.forged("wflag = 2 on the still trace", "n16_t2", every_row(wflag_1=2), AIR)
        self.forged("mv = 2", "varied", every_row(mv_0=2), AIR)                  # mv_domain (and head_update)
        self.forged("head + 1 on odd rows", "varied", every_row(head_0=lambda i, r: r["head_0"] + (i & 1)), AIR)
        self.forged("wrong in_off", "varied", every_row(in_off_1=1), AIR)        # boundary_first
        self.forged("wrong out_off", "varied", every_row(out_off_1=lambda i, r: r["out_off_1"] + 1), AIR)
        # (1 - 2)(next head - head - next mv) + 2 (head - out_off) = -head on a last row: the last heads are 1 or 2
        self.forged("is_last = 2", "varied", every_row(is_last=lambda i, r: 2 * r["is_last"]), AIR)
        # is_first only ever multiplies head - mv - in_off, which is 0 on an honest first row
        self.forged("is_first = p - 1", "varied", every_row(is_first=lambda i, r: (P - 1) * r["is_first"]), ACCEPTS)
        # 2 * 1 * 3 on tape 0 and (-2)(-3)(-1) on tape 1 share alpha_1; the heads follow the moves
        self.forged("mv +2 / -2 across tapes", "n16_t2",
                    every_row(mv_0=2, mv_1=-2, head_0=lambda i, r: 2 * (i % 4 + 1), head_1=lambda i, r: -2 * (i % 4 + 1),
                              out_off_0=8, out_off_1=-8), ACCEPTS)
        # on a one-row block head - mv - in_off = -1 and head - out_off = +1 share alpha_2
        self.forged("one-row-block boundary cancellation", "n16_b1_t2",
                    every_row(mv_0=1, head_0=1, in_off_0=1, out_off_0=0), ACCEPTS)
        plus_p = lambda lab, v: v + P if v < 2 ** 32 - 1 else v
        self.forged("every value written as v + p", "varied", {"enc": plus_p}, ACCEPTS)
        self.forged("v + p with mv = 2", "varied", dict(every_row(mv_0=2), enc=plus_p), AIR)
        self.forged("v + p with wflag = 2", "n16_t2", dict(every_row(wflag_0=2), enc=plus_p), AIR)
        self.forged("next_row = row", "varied", {"next_row": lambda row: row}, AIR)
        self.forged("next_row = row + 5 on the still trace", "n16_t2", {"next_row": lambda row: (row + 5) % 16}, ACCEPTS)
        self.forged("query_rows shifted by one", "varied", {"query_rows": lambda q: [(x + 1) % 16 for x in q]},
                    "AIR query row mismatch at position ")
        self.forged("fri_roots = []", "varied", {"fri_roots": lambda r: []}, "no FRI roots")
        self.forged("fri_roots one fewer", "varied", {"fri_roots": lambda r: r[:-1]},
                    "final FRI value mismatch with last root")
        self.forged("wflag = 2, wrong tau passed", "varied", every_row(wflag_0=2), "tau mismatch vs. block windows", tau=3)

    # ------------------------------------------------------ e: host fallback
    def host_fallback(self):
        base = "n16_t2"
        junk = lambda n, have: [struct.pack("<Q", i) * 4 for i in range(n - len(have))]

        def edited(name, edit):
            pf = self.parsed(base)
            edit(pf)
            return self.add("e", name, _write_proof(pf), self.root[base], 2)
        for n in (1025, 1024):  # 1025: answered on the host inside the call; 1024: the longest chain the kernel gets
            def f(pf):
                vi, pi, vj, pj = pf["fri_queries"][0]["pairs"][0]
                pf["fri_queries"][0]["pairs"][0] = (vi, pi + junk(n, pi), vj, pj)
            edited(f"{n} siblings, first FRI pair of query 0", f)  # job 0, in front of every device job

            def f(pf):
                o = pf["queries"][15]["per_tape"][0]["head"]
                o["path_in_chunk"] = o["path_in_chunk"] + junk(n, o["path_in_chunk"])
            edited(f"{n} siblings, path_in of a middle opening", f)

            def f(pf):
                o = pf["queries"][29]["input_mv"]  # the last opening of the file: the last job of the proof
                o["path_to_chunk"] = o["path_to_chunk"] + junk(n, o["path_to_chunk"])
            edited(f"{n} siblings, path_to of the last opening", f)

        # A host job in front of a device chain that fails between chains that hold: were the result words
        # numbered over the device jobs only, the 0 would land one word early, on the path_to job of the
        # opening before (another column), and the verdict would name that column.
        def flipped(o):
            s = bytearray(o["path_in_chunk"][1])
            s[9] ^= 0x10
            o["path_in_chunk"] = o["path_in_chunk"][:1] + [bytes(s)] + o["path_in_chunk"][2:]

        def f(pf):
            vi, pi, vj, pj = pf["fri_queries"][0]["pairs"][0]
            pf["fri_queries"][0]["pairs"][0] = (vi, pi + junk(1025, pi), vj, pj)
            flipped(pf["queries"][15]["per_tape"][0]["head"])
        c = edited("1025 siblings on the first FRI pair, then a path_in sibling flipped", f)
        assert c.want.startswith("chunked merkle path failed for column head_0 @ "), c.want

        def f(pf):  # label ids 3 + 7 t + u: 65530..65536 in tape 9361, so its out_off opening is the host's
            q = pf["queries"][7]
            blank = dict(q["per_tape"][0]["mv"], path_in_chunk=[], path_to_chunk=[])
            q["per_tape"] = q["per_tape"] + [{kk: blank for kk in q["per_tape"][0]}] * 9360
            assert 3 + 7 * 9361 + 6 == 65536
        c = edited("9362 tapes in one row query", f)
        assert c.want == "missing col root for mv_2", c.want

    # -------------------------------------------------------------- coverage
    def check_coverage(self):
        src = inspect.getsource(self.V._verify_v1)
        msgs = re.findall(r'return f?"([^"]*)"', src)
        assert len(msgs) == 16, msgs
        seen = {verdict_class(c.want) for c in self.cases}
        assert "parse" in seen
        for m in msgs:  # a message that names a row, layer or column: its text before the name; else all of it
            head = normalise(m).split("{")[0]
            assert any(s is not None and (s.startswith(head) if "{" in m else s == head) for s in seen), m
        for fam in "abcd":
            assert any(c.want is None for c in self.cases if c.family == fam), f"no accepted case in family {fam}"
        names = [c.name for c in self.cases]
        assert len(set(names)) == len(names)
        assert set(DIVERGENCES) == {divergence(c) for c in self.cases} - {None}


_CORPUS = []


def corpus(oracle):
    """The list of cases, built once per session (oracle: the oracle_ctypes module)."""
    if not _CORPUS:
        b = _Builder(oracle)
        b.honest_cases()
        b.field_walk("n16_t2")
        b.field_walk("n2048_t1")
        b.random_flips("n16_t2", 300, 20240611)
        b.random_flips("n2048_t1", 100, 20240612)
        b.reserialised()
        b.forgeries()
        b.host_fallback()
        b.check_coverage()
        _CORPUS.extend(b.cases)
    return _CORPUS


def family(oracle, fam):
    return [c for c in corpus(oracle) if c.family == fam]


def by_name(oracle, name):
    return next(c for c in corpus(oracle) if c.name == name)
