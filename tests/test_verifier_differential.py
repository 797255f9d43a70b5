"""The host verifier (sezkp_stark_v1_verify: csrc/verify.cpp's parse_v1 and
decide_v1) against the independent restatement of the reference's verify_v1
(oracle/sezkp_oracle_py.py) over the corpus of tests/proof_corpus.py: honest
proofs of the smallest traces that reach every structure, a walk over every
field of the bincode layout, seeded bit flips, re-serialised shapes, forged
proofs whose Merkle paths all hold, and the shapes the batch verifier leaves
to the host. CPU only.

For every case: accept and reject are equal; on reject the check that failed
is equal (all failed bincode reads are one class) and so is the row, layer or
column the message names. The three places where the product departs from
the reference on purpose are proof_corpus.DIVERGENCES, each pinned below on
both arms; anything else that differs is a bug on one side.

The restatement's verdicts are computed with the C oracle's BLAKE3 (it shares
no code with csrc/host_crypto.cpp); test_both_hashes_give_the_same_verdict
repeats a subset with the restatement's own pure-Python BLAKE3.
"""
import pytest

import proof_corpus as PC


@pytest.fixture(scope="module")
def cases(oracle):
    return PC.corpus(oracle)


@pytest.mark.parametrize("fam", ["h", "a", "b", "c", "d", "e"])
def test_host_agrees_with_restatement(product, cases, fam):
    mine = [c for c in cases if c.family == fam]
    assert len(mine) >= {"h": 7, "a": 280, "b": 400, "c": 22, "d": 23, "e": 8}[fam]
    bad = []
    for c in mine:
        d = PC.agrees(c, PC.host_verdict(product, c.proof, c.root, c.tau))
        if d:
            bad.append((c.name, d))
    assert not bad, bad
    if fam != "e":  # e: every case carries a chain that cannot hold
        assert any(c.want is None for c in mine)


def test_random_flips_are_all_there(cases):
    b = [c for c in cases if c.family == "b"]
    assert sum("n16_t2 " in c.name for c in b) == 300 and sum("n2048_t1 " in c.name for c in b) == 100
    assert sum(c.want is None for c in b) >= 1 and sum(c.want is not None for c in b) > 300


def _both(product, oracle, name):
    c = PC.by_name(oracle, name)
    return c, PC.host_verdict(product, c.proof, c.root, c.tau)


def test_divergence_trailing_bytes(product, oracle):
    """The reference accepts a proof with bytes after it (bincode 1.3's
    top-level deserialize, lib.rs:159); the product rejects it."""
    c, host = _both(product, oracle, "c/one trailing byte")
    assert PC.divergence(c) == "trailing bytes"
    assert c.want is None
    assert host == (PC.E_VERIFY, "trailing bytes in proof")
    # a pair count one lower leaves the last pair behind the proof: the same divergence, met by the field walk
    c, host = _both(product, oracle, next(x.name for x in PC.corpus(oracle)
                                          if x.family == "a" and PC.divergence(x) == "trailing bytes"))
    assert c.want is not None and host == (PC.E_VERIFY, "trailing bytes in proof")


def test_divergence_layer_count(product, oracle):
    """A proof one FRI root short, its row queries drawn to match: the
    reference fails when the last root is not the final value's leaf; the
    product refuses the layer count before it sizes a shift with it."""
    c, host = _both(product, oracle, "d/fri_roots one fewer")
    assert PC.divergence(c) == "layer count"
    assert c.want == "final FRI value mismatch with last root"
    assert host == (PC.E_VERIFY, "FRI layer count does not match domain_n")


def test_divergence_root_argument(product, oracle):
    """The proof's own manifest root with a bit flipped and the honest root
    passed: the reference's verify_v1 never compares the two (the transcript
    changes and the row queries no longer match); the C ABI compares first."""
    c, host = _both(product, oracle, "a/n16_t2 manifest root, root passed")
    assert PC.divergence(c) == "root argument"
    assert PC.verdict_class(c.want) == "AIR query row mismatch at position "
    assert host == (PC.E_VERIFY, "manifest root mismatch")
    # without a root passed both arms give the reference's verdict
    p = PC.by_name(oracle, c.name)
    assert PC.agrees(p._replace(root=None), PC.host_verdict(product, p.proof, None, p.tau)) is None


def test_decode_errors_are_one_class(product, oracle):
    """Wording differs ('bad length prefix' / 'truncated proof bytes' / 'column
    label is not valid UTF-8' against the restatement's), code and class do not."""
    seen = set()
    for c in PC.corpus(oracle):
        if PC.verdict_class(c.want) == "parse" and PC.divergence(c) is None:
            code, msg = PC.host_verdict(product, c.proof, c.root, c.tau)
            assert code == PC.E_DECODE, (c.name, code, msg)
            seen.add(msg)
    assert {"bad length prefix", "truncated proof bytes", "column label is not valid UTF-8"} <= seen


def test_forgeries_reach_the_checks_they_name(oracle):
    """Family d by verdict: each algebraic or structural check of decide_v1 is
    the restatement's verdict on a proof whose Merkle paths all hold."""
    d = {c.name[2:]: c.want for c in PC.family(oracle, "d")}
    assert d["layer 1 + 1"] == "FRI fold mismatch at layer 0"
    assert d["layer 4 + 1"] == "FRI fold mismatch at layer 3"
    assert d["layer 6 + 1"] == "FRI fold mismatch at layer 5"
    assert d["layer 7 + 1 (the final value)"] == "final FRI value mismatch"
    assert d["fri_roots = []"] == "no FRI roots"
    for name in ("wflag = 2", "wflag = 2 on the still trace", "mv = 2", "head + 1 on odd rows", "wrong in_off",
                 "wrong out_off", "is_last = 2", "v + p with mv = 2", "v + p with wflag = 2", "next_row = row"):
        assert d[name].startswith("AIR composition non-zero at row "), (name, d[name])
    for name in ("is_first = p - 1", "mv +2 / -2 across tapes", "one-row-block boundary cancellation",
                 "every value written as v + p", "next_row = row + 5 on the still trace"):
        assert d[name] is None, (name, d[name])


# an accept, an AIR reject, a column path reject, a FRI path reject, a fold reject, and the other stages
_SUBSET = ("h/n16_t2", "h/n1_t1", "d/every value written as v + p", "d/wflag = 2", "d/is_last = 2",
           "d/layer 4 + 1", "d/layer 7 + 1 (the final value)", "d/fri_roots = []", "d/query_rows shifted by one",
           "c/empty path_in", "c/70 FRI siblings", "c/label not UTF-8", "c/domain_n = 24", "c/position dropped")


def test_both_hashes_give_the_same_verdict(oracle):
    import sezkp_oracle_py as V
    classes = set()
    for name in _SUBSET:
        c = PC.by_name(oracle, name)
        assert V.verify_v1(c.proof, c.tau or None) == c.want, name  # the pure-Python BLAKE3
        classes.add(PC.verdict_class(c.want))
    assert {None, "AIR composition non-zero at row ", "chunked merkle path failed for column head_",
            "FRI Merkle path failed at layer ", "FRI fold mismatch at layer "} <= classes
    # and the hooked prover writes the same bytes under either hash
    blocks, _ = PC.BASES["n16_t2"]()
    root = oracle.manifest_root(oracle.Blocks(blocks))
    forge = {"layer": lambda r, v: [x + 1 for x in v] if r == 2 else v}
    assert V.prove_v1(blocks, root, forge=forge) == V.prove_v1(blocks, root, forge=forge, blake3=oracle.blake3)
