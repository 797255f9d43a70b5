"""Batch verification on the GPU (sezkp_ctx_verify_batch, k_verify_chains)
over the differential corpus of tests/proof_corpus.py. For every case the
batch result's (code, message) equals the host verifier's for the same bytes,
root and tau, and agrees with the verdict of the independent restatement of
the reference's verify_v1 under the rules of test_verifier_differential.py
(proof_corpus.agrees): the GPU arm is compared with a yardstick that shares
no code with verify.cpp, not only with its sibling.

Family e holds the chains the batch verifier leaves to the host (VJ_HOST:
more than 1024 siblings, label ids from 2^16 on). The result words are
numbered over all jobs of a slice and the device job table over the device
jobs only; e's cases put host jobs in front of, between and behind device
jobs whose outcomes differ, alone, in mixed batches and in slices of their
own, so a slip between the two counters changes a verdict.

Every input is bytes the host parser has bounds-checked before a job names
them (tools/verify_hostile.cpp runs the same corpus under host sanitizers).
"""
import pytest

import proof_corpus as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(oracle):
    return PC.corpus(oracle)


@pytest.fixture(scope="module")
def ctx(product, gpu_ok):
    c = product.ProverContext(0)
    yield c
    c.close()


def _gpu(ctx, cs):
    res = ctx.verify_batch([c.proof for c in cs], [c.root for c in cs], [c.tau for c in cs])
    for r in res:
        assert r.ok == (r.code == 0)
    return [(r.code, r.message) for r in res]


def _check(product, ctx, cs):
    """One batch call; each verdict equal to the host's and in agreement with the restatement's."""
    got = _gpu(ctx, cs)
    assert len(got) == len(cs)
    bad = []
    for c, g in zip(cs, got):
        h = PC.host_verdict(product, c.proof, c.root, c.tau)
        d = PC.agrees(c, g)
        if g != h or d:
            bad.append((c.name, g, h, d))
    assert not bad, bad
    return got


def _jobs(case):
    """The Merkle chains of a case's proof, host jobs included: two per FRI pair
    of a query the checks can walk, the final value's, and per opening path_in
    and, where the label has a column root, path_to (verify_plan.h)."""
    import sezkp_oracle_py as V
    pf = V.parse_proof_v1(case.proof)
    nl, labels = len(pf["fri_roots"]), {lab for lab, _ in pf["col_roots"]}
    n = 1 if nl else 0
    if nl and 1 << (nl - 1) == pf["domain_n"]:
        n += sum(2 * len(f["pairs"]) for f in pf["fri_queries"]
                 if len(f["positions"]) == nl and len(f["pairs"]) == nl - 1)
    kinds = ("mv", "mv", "wflag", "wsym", "head", "head", "winlen", "in_off", "out_off")
    for q in pf["queries"]:
        n += sum(1 + (lab in labels) for lab in ("input_mv", "is_first", "is_last"))
        n += sum(1 + (f"{k}_{t}" in labels) for t in range(len(q["per_tape"])) for k in kinds)
    return n


# ---------------------------------------------------------------------------
# First in the module, on a context of its own: the label table is created by
# the first batch and only ever grows.
def test_two_digit_labels_and_label_table_growth(product, gpu_ok, cases, oracle):
    import sezkp_oracle_py as V
    h11, h2 = PC.by_name(oracle, "h/n16_t11"), PC.by_name(oracle, "h/n16_t2")
    big = PC.by_name(oracle, "e/9362 tapes in one row query")
    L = PC._layout(h11.proof)
    o = L["rows"][11]["opens"][9 * 10 + 8]  # tape 10's out_off: the label is out_off_10
    p = PC._flip(h11.proof, o["path_in"] + 32 + 17, 3)
    want = V.verify_v1(p, 11, blake3=oracle.blake3)
    assert want.startswith("chunked merkle path failed for column out_off_10 @ "), want
    bad11 = PC.Case("out_off_10 sibling", "h", p, h11.root, 11, want, h11.shape)
    c = product.ProverContext(0)
    try:
        _check(product, c, [h11, bad11])            # the table is created at 3 + 7 * 11 = 80 labels
        assert c.verify_times()["jobs"] == 2 * _jobs(h11)
        assert _check(product, c, [h2]) == [(0, "")]  # large enough already
        _check(product, c, [big])                   # grows to 65536 labels; label id 65536 stays on the host
        assert c.verify_times()["jobs"] == _jobs(big) == _jobs(h2) + 9 * 9360
        assert _check(product, c, [h11, bad11, h2])[0] == (0, "")
    finally:
        c.close()


@pytest.mark.parametrize("fam", ["h", "a", "b", "c", "d", "e"])
def test_family_in_one_batch(product, ctx, cases, fam):
    mine = [c for c in cases if c.family == fam]
    got = _check(product, ctx, mine)
    assert ctx.verify_times()["slices"] == 1
    if fam != "e":
        assert (0, "") in got
    if fam == "d":  # the forged proofs' paths all hold: what rejects them is a check on the host side of the call
        rejected = {g[1].rstrip("0123456789") for g in got if g[0]}
        assert {"AIR composition non-zero at row ", "FRI fold mismatch at layer ", "final FRI value mismatch",
                "no FRI roots", "FRI layer count does not match domain_n"} <= rejected, rejected


def test_host_fallback_one_at_a_time(product, ctx, cases, oracle):
    plain = _jobs(PC.by_name(oracle, "h/n16_t2"))
    for c in (c for c in cases if c.family == "e"):
        _check(product, ctx, [c])
        t = ctx.verify_times()
        assert t["slices"] == 1
        assert t["jobs"] == _jobs(c) == plain + (9 * 9360 if "9362" in c.name else 0), c.name  # the host's jobs count too


def _mixed(cases, oracle):
    """Each host-fallback proof between an honest proof and one with a single
    failing device chain (a path_in sibling of a middle opening, a FRI path):
    a result word that lands one early or late names another column or layer."""
    tampered = [c for c in cases if c.family == "a" and c.name.startswith("n16_t2 ", 2) and
                ("path_in sibling" in c.name or "path_j sibling" in c.name)]
    assert len(tampered) >= 8 and all(c.want and "path failed" in c.want for c in tampered)
    honest = [PC.by_name(oracle, "h/n16_t2"), PC.by_name(oracle, "h/n2048_t1"), PC.by_name(oracle, "h/n16_t11")]
    out = []
    for i, c in enumerate(c for c in cases if c.family == "e"):
        out += [honest[i % 3], c, tampered[i % len(tampered)]]
    return out + [honest[0]]


def test_host_fallback_in_a_mixed_batch(product, ctx, cases, oracle):
    items = _mixed(cases, oracle)
    got = _check(product, ctx, items)
    t = ctx.verify_times()
    assert t["slices"] == 1 and t["jobs"] == sum(_jobs(c) for c in items)
    assert _check(product, ctx, items[::-1]) == got[::-1]


def test_host_fallback_in_slices_of_their_own(product, ctx, cases, oracle, monkeypatch):
    items = _mixed(cases, oracle)
    want = _check(product, ctx, items)
    monkeypatch.setenv("SEZKP_VERIFY_CHUNK_BYTES", "1000")  # smaller than any proof: each is a slice of its own
    assert _check(product, ctx, items) == want
    t = ctx.verify_times()
    assert t["slices"] == len(items) and t["jobs"] == sum(_jobs(c) for c in items)
    # a cap that keeps the honest proof and the fallback proof apart but lets small neighbours share a slice
    monkeypatch.setenv("SEZKP_VERIFY_CHUNK_BYTES", str(2 * len(items[0].proof) + 100))
    assert _check(product, ctx, items) == want
    assert 1 < ctx.verify_times()["slices"] < len(items)
