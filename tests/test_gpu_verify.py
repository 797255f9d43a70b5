"""Batch verification on the GPU (sezkp_ctx_verify_batch, k_verify_chains)
against the host verifier (sezkp_stark_v1_verify): for every proof, honest,
tampered by design, re-serialised with odd shapes, truncated or with a random
bit flipped, the batch result's (code, message) equals the host's for the same
bytes, manifest root and tau. Proofs come from the C oracle on the CPU.

The T = 128 proof's path_to_chunk is empty (128 rows are one chunk), so the
path_to sibling cases use the 4096-row tau = 8 proof, whose openings carry two
siblings there.

`python tests/test_gpu_verify.py --dump-corpus DIR` (no GPU) writes the
tampered, re-serialised, truncated and bit-flipped proofs of this module and
the differential corpus of tests/proof_corpus.py to DIR, one file each, for
tools/verify_hostile.cpp.
"""
import ctypes as C
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN, PKG  # noqa: E402
from proof_corpus import _layout, _write_proof  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_DECODE, E_VERIFY = -1, -4, -5


# ------------------------------------------------------------------ proofs
def _still_128(product):
    T, tau = 128, 2
    z = np.zeros((T, tau), np.int8)
    return product.partition(np.zeros(T, np.int8), z, z.astype(np.uint8), z.astype(np.uint16), 32)


def _honest_cases(product):
    out = []
    for f in ("ref_blocks.cbor", "riscv_blocks.cbor"):
        out.append((f, product.BlockSoA.from_cbor(open(os.path.join(GOLDEN, f), "rb").read())))
    out.append(("synthetic_256", product.synthetic_blocks(256, 64, 2, 5)))
    out.append(("still_128", _still_128(product)))
    out.append(("tau8_4096", product.synthetic_blocks(4096, 512, 8, 42)))
    return out


_PROOFS = {}


def _proofs(product, oracle):
    """name -> (blocks, manifest root, proof bytes); proved once per session."""
    if not _PROOFS:
        for name, blocks in _honest_cases(product):
            root = blocks.manifest_root()
            _PROOFS[name] = (blocks, root, oracle.prove_v1(blocks, root))
    return _PROOFS


@pytest.fixture(scope="module")
def proofs(product, oracle):
    return _proofs(product, oracle)


@pytest.fixture(scope="module")
def ctx(product, gpu_ok):
    c = product.ProverContext(0)
    yield c
    c.close()


# ------------------------------------------------------------- the two arms
def _host(product, proof, root=None, tau=0):
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


def _gpu(ctx, items):
    """items: (proof, root or None, tau) -> [(code, message)] from one batch call."""
    res = ctx.verify_batch([p for p, _, _ in items], [r for _, r, _ in items], [t for _, _, t in items])
    for r in res:
        assert r.ok == (r.code == 0)
    return [(r.code, r.message) for r in res]


def _agree(product, ctx, items):
    got = _gpu(ctx, items)
    want = [_host(product, p, r, t) for p, r, t in items]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    return want


# ------------------------------------------------------------------ layout
def _flip(proof, at, bit=0):
    b = bytearray(proof)
    b[at] ^= 1 << bit
    return bytes(b)


def _designed(proofs):
    """(name, tampered proof, root passed or None, expected check in the host message)."""
    _, root, p128 = proofs["still_128"]
    _, _, p8 = proofs["tau8_4096"]
    L, L8 = _layout(p128), _layout(p8)
    rows, rows8 = L["rows"], L8["rows"]
    first, mid, last = rows[0]["opens"][0], rows[14]["opens"][9], rows[29]["opens"][-1]
    out = []
    chunked = "chunked merkle path failed"
    for nm, o in (("first", first), ("middle", mid), ("last", last)):
        out.append((f"path_in sibling, {nm} opening", _flip(p128, o["path_in"] + 32 * (o["n_in"] // 2) + 5), None, chunked))
    for nm, o in (("first", rows8[0]["opens"][0]), ("middle", rows8[14]["opens"][40]), ("last", rows8[29]["opens"][-1])):
        assert o["n_to"] == 2
        out.append((f"path_to sibling, {nm} opening", _flip(p8, o["path_to"] + 32 * (o["n_to"] - 1) + 31, 7), None, chunked))
    fq = L["fq"]
    k = L["nroots"] - 1
    out.append(("first FRI path", _flip(p128, fq[0]["pairs"][0]["path_i"]), None, "FRI Merkle path failed at layer 0"))
    out.append(("last FRI path", _flip(p128, fq[29]["pairs"][k - 1]["path_j"] + 3), None,
                f"FRI Merkle path failed at layer {k - 1}"))
    out.append(("middle FRI layer", _flip(p128, fq[11]["pairs"][k // 2]["path_j"] + 32 + 1, 4), None,
                f"FRI Merkle path failed at layer {k // 2}"))
    out.append(("opened value", _flip(p128, mid["value"]), None, chunked))
    out.append(("chunk_root", _flip(p128, first["chunk_root"] + 7), None, chunked))
    # an index bit matters where the two subtrees it picks between differ: the still trace's columns are
    # constant, and with no sibling above the chunk root the chunk index picks no side: the 4096-row proof
    out.append(("index_in_chunk", _flip(p8, rows8[9]["opens"][4]["index_in_chunk"], 3), None, chunked))
    out.append(("chunk_index", _flip(p8, rows8[3]["opens"][5]["chunk_index"]), None, chunked))
    out.append(("query row", _flip(p128, rows[0]["row"]), None, "AIR query row mismatch at position 0"))
    out.append(("FRI root", _flip(p128, L["roots"] + 32 * 3), None, "AIR query row mismatch"))
    out.append(("FRI position", _flip(p128, fq[2]["pos"] + 8), None, "FRI index propagation failed at layer 0"))
    # a layer's first value is checked against the fold of the layer before, its second only by its path
    out.append(("FRI pair value (vj)", _flip(p128, fq[0]["pairs"][1]["vj"]), None, "FRI Merkle path failed at layer 1"))
    out.append(("FRI pair value (vi)", _flip(p128, fq[0]["pairs"][1]["vi"]), None, "FRI fold mismatch at layer 0"))
    out.append(("final value", _flip(p128, L["final"]), None, "final FRI value mismatch with last root"))
    out.append(("manifest root, root passed", _flip(p128, L["mroot"] + 31), root, "manifest root mismatch"))
    out.append(("manifest root, no root passed", _flip(p128, L["mroot"] + 31), None, "AIR query row mismatch"))
    out.append(("column label byte", _flip(p128, L["cols"][0]["label"]), None, "missing col root for input_mv"))
    out.append(("length prefix", _flip(p128, first["n_in_at"] + 6), None, "bad length prefix"))
    out.append(("query count", _flip(p128, L["nq_at"]), None, "bad length prefix"))  # a 31st row is read from the FRI roots
    return out


def _reserialised(proofs):
    """(name, bytes, expected check in the host message)."""
    import sezkp_oracle_py as V
    _, _, p128 = proofs["still_128"]
    assert _write_proof(V.parse_proof_v1(p128)) == p128
    out = []
    pf = V.parse_proof_v1(p128)
    pf["queries"][4]["per_tape"][1]["head"]["path_in_chunk"] = []
    out.append(("empty path_in", _write_proof(pf), "chunked merkle path failed for column head_1"))
    pf = V.parse_proof_v1(p128)
    vi, pi, vj, pj = pf["fri_queries"][7]["pairs"][2]
    pf["fri_queries"][7]["pairs"][2] = (vi, pi + [bytes([i]) * 32 for i in range(70 - len(pi))], vj, pj)
    out.append(("70 FRI siblings", _write_proof(pf), "FRI Merkle path failed at layer 2"))
    pf = V.parse_proof_v1(p128)
    for q in pf["queries"]:
        q["per_tape"] = []
    out.append(("0 tapes per row", _write_proof(pf), ""))  # the three row columns hold and the AIR sum is empty
    pf = V.parse_proof_v1(p128)
    pf["fri_roots"] = pf["fri_roots"][:-1]
    out.append(("one layer fewer", _write_proof(pf), "AIR query row mismatch"))
    pf = V.parse_proof_v1(p128)
    pf["fri_roots"] = pf["fri_roots"] + [pf["fri_roots"][-1]]
    out.append(("one layer more", _write_proof(pf), "AIR query row mismatch"))
    for n in (0, 1, 39, 40, len(p128) - 1):  # at 39 and 40 bytes the column count exceeds what is left
        out.append((f"truncated to {n}", p128[:n], "bad length prefix" if n in (39, 40) else "truncated proof bytes"))
    return out


def _random_flips(p128):
    rng = random.Random(20240607)
    return [_flip(p128, rng.randrange(len(p128)), rng.randrange(8)) for _ in range(200)]


# ------------------------------------------------------------------- tests
def test_honest_proofs(product, ctx, proofs):
    items = [(p, root, blocks.tau) for blocks, root, p in proofs.values()]
    want = _agree(product, ctx, items)
    assert any(w[0] == 0 for w in want)
    assert any(w[0] == E_VERIFY and "AIR composition non-zero" in w[1] for w in want), want
    # the tau check against a wrong tau, and none at all
    _, root, p = proofs["still_128"]
    w = _agree(product, ctx, [(p, root, 3), (p, root, 0), (p, None, 2)])
    assert "tau mismatch vs. block windows" in w[0][1] and w[1] == (0, "") and w[2] == (0, "")


def test_designed_tampering(product, ctx, proofs):
    cases = _designed(proofs)
    for name, p, root, kind in cases:
        w = _host(product, p, root)
        assert w[0] != 0 and kind in w[1], (name, w)  # the offset hit the field it names
    _agree(product, ctx, [(p, root, 0) for _, p, root, _ in cases])
    for name, p, root, _ in cases:  # and one at a time
        assert _gpu(ctx, [(p, root, 0)]) == [_host(product, p, root)], name


def test_reserialised_proofs(product, ctx, proofs):
    cases = _reserialised(proofs)
    for name, p, kind in cases:
        w = _host(product, p)
        assert (w == (0, "")) if kind == "" else (w[0] != 0 and kind in w[1]), (name, w)
    assert _host(product, b"")[0] == E_DECODE
    _agree(product, ctx, [(p, None, 0) for _, p, _ in cases])
    # an empty proof given as a null pointer of length 0
    from sezkp_amd._lib import ProofRef, VerifyResultC
    refs, out = (ProofRef * 1)(), (VerifyResultC * 1)()
    err = C.create_string_buffer(256)
    assert product.lib.sezkp_ctx_verify_batch(ctx._h, refs, 1, out, err, 256) == 0
    assert (out[0].code, out[0].msg.decode()) == _host(product, b"")


def test_random_bit_flips(product, ctx, proofs):
    _, root, p128 = proofs["still_128"]
    flips = _random_flips(p128)
    want = _agree(product, ctx, [(p, None, 2) for p in flips])  # all 200 in one call
    assert len(want) == 200 and sum(w[0] != 0 for w in want) > 100


def _mixed(proofs):
    items = []
    designed = _designed(proofs)
    for i, (blocks, root, p) in enumerate(proofs.values()):
        items.append((p, root, blocks.tau))
        name, tp, troot, _ = designed[(5 * i) % len(designed)]
        items.append((tp, troot, 0))
    items.append((b"", None, 0))
    items.append((proofs["still_128"][2][:1000], None, 0))
    return items


def test_mixed_batch_order_and_alone(product, ctx, proofs):
    items = _mixed(proofs)
    want = _agree(product, ctx, items)
    assert _gpu(ctx, items[::-1]) == want[::-1]
    for it, w in zip(items, want):
        assert _gpu(ctx, [it]) == [w]
    assert ctx.verify_batch([]) == []
    assert product.StarkV1.verify_batch([]) == []
    assert [(r.code, r.message) for r in product.StarkV1.verify_batch([items[0][0], items[1][0]])] == \
        [_host(product, items[0][0]), _host(product, items[1][0])]


def test_batch_of_64_and_slices(product, ctx, proofs, monkeypatch):
    _, root, p128 = proofs["still_128"]
    bad = _designed(proofs)[7][1]
    batch = [(bad if i in (0, 31, 63) else p128, root, 2) for i in range(64)]
    want = [_host(product, bad, root, 2) if i in (0, 31, 63) else (0, "") for i in range(64)]
    assert _host(product, p128, root, 2) == (0, "") and want[0][0] == E_VERIFY
    assert _gpu(ctx, batch) == want
    t = ctx.verify_times()
    assert t["slices"] == 1 and t["jobs"] > 9e4  # about 10^5 chains, many workgroups
    # the same batch in slices of at most 3 proofs, then with every proof larger than the cap
    monkeypatch.setenv("SEZKP_VERIFY_CHUNK_BYTES", str(3 * len(p128) + 100))
    assert _gpu(ctx, batch) == want
    assert ctx.verify_times()["slices"] >= 22
    mixed = _mixed(proofs)
    assert _gpu(ctx, mixed) == [_host(product, *it) for it in mixed]
    assert ctx.verify_times()["slices"] >= 3
    monkeypatch.setenv("SEZKP_VERIFY_CHUNK_BYTES", "1000")
    assert _gpu(ctx, batch[:5]) == want[:5]
    assert ctx.verify_times()["slices"] == 5


def test_context_with_resident_trace(product, gpu_ok, proofs):
    blocks, root, want_proof = proofs["tau8_4096"]
    c = product.ProverContext(0)
    try:
        c.upload(blocks)
        a1 = c.prove(root)
        r = c.verify_batch([a1], [root], [blocks.tau])[0]
        a2 = c.prove(root)
        assert a1.proof_bytes == a2.proof_bytes == want_proof
        assert (r.code, r.message) == _host(product, a1.proof_bytes, root, blocks.tau)
        c.verify(a1, blocks, root)  # accepted: returns None as StarkV1.verify does
        product.StarkV1.verify(a1, blocks, root)
        # a proof in flight: refused, and the proof still completes
        from sezkp_amd._lib import ProofRef, VerifyResultC
        refs, out = (ProofRef * 1)(), (VerifyResultC * 1)()
        buf = C.create_string_buffer(want_proof, len(want_proof))
        refs[0].bytes, refs[0].len = C.addressof(buf), len(want_proof)
        err = C.create_string_buffer(256)
        c.prove_async(root)
        rc = product.lib.sezkp_ctx_verify_batch(c._h, refs, 1, out, err, 256)
        got = bytes(c.wait_view())
        assert rc == E_INVALID and b"in flight" in err.value
        assert got == want_proof
        assert product.lib.sezkp_ctx_verify_batch(c._h, refs, 1, out, err, 256) == 0 and out[0].code == 0
    finally:
        c.close()


def test_sharded_context_is_refused(product, gpu_ok, proofs):
    solo = product.ShardedProverContext(0, 2, device=0, comm="solo")
    try:
        with pytest.raises(product.SezkpError, match="sharded") as e:
            solo.verify_batch([proofs["still_128"][2]])
        assert e.value.code == E_INVALID
    finally:
        solo.close()


def test_context_verify_raises_as_starkv1(product, ctx, proofs):
    def verdict(f, *a):
        try:
            return f(*a)
        except product.SezkpError as e:
            return (e.code, str(e))
    blocks, root, p = proofs["still_128"]
    rblocks, rroot, rp = proofs["ref_blocks.cbor"]
    bad = _designed(proofs)[0][1]
    art = lambda backend, r, b: product.ProofArtifact(backend, r, b, {})
    for a, b, r in ((art("stark", root, p), blocks, root), (art("stark", rroot, rp), rblocks, rroot),
                    (art("stark", root, bad), blocks, root), (art("groth", root, p), blocks, root),
                    (art("stark", rroot, p), blocks, root), (art("stark", root, p), proofs["tau8_4096"][0], root),
                    (art("stark", root, p[:77]), blocks, root)):
        assert verdict(ctx.verify, a, b, r) == verdict(product.StarkV1.verify, a, b, r)
    assert verdict(ctx.verify, art("stark", root, p), blocks, root) is None
    assert verdict(ctx.verify, art("stark", rroot, rp), rblocks, rroot)[0] == E_VERIFY


def test_two_contexts_from_two_threads(product, gpu_ok, proofs):
    items = _mixed(proofs)
    want = [_host(product, *it) for it in items]
    ctxs = [product.ProverContext(0), product.ProverContext(0)]  # neither has an upload
    got, errs = [None, None], []

    def run(k):
        try:
            for _ in range(3):
                got[k] = _gpu(ctxs[k], items if k == 0 else items[::-1])
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for c in ctxs:
        c.close()
    assert not errs, errs
    assert got[0] == want and got[1] == want[::-1]


def test_cli_verify_gpu_flag(product, gpu_ok, proofs, tmp_path):
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    for name in ("still_128", "synthetic_256"):  # accepted, rejected by the AIR sum
        blocks, root, p = proofs[name]
        bf, mf, pf = (str(tmp_path / f"{name}.{x}.cbor") for x in ("blocks", "manifest", "proof"))
        open(bf, "wb").write(blocks.to_cbor())
        assert subprocess.run([cli, "commit", "--blocks", bf, "--out", mf], capture_output=True).returncode == 0
        open(pf, "wb").write(product.ProofArtifact("stark", root, p, {"proto": "stark-v1"}).to_cbor())
        base = [cli, "verify", "--backend", "stark", "--blocks", bf, "--manifest", mf, "--proof", pf]
        a = subprocess.run(base, capture_output=True, text=True)
        b = subprocess.run(base + ["--gpu"], capture_output=True, text=True)
        assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b.stdout, b.stderr)
        assert a.returncode == (0 if name == "still_128" else 1), (a.stdout, a.stderr)


# ------------------------------------------------------------ corpus dump
def _dump_corpus(out_dir):
    import oracle_ctypes
    import sezkp_amd
    oracle_ctypes.build()
    proofs = _proofs(sezkp_amd, oracle_ctypes)
    os.makedirs(out_dir, exist_ok=True)
    files = [(f"honest_{n}", p) for n, (_, _, p) in proofs.items()]
    files += [(f"designed_{i:02d}", p) for i, (_, p, _, _) in enumerate(_designed(proofs))]
    files += [(f"reserialised_{i:02d}", p) for i, (_, p, _) in enumerate(_reserialised(proofs))]
    files += [(f"flip_{i:03d}", p) for i, p in enumerate(_random_flips(proofs["still_128"][2]))]
    import proof_corpus  # the differential corpus (test_verifier_differential.py), family and number in the name
    files += [(f"diff_{c.family}_{i:03d}", c.proof) for i, c in enumerate(proof_corpus.corpus(oracle_ctypes))]
    for name, p in files:
        with open(os.path.join(out_dir, name + ".bin"), "wb") as f:
            f.write(p)
    print(f"wrote {len(files)} proofs to {out_dir}")


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--dump-corpus":
        sys.exit("usage: test_gpu_verify.py --dump-corpus DIR")
    _dump_corpus(sys.argv[2])
