"""C ABI + host-side product pieces, CPU only (no compute calls on a GPU).

* the library loads and exports every symbol include/sezkp_stark.h declares;
* CBOR Vec<BlockSummary> decode, manifest commitment, host BLAKE3 and the
  transcript-level pieces agree with the oracle;
* the host verifier (v1/verify.rs restatement) accepts oracle proofs of
  AIR-valid traces and rejects tampering; malformed input never crashes;
* `sezkp-cli commit` reproduces the reference's committed manifest.cbor bytes.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT


def test_library_exports_every_declared_symbol(product):
    hdr = open(os.path.join(ROOT, "include", "sezkp_stark.h")).read()
    declared = set(re.findall(r"\b(sezkp_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(product.LIB_PATH)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert declared == set(product._lib.EXPORTS)
    assert lib.sezkp_abi_version() == 4


def test_cbor_decode_matches_oracle_decode(product, oracle):
    import cbor_min
    for f in ("ref_blocks.cbor", "riscv_blocks.cbor"):
        raw = open(os.path.join(GOLDEN, f), "rb").read()
        a = product.BlockSoA.from_cbor(raw)
        b = oracle.Blocks(cbor_min.loads(raw))
        for name, _ in product._lib.VIEW_FIELDS:
            np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
        assert a.manifest_root() == oracle.manifest_root(b)


def test_cbor_decode_errors_are_reported(product):
    raw = open(os.path.join(GOLDEN, "ref_blocks.cbor"), "rb").read()
    for bad in (raw[:100], raw[:-1], b"\xa0", b"", raw + b"\x00"):
        with pytest.raises(product.SezkpError):
            product.BlockSoA.from_cbor(bad)


def test_host_blake3_matches_oracle(product, oracle):
    for L in (0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3000, 70000):
        d = bytes((i * 13 + 5) % 256 for i in range(L))
        out = C.create_string_buffer(200)
        product.lib.sezkp_blake3(d, len(d), out, 200)
        assert out.raw == oracle.blake3(d, 200), L


def test_synthetic_manifest_root_matches_oracle(product, oracle):
    b = product.synthetic_blocks(4096, 512, 8, 42)
    assert b.n_rows == 4096 and b.n_blocks == 8
    assert b.manifest_root() == oracle.manifest_root(b)


def _valid_trace(product, T=512, tau=2, b=64, seed=1):
    rng = np.random.default_rng(seed)
    mv = rng.integers(0, 2, (T, tau), dtype=np.int8)  # heads stay >= 0: every AIR term vanishes
    hw = (rng.random((T, tau)) < 0.5).astype(np.uint8)
    ws = (rng.integers(0, 16, (T, tau)) * hw).astype(np.uint16)
    return product.partition(rng.integers(-1, 2, T, dtype=np.int8), mv, hw, ws, b)


def test_host_verifier_accepts_oracle_proof_and_rejects_tampering(product, oracle):
    blocks = _valid_trace(product)
    root = blocks.manifest_root()
    proof = oracle.prove_v1(blocks, root)
    art = product.ProofArtifact("stark", root, proof, {})
    product.StarkV1.verify(art, blocks, root)
    # bound fields: tau, a column root, the FRI final value, the manifest root
    # (Opening.index is NOT bound by the reference verifier either: merkle.rs:243-281
    # only uses chunk_index / index_in_chunk — a faithful restatement accepts it)
    for pos in (8, 45, len(proof) - 40, len(proof) - 33, len(proof) - 1):
        bad = bytearray(proof)
        bad[pos] ^= 0x40
        with pytest.raises(product.SezkpError):
            product.StarkV1.verify(product.ProofArtifact("stark", root, bytes(bad), {}), blocks, root)
    with pytest.raises(product.SezkpError):
        product.StarkV1.verify(product.ProofArtifact("stark", root, proof[:-7], {}), blocks, root)
    # domain_n no longer matching the FRI layer count (untrusted sizes never size a shift)
    bad = bytearray(proof)
    bad[0:8] = (int.from_bytes(proof[0:8], "little") * 2).to_bytes(8, "little")
    with pytest.raises(product.SezkpError):
        product.StarkV1.verify(product.ProofArtifact("stark", root, bytes(bad), {}), blocks, root)
    with pytest.raises(product.SezkpError):
        product.StarkV1.verify(art, blocks, bytes(32))
    with pytest.raises(product.SezkpError):
        product.StarkV1.verify(product.ProofArtifact("fold", root, proof, {}), blocks, root)


def test_host_verifier_on_reference_fixture_reports_air_failure(product, oracle):
    """The generator's traces can violate the boundary terms (SURVEY §3C note):
    the reference verifier rejects them with "AIR composition non-zero"; so do we."""
    raw = open(os.path.join(GOLDEN, "ref_blocks.cbor"), "rb").read()
    blocks = product.BlockSoA.from_cbor(raw)
    root = blocks.manifest_root()
    proof = oracle.prove_v1(blocks, root)
    try:
        product.StarkV1.verify(product.ProofArtifact("stark", root, proof, {}), blocks, root)
    except product.SezkpError as e:
        assert "AIR composition non-zero" in str(e)


def test_artifact_cbor_layout(product, oracle):
    import cbor_min
    art = product.ProofArtifact("stark", bytes(range(32)), bytes(range(40)) * 3,
                                {"proto": "stark-v1", "domain_n": 512, "tau": 2, "mode": "streaming"})
    assert art.to_cbor() == cbor_min.proof_artifact_cbor("stark", art.manifest_root, art.proof_bytes, art.meta)


def test_cli_commit_reproduces_reference_manifest(tmp_path):
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    for b, m in (("ref_blocks.cbor", "ref_manifest.cbor"), ("riscv_blocks.cbor", "riscv_manifest.cbor")):
        out = tmp_path / "m.cbor"
        subprocess.run([cli, "commit", "--blocks", os.path.join(GOLDEN, b), "--out", str(out)], check=True,
                       capture_output=True)
        assert out.read_bytes() == open(os.path.join(GOLDEN, m), "rb").read()


def test_cli_rejects_jsonl_for_stark_and_mismatched_manifest(tmp_path):
    import sezkp_amd
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    jl = tmp_path / "x.jsonl"  # a real JSONL file of the reference's blocks (8 blocks: Frontier == batch root)
    jl.write_bytes(sezkp_amd.BlockSoA.from_cbor(open(os.path.join(GOLDEN, "ref_blocks.cbor"), "rb").read()).to_jsonl())
    r = subprocess.run([cli, "prove", "--backend", "stark", "--blocks", str(jl), "--manifest",
                        os.path.join(GOLDEN, "ref_manifest.cbor"), "--out", str(tmp_path / "p.cbor")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "unsupported blocks extension: jsonl" in r.stderr, r.stderr
    r = subprocess.run([cli, "prove", "--backend", "stark", "--blocks", os.path.join(GOLDEN, "riscv_blocks.cbor"),
                        "--manifest", os.path.join(GOLDEN, "ref_manifest.cbor"), "--out", str(tmp_path / "p.cbor")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "root mismatch" in r.stderr


def test_cli_export_jsonl_round_trips_reference_blocks(tmp_path, product):
    """`sezkp-cli export-jsonl` (main.rs:400-424): the reference's blocks.cbor
    -> JSONL, one serde_json object per line; the lines decode back to blocks
    whose CBOR encoding is byte-identical to the reference's file, and a JSONL
    input exports to itself. The JSON text itself is parity unpinned (the
    reference commits no JSONL fixture): it is the layout of `simulate`'s
    .jsonl output, the encoder of write_block_summaries_jsonl."""
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    for b, m in (("ref_blocks.cbor", "ref_manifest.cbor"), ("riscv_blocks.cbor", "riscv_manifest.cbor")):
        src = os.path.join(GOLDEN, b)
        out = tmp_path / "sub" / "dir" / "blocks.jsonl"  # the parent directories are created
        r = subprocess.run([cli, "export-jsonl", "--input", src, "--output", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        data = out.read_bytes()
        back = product.BlockSoA.from_jsonl(data)
        ref = open(src, "rb").read()
        assert back.to_cbor() == ref
        assert r.stdout.startswith(f"Exported {back.n_blocks} blocks")
        assert data.count(b"\n") == back.n_blocks and data.endswith(b"}\n")
        again = tmp_path / "again.ndjson"
        subprocess.run([cli, "export-jsonl", "--input", str(out), "--output", str(again)], check=True,
                       capture_output=True)
        assert again.read_bytes() == data
        # the exported file passes verify-commit against the reference manifest
        # when its Frontier root equals the batch root (power-of-two leaf count)
        if back.n_blocks & (back.n_blocks - 1) == 0:
            r = subprocess.run([cli, "verify-commit", "--blocks", str(out), "--manifest", os.path.join(GOLDEN, m)],
                               capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.startswith("OK:"), r.stderr
    r = subprocess.run([cli, "export-jsonl", "--input", str(tmp_path / "x.txt"), "--output", str(tmp_path / "y.jsonl")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "unsupported blocks extension: txt" in r.stderr


def test_cli_verify_commit(tmp_path):
    """`sezkp-cli verify-commit` (main.rs:377-398): OK on the reference's own
    blocks/manifest pair, a root mismatch on the other fixture's manifest."""
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    r = subprocess.run([cli, "verify-commit", "--blocks", os.path.join(GOLDEN, "ref_blocks.cbor"), "--manifest",
                        os.path.join(GOLDEN, "ref_manifest.cbor")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK:"), r.stderr
    r = subprocess.run([cli, "verify-commit", "--blocks", os.path.join(GOLDEN, "riscv_blocks.cbor"), "--manifest",
                        os.path.join(GOLDEN, "ref_manifest.cbor")], capture_output=True, text=True)
    assert r.returncode != 0 and "root mismatch" in r.stderr


def test_kernel_abi_rejects_null_pointers_before_any_launch(product):
    """Every kernel-level entry point checks its device pointers before it
    touches HIP, so these return SEZKP_E_INVALID on a machine without a GPU."""
    lib, E = product.lib, product._lib.SEZKP_E_INVALID
    buf = C.create_string_buffer(64)
    assert lib.sezkp_fri_fold(None, 4, 3, None, None) == E
    assert lib.sezkp_blake3_leaves_u64(None, 8, None, None) == E
    assert lib.sezkp_blake3_leaves_labeled(None, 8, b"x", 1, None, None) == E
    assert lib.sezkp_merkle_build(None, 8, None, None) == E
    assert lib.sezkp_merkle_paths(None, 8, None, 1, None, None) == E
    assert lib.sezkp_fri_fold_commit(None, 4, 3, None, buf, None) == E
    assert lib.sezkp_merkle_root_u64(None, 4, buf, None) == E
    out = C.c_void_p()
    assert lib.sezkp_blocks_decode_cbor(None, 10, C.byref(out), buf, 64) == E
    assert lib.sezkp_blocks_decode_jsonl(b"{}", 2, None, buf, 64) == E


def test_dict_plans_rejects_a_null_context(product):
    """sezkp_ctx_dict_plans without a context is SEZKP_E_INVALID whatever the
    other arguments (the null-output and negative-max cases need a context:
    tests/test_gpu_dict_forms.py)."""
    lib, E = product.lib, product._lib.SEZKP_E_INVALID
    buf = (product._lib.DictPlanInfo * 4)()
    assert lib.sezkp_ctx_dict_plans(None, buf, 4) == E
    assert lib.sezkp_ctx_dict_plans(None, None, 0) == E
    assert lib.sezkp_ctx_dict_plans(None, buf, -1) == E
    assert C.sizeof(product._lib.DictPlanInfo) == 40  # sezkp_dict_plan_info: 8 x 32 bits + int64


def test_block_shapes_checked_before_the_c_abi(product):
    """partial views (meta_only, concat_meta, with_steps)
    and wrong row counts must be refused on the host, since sezkp_block_view
    carries no lengths and the C side would read past the numpy buffers."""
    b = product.synthetic_blocks(4096, 512, 8, 42)
    b.check_shape()
    n = int(b.step_start[-1])
    meta = b.meta_only()
    with pytest.raises(product.SezkpError, match="input_mv"):
        meta.check_shape()
    meta.check_shape(0)  # metadata-only view: zero rows is consistent
    with pytest.raises(product.SezkpError):
        b.check_shape(n - 8)  # upload_rows with more rows in the arrays than nrows
    sl = product.BlockSoA(b.tau, **{f: getattr(b, f) for f, _ in product._lib.VIEW_FIELDS})
    sl.mv = sl.mv[: 8 * (n - 1)]
    with pytest.raises(product.SezkpError, match="mv"):
        sl.check_shape()
    bad = product.BlockSoA(b.tau, **{f: getattr(b, f) for f, _ in product._lib.VIEW_FIELDS})
    bad.off_in = bad.off_in[:-1]
    with pytest.raises(product.SezkpError, match="off_in"):
        bad.check_shape()
    # the prove entry point refuses it too (no device needed: it fails first)
    with pytest.raises(product.SezkpError):
        product.StarkV1.prove(meta, b.manifest_root())


def test_block_step_start_checked_on_host(product):
    b = product.synthetic_blocks(64, 32, 2)
    b.step_start[:] += 32
    with pytest.raises(product.SezkpError, match="step_start"):
        b.check_shape()


def test_zero_step_blocks_host_side(product, oracle):
    """Blocks of zero steps (step_hi = step_lo - 1) on the host side of the
    boundary: the BlockSoA helper gives the oracle's blocks, the manifest
    commits to every block (leaf_hash has steps.len() = 0; product root ==
    oracle root), the CBOR codec round-trips them."""
    from conftest import insert_zero_step_blocks
    b = product.synthetic_blocks(1 << 10, 100, 3, 5)
    zb = insert_zero_step_blocks(b, [0, 4, 4, b.n_blocks])
    assert zb.n_blocks == b.n_blocks + 4 and zb.n_rows == b.n_rows
    zb.check_shape()
    assert zb.manifest_root() == oracle.manifest_root(zb) != b.manifest_root()
    rt = product.BlockSoA.from_cbor(zb.to_cbor())
    assert rt.manifest_root() == zb.manifest_root()
    assert (rt.step_hi == zb.step_hi).all() and (rt.step_start == zb.step_start).all()
    jl = product.BlockSoA.from_jsonl(zb.to_jsonl())
    assert (jl.step_hi == zb.step_hi).all() and (jl.step_start == zb.step_start).all()
    assert jl.manifest_frontier_root() == zb.manifest_frontier_root()
