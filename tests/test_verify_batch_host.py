"""Host side of the batch verifier (no GPU): the header declares the new
symbols and the library exports them, the struct layouts the Python mirror
binds, and the argument checks that answer before any device is touched."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ("sezkp_ctx_verify_batch", "sezkp_stark_v1_verify_batch", "sezkp_ctx_verify_times")


def test_header_declares_and_library_exports(product):
    hdr = open(os.path.join(ROOT, "include", "sezkp_stark.h")).read()
    declared = set(re.findall(r"\b(sezkp_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(product.LIB_PATH)
    for s in NEW:
        assert s in declared and hasattr(lib, s) and s in product._lib.EXPORTS, s
    assert "typedef struct sezkp_proof_ref" in hdr and "typedef struct sezkp_verify_result" in hdr
    assert lib.sezkp_abi_version() == 4  # symbols added, nothing changed
    from sezkp_amd._lib import VERIFY_TIMES, ProofRef, VerifyResultC
    assert C.sizeof(ProofRef) == 32 and C.sizeof(VerifyResultC) == 256
    assert ProofRef.len.offset == 8 and ProofRef.manifest_root.offset == 16 and ProofRef.tau.offset == 24
    assert VerifyResultC.msg.offset == 8 and VerifyResultC.msg.size == 248
    n_times = int(re.search(r"SEZKP_VT_PARSE,(.*?)SEZKP_VERIFY_TIMES", hdr, re.S).group(1).count(",")) + 1
    assert n_times == len(VERIFY_TIMES)
    assert {"VerifyResult"} <= set(product.__all__)
    for m in ("verify_batch", "verify", "verify_times"):
        assert hasattr(product.ProverContext, m)
    assert hasattr(product.StarkV1, "verify_batch")


def test_null_arguments_are_invalid_without_a_device(product):
    from sezkp_amd._lib import ProofRef, VerifyResultC
    lib = product.lib
    refs, out = (ProofRef * 2)(), (VerifyResultC * 2)()
    err = C.create_string_buffer(256)
    assert lib.sezkp_stark_v1_verify_batch(None, 2, out, err, 256) == -1   # null proofs, n > 0
    assert b"null" in err.value
    err = C.create_string_buffer(256)
    assert lib.sezkp_stark_v1_verify_batch(refs, 2, None, err, 256) == -1  # null out, n > 0
    assert b"null" in err.value
    assert lib.sezkp_stark_v1_verify_batch(None, 1, None, None, 0) == -1
    # null bytes with a length
    refs[1].len = 5
    err = C.create_string_buffer(256)
    assert lib.sezkp_stark_v1_verify_batch(refs, 2, out, err, 256) == -1
    assert b"proof 1" in err.value
    # the context entry point: a null context, and the same checks
    assert lib.sezkp_ctx_verify_batch(None, refs, 0, out, err, 256) == -1
    assert lib.sezkp_ctx_verify_batch(None, None, 2, out, err, 256) == -1
    assert lib.sezkp_ctx_verify_times(None, None, 0) == 0


def test_stateless_empty_batch_is_ok(product):
    from sezkp_amd._lib import ProofRef, VerifyResultC
    lib = product.lib
    err = C.create_string_buffer(256)
    assert lib.sezkp_stark_v1_verify_batch(None, 0, None, err, 256) == 0
    assert lib.sezkp_stark_v1_verify_batch((ProofRef * 1)(), 0, (VerifyResultC * 1)(), err, 256) == 0
    assert product.StarkV1.verify_batch([]) == []


def test_python_argument_checks(product):
    import pytest
    with pytest.raises(product.SezkpError):
        product.StarkV1.verify_batch([b"x"], manifest_roots=[b"short"])
    with pytest.raises(product.SezkpError):
        product.StarkV1.verify_batch([b"x"], taus=[1, 2])
    r = product.VerifyResult(False, -5, "manifest root mismatch")
    assert (r.ok, r.code, r.message) == (False, -5, "manifest root mismatch")
