"""Host side of the AIR audit (no GPU): the AirAudit result type, the CLI's
usage errors and the null-argument checks of the two C entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG

NO_ROW = (1 << 64) - 1
FAMS = ("mv_domain", "head_range", "slack_range", "sym_range", "boundary")


def _audit(product, n, viol, rej, bitmaps=True):
    bits = lambda rows: np.packbits(np.isin(np.arange(n), rows), bitorder="little").tobytes()
    none = {"cells": 0, "rows": 0, "first_row": NO_ROW, "first_tape": 0, "first_value": 0}
    return product.AirAudit(n, 2, {f: dict(none) for f in FAMS}, len(viol), min(viol, default=NO_ROW), len(rej),
                            min(rej, default=NO_ROW), bits(viol) if bitmaps else None, bits(rej) if bitmaps else None)


def test_bitmap_decoding(product):
    # row i is bit i % 8 of byte i / 8; the bits from n on are padding
    a = _audit(product, 21, [0, 7, 8, 20], [8])
    assert a.violating_bits == bytes([0b10000001, 0b00000001, 0b00010000])
    assert a.violating_rows().tolist() == [0, 7, 8, 20] and a.rejectable_rows().tolist() == [8]
    assert not a.ok
    a.violating_bits = bytes([0x81, 0x01, 0xF0])  # padding bits set: still only rows below n
    assert a.violating_rows().tolist() == [0, 7, 8, 20]
    b = _audit(product, 3, [], [])
    assert b.ok and b.violating_rows().size == 0 and b.rejectable_rows().size == 0
    c = _audit(product, 3, [], [], bitmaps=False)
    assert c.violating_rows() is None and c.rejectable_rows() is None
    big = _audit(product, 1 << 12, [4095], [0, 4095])
    assert big.violating_rows().tolist() == [4095] and big.rejectable_rows().tolist() == [0, 4095]


def test_verify_reject_probability(product):
    assert _audit(product, 64, [], []).verify_reject_probability() == 0.0
    assert _audit(product, 4, [0, 1, 2, 3], [0, 1, 2, 3]).verify_reject_probability() == 1.0
    # 30 independent draws mod n: 1 - (1 - k / n)^30
    assert _audit(product, 2, [0], [0]).verify_reject_probability() == pytest.approx(1 - 0.5 ** 30, rel=1e-15)
    assert _audit(product, 1024, [5], [5]).verify_reject_probability() == pytest.approx(1 - (1023 / 1024) ** 30, rel=1e-12)
    p = _audit(product, 1 << 21, [9], [9]).verify_reject_probability()
    assert p == pytest.approx(30 / (1 << 21), rel=1e-4)  # one bad row in 2^21: about 30 / 2^21
    # violating rows that are not rejectable do not count
    assert _audit(product, 8, [1, 2], []).verify_reject_probability() == 0.0


def test_first_rejected_query(product):
    a = _audit(product, 64, [3, 9, 40], [9, 40])
    assert a.first_rejected_query([1, 2, 3]) is None  # row 3 violates, but no verifier sees it
    assert a.first_rejected_query([5, 40, 9]) == 40   # query order, not row order
    assert a.first_rejected_query([9, 9, 40]) == 9
    assert a.first_rejected_query([]) is None
    assert a.first_rejected_query(np.array([63, 9], np.uint64)) == 9
    with pytest.raises(product.SezkpError):
        _audit(product, 64, [9], [9], bitmaps=False).first_rejected_query([9])


def test_cli_audit_usage_errors():
    cli = os.path.join(PKG, "bin", "sezkp-cli")
    r = subprocess.run([cli, "audit"], capture_output=True, text=True)
    assert r.returncode == 2 and "--blocks" in r.stderr
    r = subprocess.run([cli, "audit", "--json"], capture_output=True, text=True)
    assert r.returncode == 2
    r = subprocess.run([cli, "audit", "--blocks"], capture_output=True, text=True)
    assert r.returncode == 2
    r = subprocess.run([cli, "audit", "--blocks", "/nonexistent/blocks.cbor"], capture_output=True, text=True)
    assert r.returncode == 1
    r = subprocess.run([cli], capture_output=True, text=True)
    assert r.returncode == 2 and "sezkp-cli audit --blocks B [--json]" in r.stderr


def test_null_arguments_are_invalid_without_a_device(product):
    from sezkp_amd._lib import AirAuditC, Buf
    lib = product.lib
    out, vb, rb = AirAuditC(), Buf(), Buf()
    err = C.create_string_buffer(256)
    assert lib.sezkp_ctx_air_audit(None, C.byref(out), None, None, err, 256) == -1
    assert b"null" in err.value
    assert lib.sezkp_ctx_air_audit(None, None, None, None, None, 0) == -1
    blocks = product.synthetic_blocks(8, 8, 2, 4)
    err = C.create_string_buffer(256)
    assert lib.sezkp_stark_v1_air_audit(None, C.byref(out), C.byref(vb), C.byref(rb), err, 256) == -1
    assert b"null" in err.value
    assert lib.sezkp_stark_v1_air_audit(C.byref(blocks.view()), None, None, None, err, 256) == -1
    assert not vb.data and vb.len == 0 and not rb.data
    assert C.sizeof(AirAuditC) == 48 + 5 * 40  # the layout of sezkp_air_audit
