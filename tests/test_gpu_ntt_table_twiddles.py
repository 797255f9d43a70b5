"""GPU parity of k_ntt4's table twiddles (SEZKP_NTT_TW_TABLE, ntt_pass.hip;
the switch is read by the runner in ntt_run.cpp).

A wide pass (sL >= 4) of m stages whose m + sL <= 16 takes its pass twiddle
w_{2^(m + sL)}^(low j) as one load per element from a table of the pass's
geometry (copies of `hi` entries, row j, column low) instead of the two
tw_pow and the multiplication chain, and every k_ntt4 pass fills its W[] from
`hi` without the product. `SEZKP_NTT_TW_TABLE=0` (read per launch) restores tw_pow and
the chains. Both arms must give the oracle's values, bit for bit.

The smallest sizes with such a pass on the register kernel (m in 6..8, 16
columns), from plan_passes / plan_passes_x16 (ntt_plan.h; 2^10..2^12 are one X16 tile, no
wide pass; below 2^10 the passes have m < 6 and run k_ntt_pass):

  DIF, forward and inverse (sezkp_gl_ntt without scratch: ntt_dif + bit
    reversal): 2^13 = 7 + 6, first pass m = 7, sL = 6; next 2^14 = 7 + 7, first
    pass m = 7, sL = 7.
  DIT inverse (one-rank sezkp_ctx_dist_ntt, inverse: bit reversal + ntt_dit):
    2^13 = 7 + 6, second pass m = 6, sL = 7; next 2^14, second pass m = 7, sL = 7.
  DIT forward: the LDE's replicated load, N = 2^13 (n = 2^10): second pass
    m = 6, sL = 7, then the DEEP kernel; next N = 2^14 (n = 2^11): second pass
    m = 7, sL = 7 with DEEP fused. A plain forward DIT exists from 2^21 on
    (the natural-order transform with scratch, 7 + 7 + 7: second pass m = 7,
    sL = 7; its inverse is a DIT too), so 2^21 and 2^22 (8 + 7 + 7: m = 7,
    sL = 8) run as well.
  LDE + DEEP at n = 2^13 (N = 2^16 = 8 + 8: the second pass is m = 8, sL = 8,
    the headline geometry, with DEEP fused) and n = 2^14 (N = 2^17 = 6 + 6 + 5:
    second pass m = 6, sL = 6).
"""
import os

import numpy as np
import pytest

from test_gpu_parity import EDGE, P, _dev, _host

pytestmark = pytest.mark.gpu

ARMS = ["table", "chain"]
_ref = {}


@pytest.fixture(autouse=True)
def _arm_env(monkeypatch):
    monkeypatch.delenv("SEZKP_NTT_TW_TABLE", raising=False)


def _set_arm(monkeypatch, arm):
    if arm == "chain":
        monkeypatch.setenv("SEZKP_NTT_TW_TABLE", "0")


def _vec(oracle, kind, log_n):
    """(x, forward transform of x), computed once per (kind, size)."""
    if (kind, log_n) not in _ref:
        n = 1 << log_n
        if log_n > 20:
            oracle.use_mt(int(os.environ.get("OMP_NUM_THREADS", "8")))
        if kind == "random":
            x = oracle.det_vec(n, 900 + log_n)
        else:  # the edge vectors of test_ntt_edge_values_match_oracle
            x = EDGE[np.random.default_rng(log_n).integers(0, len(EDGE), n)]
            x[: n // 4] = P - 1
        want = oracle.ntt_forward(x)
        x.setflags(write=False)
        want.setflags(write=False)
        _ref[(kind, log_n)] = (x, want)
    return _ref[(kind, log_n)]


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("kind", ["random", "edge"])
@pytest.mark.parametrize("log_n", [13, 14])
def test_dif_forward_and_inverse(gpu_ok, product, oracle, monkeypatch, log_n, kind, arm):
    """ntt_dif forward on x and ntt_dif inverse on the oracle's transform
    (no scratch: the DIF passes, then the in-place bit reversal)."""
    torch = gpu_ok
    _set_arm(monkeypatch, arm)
    x, want = _vec(oracle, kind, log_n)
    d = _dev(torch, x)
    assert product.lib.sezkp_gl_ntt(d.data_ptr(), None, log_n, 1, None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_host(d), want)
    d = _dev(torch, want)
    assert product.lib.sezkp_gl_ntt(d.data_ptr(), None, log_n, -1, None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_host(d), x)


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("kind", ["random", "edge"])
@pytest.mark.parametrize("log_n", [13, 14])
def test_dit_inverse(gpu_ok, product, oracle, monkeypatch, log_n, kind, arm):
    """One rank's dist_ntt inverse: bit reversal, then the inverse DIT passes."""
    torch = gpu_ok
    _set_arm(monkeypatch, arm)
    x, want = _vec(oracle, kind, log_n)
    ctx = product.ProverContext(0)
    try:
        d = _dev(torch, want)
        ctx.dist_ntt(d, inverse=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_host(d), x)
    finally:
        ctx.close()


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("kind", ["random", "edge"])
@pytest.mark.parametrize("log_n", [21, 22])
def test_dit_natural_forward_and_inverse(gpu_ok, product, oracle, monkeypatch, log_n, kind, arm):
    """The natural-order DIT (with scratch), forward and inverse: the first
    sizes at which a plain forward DIT runs."""
    torch = gpu_ok
    _set_arm(monkeypatch, arm)
    x, want = _vec(oracle, kind, log_n)
    d = _dev(torch, x)
    scratch = torch.empty_like(d)
    assert product.lib.sezkp_gl_ntt(d.data_ptr(), scratch.data_ptr(), log_n, 1, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(d, _dev(torch, want))
    assert product.lib.sezkp_gl_ntt(d.data_ptr(), scratch.data_ptr(), log_n, -1, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(d, _dev(torch, x))


def _lde_case(oracle, kind, log_n):
    if ("lde", kind, log_n) not in _ref:
        n = 1 << log_n
        if kind == "random":
            base, z = oracle.det_vec(n, 7 + log_n), 0x1234567890ABCDEF % P
        else:  # as test_coset_lde_deep_edge_values
            eps = (1 << 32) - 1
            edge = np.array([0, 1, P - 1, P - 2, eps, 1 << 32, 1 << 63, P - eps, (1 << 64) - (1 << 33)],
                            dtype=np.uint64)
            base = edge[np.random.default_rng(log_n).integers(0, len(edge), n)]
            base[: n // 2] = P - 1
            z = P - 1
        want = oracle.lde_deep(base, 3, z)
        base.setflags(write=False)
        want.setflags(write=False)
        _ref[("lde", kind, log_n)] = (base, z, want)
    return _ref[("lde", kind, log_n)]


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("kind", ["random", "edge"])
@pytest.mark.parametrize("log_n", [10, 11, 13, 14])
def test_coset_lde_deep(gpu_ok, product, oracle, monkeypatch, log_n, kind, arm):
    """INTT (DIF inverse) -> coset LDE x8 (forward DIT from the replicated
    load) -> DEEP: N = 2^13 and 2^14 (the smallest forward DIT with a table
    pass, DEEP as a kernel / fused), 2^16 (m = 8, sL = 8, fused) and 2^17."""
    torch = gpu_ok
    _set_arm(monkeypatch, arm)
    base, z, want = _lde_case(oracle, kind, log_n)
    d_in = _dev(torch, base)
    d_out = torch.empty(8 << log_n, dtype=torch.int64, device="cuda")
    assert product.lib.sezkp_gl_coset_lde_deep(d_in.data_ptr(), log_n, 3, 3, z, d_out.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_host(d_out), want)


@pytest.mark.parametrize("arm", ARMS)
def test_prove_both_arms(gpu_ok, product, oracle, monkeypatch, arm):
    """A whole proof at T = 2^12 (the DEEP-polynomial LDE of N = 2^15 = 8 + 7:
    second pass m = 7, sL = 8) under either arm: the oracle's bytes."""
    _set_arm(monkeypatch, arm)
    if "prove" not in _ref:
        blocks = product.synthetic_blocks(1 << 12, 512, 2, 77)
        root = blocks.manifest_root()
        _ref["prove"] = (blocks, root, oracle.prove_v1(blocks, root))
    blocks, root, want = _ref["prove"]
    ctx = product.ProverContext(0)
    try:
        ctx.upload(blocks)
        assert ctx.prove(root).proof_bytes == want
    finally:
        ctx.close()
