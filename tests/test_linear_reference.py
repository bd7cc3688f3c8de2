"""tests/linear_ref.py (the float64 reference tests/test_gpu_linear.py grades every linear / GEMM kernel variant with) against
the oracle's exported primitives (oracle/q3_oracle.c: orc_round_f16_array, orc_rmsnorm_fold, orc_matvec -- the oracle is
itself pinned to transformers' Qwen3Model by tests/test_oracle_vs_hf.py) and against plain RMSNorm followed by a
projection in float64, so the kernels' reference cannot share a misunderstanding with the kernels.  CPU only."""
import numpy as np
import pytest

from oracle import oracle
from tests import linear_ref as L


def edge_values():
    """f32 inputs around every fp16 boundary: ties, the subnormal range, the largest finite value and beyond."""
    rng = np.random.default_rng(11)
    v = [0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -24, 2.0 ** -25,
         2.0 ** -25 + 2.0 ** -40, 3 * 2.0 ** -25, 2.0 ** -26, 1e-8, 5.9e-8, 6.1e-5, 65504.0, 65519.9, 65520.0, 65536.0, 7e4,
         1e6, 3e38, np.inf]
    v = np.array(v + [-x for x in v], np.float32)
    r = (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 12, 4096))).astype(np.float32)
    sub = (rng.uniform(-1, 1, 1024) * 2.0 ** -14).astype(np.float32)
    return np.concatenate([v, r, sub])


def test_round_f16_sat_matches_the_oracle_bit_for_bit():
    x = edge_values()
    want = oracle.round_f16(x)
    got = L.round_f16_sat(x)
    assert np.isfinite(got.astype(np.float32)).all()
    np.testing.assert_array_equal(got.astype(np.float32).view(np.uint32), want.view(np.uint32))
    assert float(L.round_f16_sat(np.float32(np.inf))) == 65504.0 and float(L.round_f16_sat(np.float32(-1e9))) == -65504.0
    assert float(L.round_f16_sat(np.float32(2.0 ** -25))) == 0.0            # tie to even
    assert float(L.round_f16_sat(np.float32(3 * 2.0 ** -25))) == 2.0 ** -23  # tie to even, upwards


@pytest.mark.parametrize("scale,eps", [(3.0, 1e-6), (1e-4, 1e-6), (1e-4, 1e-3), (0.0, 1e-6), (3e5, 1e-6)])
def test_fold_matches_the_oracle(scale, eps):
    """pre_scaled is bit-equal to the oracle's GEMM input (saturating rows and rows in the fp16 subnormals included);
    post_scale from the 16-column partials equals the oracle's factor to f32 round-off."""
    K = 1024
    rng = np.random.default_rng(5)
    h = (scale * rng.standard_normal(K)).astype(np.float32)
    gamma = (1.0 + 0.5 * rng.standard_normal(K)).astype(np.float32)
    if scale > 1e5:
        gamma[:8] = 40.0             # |h * gamma| / 16 beyond 65504 on some entries
    x16 = np.empty(K, np.float32)
    post = oracle.lib().orc_rmsnorm_fold(oracle.fp(h), oracle.fp(gamma), np.float32(eps), K, oracle.fp(x16))
    got = L.pre_scaled(h, gamma)
    np.testing.assert_array_equal(got.astype(np.float32).view(np.uint32), x16.view(np.uint32))
    if scale > 1e5:
        assert (np.abs(got.astype(np.float32)) == 65504.0).any()
    if 0 < scale < 1e-3:
        tiny = np.abs(got.astype(np.float32))
        assert ((tiny > 0) & (tiny < 2.0 ** -14)).any()      # subnormal GEMM inputs were pinned too
    mine = L.post_scale(L.ssq_partials(h[None]), K, eps)[0]
    assert abs(mine - post) <= 4 * L.U24 * mine


def test_linear_matches_the_oracle_matvec():
    """The float64 product against the oracle's f32 matvec on the same fp16 values, within the accumulation bound."""
    N, K = 96, 2048
    rng = np.random.default_rng(6)
    W = (0.05 * rng.standard_normal((N, K))).astype(np.float16)
    x = rng.standard_normal((1, K)).astype(np.float16)
    y = np.empty(N, np.float32)
    Wf, xf = np.ascontiguousarray(W.astype(np.float32)), np.ascontiguousarray(x[0].astype(np.float32))
    oracle.lib().orc_matvec(oracle.fp(Wf), oracle.fp(xf), oracle.fp(y), N, K)
    ref, ab = L.linear(x, W)
    assert (np.abs(y - ref[0]) <= L.acc_bound(ab[0], K) + L.ulp32(ref[0])).all()
    assert (ab >= np.abs(ref)).all()
    # a dropped 32-wide k-block is far outside that bound
    ref_drop, _ = L.linear(x[:, :-32], W[:, :-32])
    assert np.median(np.abs(ref_drop - ref) / L.acc_bound(ab, K)) > 10


@pytest.mark.parametrize("eps", [1e-6, 1e-2])
def test_fold_is_rmsnorm_then_projection(eps):
    """Folded form == plain RMSNorm (x * rsqrt(mean(x^2) + eps) * gamma) followed by the projection, in float64.  The
    only difference is the fp16 rounding of the GEMM input: per output at most sum_k 2^-11 |xh_k| |w_k| * post, and with
    the unrounded input the two agree to float64 round-off."""
    M, N, K = 5, 64, 1024
    rng = np.random.default_rng(7)
    h = (np.array([3.0, 1e-4, 0.0, 40.0, 0.3])[:, None] * rng.standard_normal((M, K))).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    W = (0.05 * rng.standard_normal((N, K))).astype(np.float16)
    h64, g64, W64 = h.astype(np.float64), gamma.astype(np.float64), W.astype(np.float64)
    plain = (h64 / np.sqrt((h64 * h64).mean(-1, keepdims=True) + np.float64(np.float32(eps))) * g64) @ W64.T
    post = L.post_scale(L.ssq_partials(h), K, eps)
    # unrounded fold: identical but for float64 round-off
    exact = L.store(((h64 * g64) * 0.0625) @ W64.T, post)
    np.testing.assert_allclose(exact, plain, rtol=1e-12, atol=1e-300)
    xh = L.pre_scaled(h, gamma)
    acc, ab = L.linear(xh, W)
    folded = L.store(acc, post)
    # rounding of the input: half an fp16 ulp relative on normal values (2^-11), 2^-25 absolute in the subnormals, plus the
    # two f32 roundings of (h * gamma) / 16 before it
    slack = (2.0 ** -11 + 2 * L.U24) * ab + 2.0 ** -25 * np.abs(W64).sum(-1)[None, :]
    assert (np.abs(folded - plain) <= slack * post[:, None] + 1e-300).all()
    assert (folded[2] == 0).all() and (plain[2] == 0).all()       # the all-zero row: eps alone keeps it finite
    # and the rounding is really there (the bound is not vacuous by orders of magnitude)
    assert np.abs(folded - plain)[0].max() > 1e-3 * (slack * post[:, None])[0].max()


def test_epilogues():
    rng = np.random.default_rng(8)
    acc = rng.standard_normal((3, 64)) * 4
    post = np.array([1.0, 2.0, 0.5])
    out, g, u = L.swiglu(acc, post)
    np.testing.assert_array_equal(g, acc[:, :32] * post[:, None])
    np.testing.assert_array_equal(u, acc[:, 32:] * post[:, None])
    np.testing.assert_allclose(out, g / (1 + np.exp(-g)) * u, rtol=1e-15)
    assert float(L.round_f16_sat(np.float32(L.swiglu(np.array([[300.0, 400.0]]))[0][0, 0]))) == 65504.0
    h = rng.standard_normal((3, 64)).astype(np.float32)
    np.testing.assert_array_equal(L.resid(h, acc), h.astype(np.float64) + acc)
    p = L.ssq_partials(h)
    assert p.shape == (3, 4)
    np.testing.assert_allclose(p[1, 2], (h[1, 32:48].astype(np.float64) ** 2).sum(), rtol=1e-15)
    # |silu'| <= 1.1 (what the GPU test propagates the accumulator bounds with)
    x = np.linspace(-30, 30, 200001)
    assert np.abs(np.gradient(L.silu(x), x)).max() < 1.1
    assert L.ulp16(1.0) == 2.0 ** -10 and L.ulp16(65504.0) == 32.0 and L.ulp16(1e9) == 32.0 and L.ulp16(0.0) == 2.0 ** -24
