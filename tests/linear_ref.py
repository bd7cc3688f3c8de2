"""Float64 restatement of the linear kernels' contract (csrc/q3_kernels.h): what tests/test_gpu_linear.py
grades every linear_kernel / linear_narrow_kernel / gemm_glds_kernel / gemm_kernel instantiation with.  numpy only.

One function per piece of the contract:
  * every GEMM input is fp16, rounded to nearest even with saturation at +-65504 (round_f16_sat);
  * RMSNorm is folded around the GEMM: the producer of a residual row h writes xh = fp16_sat((h * gamma) / 16)
    (pre_scaled, evaluated in float32: bit-comparable) and 16-column sums of squares (ssq_partials); the consumer
    multiplies its f32 accumulators by 16 / sqrt(sum(ssq) / K + eps) (post_scale);
  * the product itself is exact fp16 x fp16 products summed in f32 (linear: the float64 sum, and sum |x| |w|, from which
    the accumulation error bounds follow);
  * epilogues: store, h += y with new partials and the next consumer's xh (resid), SwiGLU over gate rows [0, N/2) and up
    rows [N/2, N) (swiglu).
tests/test_linear_reference.py pins this file against the oracle's primitives and against plain RMSNorm + projection."""
import numpy as np

F16_MAX = 65504.0
NORM_PRE = np.float32(0.0625)
NORM_POST = 16.0
U24 = 2.0 ** -24          # unit round-off of f32


def round_f16_sat(x):
    """f32 -> fp16, round to nearest even, saturating at +-65504 (never inf)."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.clip(x, np.float32(-F16_MAX), np.float32(F16_MAX)).astype(np.float16)


def pre_scaled(h, gamma):
    """The producer's GEMM input xh = fp16_sat((f32(h) * f32(gamma)) * 0.0625), every step in float32."""
    h = np.asarray(h, np.float32)
    gamma = np.asarray(gamma, np.float32)
    with np.errstate(over="ignore"):
        return round_f16_sat((h * gamma) * NORM_PRE)


def ssq_partials(h):
    """[M][K] -> [M][K/16] sums of squares of 16 consecutive columns (float64)."""
    h = np.asarray(h, np.float64)
    return (h * h).reshape(h.shape[0], h.shape[1] // 16, 16).sum(-1)


def post_scale(ssq, K, eps):
    """[M][parts] partials -> [M] the consumer's accumulator scale 16 / sqrt(mean square + eps) (float64)."""
    return NORM_POST / np.sqrt(np.asarray(ssq, np.float64).sum(-1) / K + np.float64(np.float32(eps)))


def linear(x16, W16):
    """fp16 x[M][K], W[N][K] -> (x . W^T in float64, abs_bound = |x| . |W|^T in float64)."""
    assert x16.dtype == np.float16 and W16.dtype == np.float16
    x = x16.astype(np.float64)
    w = W16.astype(np.float64)
    return x @ w.T, np.abs(x) @ np.abs(w).T


def acc_bound(abs_bound, K):
    """Worst case of K f32 additions of exact products in any order: |acc - ref| <= K 2^-24 sum |x w|."""
    return K * U24 * abs_bound


def store(acc, post=None):
    """EPI_STORE: y = acc (* post[m] with the norm prologue)."""
    return acc if post is None else acc * np.asarray(post, np.float64)[:, None]


def resid(h, acc):
    """EPI_RESID, the part that depends on the accumulators: h + acc in float64."""
    return np.asarray(h, np.float64) + acc


def silu(g):
    g = np.asarray(g, np.float64)
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


def swiglu(acc, post=None):
    """EPI_SWIGLU: acc[M][N] with gate columns [0, N/2) and up columns [N/2, N) -> (silu(g) * u in float64 [M][N/2], g, u).
    The stored value is round_f16_sat of the first."""
    y = store(acc, post)
    half = y.shape[1] // 2
    g, u = y[:, :half], y[:, half:]
    return silu(g) * u, g, u


def ulp16(x):
    """Spacing of fp16 at |x| (that of the top binade at and beyond +-65504), float64."""
    a = np.minimum(np.abs(np.asarray(x, np.float64)), F16_MAX - 32.0).astype(np.float16)
    return np.spacing(a).astype(np.float64)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
