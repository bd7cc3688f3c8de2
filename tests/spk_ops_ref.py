"""Plain numpy statements of the speaker encoder's own kernels (csrc/q3_spk.hip), one op each, with the error a correct fp32
implementation of the kernel's order may have -- test infrastructure for tests/test_gpu_spk_ops.py, pinned on the CPU by
tests/test_glue_ops_reference.py (composed in spk_run's order they are tests/spk_ref.py's network).

Data movement (unfold, place) is exact: the functions keep the input's dtype, so float32 in gives the bits the kernel must
give (x + x2 is then the one float32 add the kernel makes), float64 in gives the float64 network.

Real-data ops return (reference in float64, bound), the bound element-wise and computed from the inputs alone.  U = 2^-24 is
the unit roundoff.  A row reduction is lane-strided partial sums (ceil(n / 64) terms per lane) and a 6-stage butterfly, so a
term passes through at most depth(n) = ceil(n / 64) + 6 additions; the op's own roundings (1 / L, a product, the bias add, the
final divide) come on top, with one to spare:
  rowmean   (depth + 2) U mean|x|
  matvec    dv = (depth + 2) U (|bias| + sum |w||x|); ReLU keeps it; sigmoid: dv / 4 + SIGMOID_ERR
  rowstat   mean: dm = (depth + 2) U mean|x|;  with d = x - mean and e = U |d| + dm (the device's d),
            variance: dv = mean(2 |d| e + e^2) + (depth + 3) U var;  std through |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b)
            around the 1e-12f clamp, plus the root's own rounding
  attnpool  the same with the softmax weights a in the place of 1 / L: a weight's relative error is r = U |z - max| + EXPF_REL
            (the subtraction, expf) + the denominator's + the divide's
  se_apply  U (|h g| + |h g + res|): two roundings, or one when the compiler contracts the multiply-add
  att_act   exactly 0 where the float32 sum x + bias is <= 0; else U |x + bias| + TANH_ERR (tanh is 1-Lipschitz)

EXPF_REL is the 4 ulp the project budgets for expf (tests/sample_ref.py).  TANH_ERR and SIGMOID_ERR are not derivable: they
are the device's tanhf on [0, 12] and 1 / (1 + expf(-v)) on [-30, 30] against float64, measured on a dense grid through the
hooks in their identity setting (test_device_function_probes) and rounded up to a power of two; their ceiling is 4 ulp of a
result bounded by 1, PROBE_CEILING."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
EXPF_REL = 4 * 2.0 ** -23
PROBE_CEILING = 4 * 2.0 ** -24
TANH_MEASURED, TANH_ERR = 7.500e-8, 2.0 ** -23            # |tanhf (device) - float64|, 0 <= x <= 12
SIGMOID_MEASURED, SIGMOID_ERR = 8.873e-8, 2.0 ** -23      # |1 / (1 + expf(-v)) (device) - float64|, |v| <= 30
STD_FLOOR = float(np.float32(1e-12))                    # the kernels' clamp under the root
GRADE = 2e-4                                            # the project's stage grade: a one-op bound stays under it

LENGTHS = (5, 6, 63, 64, 65, 129, 300)
BATCHES = ((5, 300, 64), (65, 6, 129), (63, 5, 6))      # ragged batches of 3; every clip also runs alone
CHANNELS = (1, 4, 5, 6, 130)                            # one workgroup is 4 rows: idle waves at 1, 5, 6, 130
MATVEC_I = (1, 63, 64, 65, 192, 3072)


def pitch(L):
    return (int(L) + 31) & ~31


def depth(n):
    return -(-int(n) // 64) + 6


def reflect(i, L):
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i >= L, 2 * (L - 1) - i, i))


# ---- data movement -------------------------------------------------------------------------------------------------
def unfold(x, c0, C, K, dil, n_f, x2=None, c02=0):
    """x [B][Cx][Lmax] (+ x2 [B][Cx2][Lmax]) -> y [B][C * K][pitch(Lmax)]: row ci * K + j, column l < L_b is
    x[c0 + ci][reflect(l + j * dil - dil * (K - 1) / 2)] (+ x2[c02 + ci][the same column]); +0 from L_b to the pitch"""
    B, _, Lmax = x.shape
    y = np.zeros((B, C * K, pitch(Lmax)), x.dtype)
    p = dil * (K - 1) // 2
    for b in range(B):
        L = int(n_f[b])
        for j in range(K):
            src = reflect(np.arange(L) + j * dil - p, L)
            v = x[b, c0:c0 + C][:, src]
            if x2 is not None:
                v = v + x2[b, c02:c02 + C][:, src]
            y[b, j::K, :L] = v
    return y


def place(x, c0x, C, relu):
    """channels [c0x, c0x + C) of x [B][Cx][ld], ReLU'd or not: what the destination's slice holds"""
    v = x[:, c0x:c0x + C]
    return np.maximum(v, 0) if relu else v.copy()


# ---- reductions and the matvec --------------------------------------------------------------------------------------
def rowmean(x, n_f):
    """x [B][C][Lmax] -> (mean [B][C], bound)"""
    B, C, _ = x.shape
    ref, bound = np.zeros((B, C)), np.zeros((B, C))
    for b in range(B):
        L = int(n_f[b])
        xb = np.asarray(x[b, :, :L], np.float64)
        ref[b] = xb.sum(1) / L
        bound[b] = (depth(L) + 2) * U * np.abs(xb).mean(1)
    return ref, bound


def _weighted_stats(xb, a, L, ra):
    """rows xb [C][L], weights a [C][L] (rows sum to 1) whose device values are off by at most ra (relative, [C][L]) plus
    2^-126 -> (mean, std, their bounds)"""
    D = depth(L)
    tiny = 2.0 ** -126
    mean = (a * xb).sum(1)
    dm = (a * np.abs(xb) * ra).sum(1) + tiny * np.abs(xb).sum(1) + (D + 1) * U * (a * np.abs(xb)).sum(1)
    d = xb - mean[:, None]
    e = U * np.abs(d) + dm[:, None]
    var = (a * d * d).sum(1)
    dv = (a * (2 * np.abs(d) * e + e * e)).sum(1) + (a * d * d * (ra + U)).sum(1) + tiny * (d * d).sum(1) + (D + 1) * U * var
    vc, lo = np.maximum(var, STD_FLOOR), np.maximum(var - dv, STD_FLOOR)
    std = np.sqrt(vc)
    dstd = dv / (std + np.sqrt(lo)) * (1 + U) + U * std
    return mean, std, dm, dstd


def rowstat(x, n_f):
    """x [B][C][Lmax] -> (stat [B][2 C] = mean | std with the weights 1 / L, bound [B][2 C])"""
    B, C, _ = x.shape
    ref, bound = np.zeros((B, 2 * C)), np.zeros((B, 2 * C))
    for b in range(B):
        L = int(n_f[b])
        xb = np.asarray(x[b, :, :L], np.float64)
        a = np.full((C, L), 1.0 / L)
        ref[b, :C], ref[b, C:], bound[b, :C], bound[b, C:] = _weighted_stats(xb, a, L, np.full((C, L), U))   # (1 / L rounds once)
    return ref, bound


def attnpool(z, x, n_f):
    """z, x [B][C][Lmax] -> (pooled [B][2 C] = mean | std under a = softmax(z) over the clip's own columns, bound)"""
    B, C, _ = x.shape
    ref, bound = np.zeros((B, 2 * C)), np.zeros((B, 2 * C))
    for b in range(B):
        L = int(n_f[b])
        xb, zb = np.asarray(x[b, :, :L], np.float64), np.asarray(z[b, :, :L], np.float64)
        t = zb - zb.max(1, keepdims=True)
        e = np.exp(t)
        den = e.sum(1, keepdims=True)
        r = U * np.abs(t) + EXPF_REL
        rd = (e * r).sum(1, keepdims=True) / den + depth(L) * U
        ref[b, :C], ref[b, C:], bound[b, :C], bound[b, C:] = _weighted_stats(xb, e / den, L, r + rd + U)
    return ref, bound


def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def matvec(w, bias, x, act):
    """w [O][I], bias [O] or None, x [B][I] -> (act(bias + w x) [B][O], bound); act 0 none, 1 ReLU, 2 sigmoid"""
    w64, x64 = np.asarray(w, np.float64), np.asarray(x, np.float64)
    v = x64 @ w64.T
    mag = np.abs(x64) @ np.abs(w64).T
    if bias is not None:
        v = v + np.asarray(bias, np.float64)
        mag = mag + np.abs(np.asarray(bias, np.float64))
    dv = (depth(w64.shape[1]) + 2) * U * mag
    if act == 1:
        return np.maximum(v, 0.0), dv
    if act == 2:
        return sigmoid64(v), 0.25 * dv + SIGMOID_ERR
    return v, dv


# ---- element-wise ---------------------------------------------------------------------------------------------------
def se_apply(h, gate, res):
    """h, res [B][C][ld], gate [B][C] -> (h * gate + res, bound)"""
    hg = np.asarray(h, np.float64) * np.asarray(gate, np.float64)[:, :, None]
    y = hg + np.asarray(res, np.float64)
    return y, U * (np.abs(hg) + np.abs(y))


def att_act(x, bias):
    """x [B][C][ld], bias [B][C] -> (tanh(relu(x + bias)), bound, zero): zero marks where the float32 sum is <= 0 (the
    result is then exactly 0; with float64 inputs: where the float64 sum is)"""
    s = x + bias[:, :, None]                      # in the inputs' dtype: float32 in, the kernel's own rounded sum
    s64 = np.asarray(x, np.float64) + np.asarray(bias, np.float64)[:, :, None]
    zero = s <= 0
    ref = np.where(zero, 0.0, np.tanh(np.maximum(s64, 0.0)))
    return ref, np.where(zero, 0.0, U * np.abs(s64) + TANH_ERR), zero


# ---- the cases' data (shared by the CPU pin and the GPU tests: the bound cap is asserted on exactly these) ------------
def _seed(*key):
    """a seed from small integers and short strings that does not depend on the interpreter's string hashing"""
    out = []
    for k in key:
        out.append(int(k) if isinstance(k, (int, np.integer)) else sum((i + 1) * ord(ch) for i, ch in enumerate(str(k))))
    return np.random.default_rng(out)


def rows(lens, C, kind, seed=0):
    """[B][C][Lmax] float32 rows, NaN past each clip's own length.  kind: 'real' a per-row mean of +-[0.5, 2] and spread of
    [0.5, 1.5] (the mean is never small against the bound's sum |x|); 'int' integers |x| <= 2^10; 'intstat' integers |x| <= 2^4
    whose row sums are multiples of the length (every d = x - mean is an integer: the variance is exact too)"""
    r = _seed("rows", kind, C, seed, *lens)
    B, Lmax = len(lens), max(lens)
    x = np.full((B, C, Lmax), np.nan, np.float32)
    for b, L in enumerate(lens):
        if kind == "real":
            mu = r.uniform(0.5, 2.0, (C, 1)) * r.choice([-1.0, 1.0], (C, 1))
            v = mu + r.uniform(0.5, 1.5, (C, 1)) * r.standard_normal((C, L))
        elif kind == "int":
            v = r.integers(-2 ** 10, 2 ** 10 + 1, (C, L)).astype(np.float64)
        else:
            v = r.integers(-14, 15, (C, L)).astype(np.float64)
            v -= np.arange(L)[None, :] < (v.sum(1) % L)[:, None]      # 1 off the first (sum mod L) columns: |x| <= 15
        x[b, :, :L] = v
    return x


def rowstat_edge_rows(L):
    """-> x [1][4][L], names: a constant power of two, (mean, std) = (4, 0.05), (-30, 2), one outlier"""
    r = _seed("edge", L)
    x = np.zeros((1, 4, L), np.float32)
    x[0, 0] = 0.25
    x[0, 1] = 4.0 + 0.05 * r.standard_normal(L)
    x[0, 2] = -30.0 + 2.0 * r.standard_normal(L)
    x[0, 3] = r.standard_normal(L)
    x[0, 3, L // 2] = 1000.0
    return x, ("const", "mean 4 std 0.05", "mean -30 std 2", "outlier")


def matvec_case(I, O, B, with_bias, seed=0):
    """w in [0.5, 1.5) / I, x in [0.5, 1.5): sum w x is in [0.25, 2.25] and sum |w||x| is the same number; the bias is +[0.5, 1] at
    even outputs and -[3, 4] at odd ones, so the ReLU clips, the sigmoid runs over [-3.75, 3.25], and output 0 is never small
    against the bound's magnitude (the cap of section 3 holds from the reference alone)"""
    r = _seed("matvec", I, O, B, int(with_bias), seed)
    w = (r.uniform(0.5, 1.5, (O, I)) / I).astype(np.float32)
    x = r.uniform(0.5, 1.5, (B, I)).astype(np.float32)
    bias = None
    if with_bias:
        bias = np.where(np.arange(O) % 2 == 0, r.uniform(0.5, 1.0, O), -r.uniform(3.0, 4.0, O)).astype(np.float32)
    return w, bias, x


def attn_logits(lens, C, kind, seed=0):
    """z [B][C][Lmax] float32, NaN past the clip.  'normal': N(0, 1); 'hot0' / 'hotlast' / 'hot63': one column ahead of the rest
    by >= 120 (column 0, L - 1, the last column = 63 mod 64 -- column 0 where the clip has fewer than 64); 'zero', 'p80', 'm1e4':
    all equal"""
    r = _seed("logits", kind, C, seed, *lens)
    B, Lmax = len(lens), max(lens)
    z = np.full((B, C, Lmax), np.nan, np.float32)
    for b, L in enumerate(lens):
        if kind == "normal":
            v = r.standard_normal((C, L))
        elif kind in ("zero", "p80", "m1e4"):
            v = np.full((C, L), {"zero": 0.0, "p80": 80.0, "m1e4": -1e4}[kind])
        else:
            v = r.standard_normal((C, L))
            v[:, hot_column(kind, L)] += 140.0           # two normals differ by less than 20
        z[b, :, :L] = v
    return z


def hot_column(kind, L):
    if kind == "hot0":
        return 0
    if kind == "hotlast":
        return L - 1
    return ((L - 64) // 64) * 64 + 63 if L >= 64 else 0


def se_case(L, C, B, seed=0):
    """h, res [B][C][pitch(L)] ~ N(0, 1) over every column of the pitch, gate [B][C] in (0, 1)"""
    r = _seed("se", L, C, B, seed)
    shape = (B, C, pitch(L))
    return (r.standard_normal(shape).astype(np.float32), r.uniform(0.02, 0.98, (B, C)).astype(np.float32),
            r.standard_normal(shape).astype(np.float32))


def att_case(L, C, B, seed=0):
    """x [B][C][pitch(L)], bias [B][C] in [-1, 1]: x + bias spans [-4, 12] (both ends are hit), a third of it is <= 0"""
    r = _seed("att", L, C, B, seed)
    bias = r.uniform(-1.0, 1.0, (B, C)).astype(np.float32)
    s = r.uniform(-4.0, 12.0, (B, C, pitch(L)))
    s[:, :, 0], s[:, :, 1], s[:, :, 2] = -4.0, 12.0, 0.0
    return (s - bias[:, :, None]).astype(np.float32), bias


def grid(lo, hi, n):
    """n float32 points over [lo, hi], both ends included"""
    return np.linspace(lo, hi, n).astype(np.float32)


def scale_of(ref, C=None, std_clamped=None):
    """the cap's scale: max |ref| over the case's output; for a [B][2 C] mean | std output the std half is graded against
    the row's own std (1e-6 where the clamp holds it)"""
    if C is None:
        return np.full(ref.shape, float(np.abs(ref).max()))
    s = np.empty(ref.shape)
    s[:, :C] = float(np.abs(ref[:, :C]).max())
    s[:, C:] = np.maximum(ref[:, C:], 1e-6)
    return s
