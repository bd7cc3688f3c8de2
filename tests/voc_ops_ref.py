"""One-op vocoder tables for everything in csrc/q3_voc_kernels.hip that is not a conv -- chan_norm, dwconv, glu, rvq, embmean, the
two full-chunk attention kernels behind the VOP_ATTN dispatch -- and for the carry-state kernels of the incremental decode
(voc_incr_prepend, voc_incr_prepend_split, voc_attn_incr), with their float64 / int64 references and derived error bounds.

The conventions are tests/voc_conv_ref.py's: a case table is  [front] -> the op(s) under test -> _tail(C),  every
launch goes through voc_load / voc_debug_run (or voc_incr_create / a push), and the input activation is chosen bit for bit through
a VOP_EMBMEAN nq = 1, cb = T front driven with a permutation in codes[b][t][0].  The fronts themselves (VOP_RVQ, VOP_EMBMEAN with
nq > 1) are op 0 of their tables.  The conv rows of a table are evaluated by voc_conv_ref.conv_f64 / conv_int: one conv reference.
tests/test_voc_ops_reference.py pins the float64 walk to oracle/voc_ref.py on every table, tests/test_gpu_voc_ops.py and
tests/test_gpu_voc_incr_ops.py run them on the device.

Error bounds (float64 reference y, device value yd; per output element; U = 2^-24; an input that already carries an error e_x
adds what the formulas below say under "chain").  Every rounding below the normal range of f32 (a subnormal result, or one flushed to
zero) costs up to TINY = 2^-126 instead of U times the value: each formula carries that floor once per rounding it counts.
It is the one term added to the formulas as first stated: a subnormal norm output (input -1e-40) missed the purely relative bound
by 19 x on the device; at 1e-38 absolute it covers no arithmetic error.
------------------------------------------------------------------------------------------------------------------------------
dwconv   |yd - y| <= (2K + 2) U S,  S = sum_k |w_k| |x| + |bias|
    K products and K adds (the first one onto the bias), each at most U S; the +2 is slack for the store; + (2K + 2) TINY.
    chain: + sum |w| e_x.

norm     propagated in the kernel's order (C channels of one column; LayerNorm; RMSNorm has mu = 0 and no step 1):
    1. mu = (sum x) / C in f32: C - 1 adds in any order and one division: d_mu = (C + 1) U mean|x|          (chain: + mean e_x)
    2. d = x - mu: |error| <= d_mu + U |d|                                  (the term that matters when |d| << |mu|; chain: + e_x)
       call it dd.
    3. ss = sum d^2: every square is off by 2 |d| dd + dd^2 and rounded, the C - 1 adds round:
       d_ss = sum (2 |d| dd + dd^2) + (C + 2) U sum (|d| + dd)^2 + (C + 1) 2^-126       (the last term: squares below the normal range)
    4. v = ss / C + eps (two roundings): d_v = d_ss / C + 2 U v;  inv = 1 / sqrtf(v) (sqrtf and the division are correctly rounded):
       relative error r = d_v / (2 (v - d_v)) + 2 U (1 + 2^-20);  d_v < v / 2 is asserted.
    5. y = (d inv) w + bias, three roundings: |yd - y| <= |w| inv (|d| r + dd (1 + r)) + 2 U |d inv w| + U |y| + 3 TINY
    eps is the f32 value the loader forms, (float)((double)eps_e9 * 1e-9) (q3_voc.hip), not eps_e9 * 1e-9 in double: loader_eps().

glu      y = act(g) u:  |yd - y| <= |u| d_act + 2 U |y| + 2 TINY     (the product's rounding and one U |y| of slack)
    d_act: kind 0 (SiLU, g / (1 + __expf(-g))) SILU_ERR for |g| <= 16, SILU_ERR |g| / 16 beyond (there 1 + expf(-g) is 1 and the
    quotient is g for g > 16, and |silu| < 2e-6 with a relative error of 2^-16 at most for g < -16: both far inside);
    kind 1 (erf GELU) voc_conv_ref.GELU_ERR, scaled by |g| / 8 beyond 8 as in the convs.  SILU_ERR is measured like SIN2_ERR / GELU_ERR:
    test_gpu_voc_ops.py::test_silu_probe compares the device's SiLU (a GLU whose up half is 1) with float64 on a dense grid over
    |x| <= 16; the constant is twice the measured maximum rounded up to a power of two, and the probe asserts measured <= constant on
    every run.  chain: (|u| + e_u) (d_act + Lip e_g) + |act(g)| e_u, Lip = 1.1 for SiLU
    (max of its derivative: 1.0998), 1.13 for GELU.

rvq      y[o] = sum_d p_sem[o][d] e0[d] + sum_d p_ac[o][d] e1[d], e0 = cb_0[id_0], e1 = sum_{q >= 1} cb_q[id_q]
    |yd - y| <= (n + 2) U S over the n = 2 DIM + NQ - 1 terms summed, S = sum |p_sem| |e0| + sum |p_ac| sum_q |cb_q|: the
    accumulator takes each of the 2 DIM products by one fused multiply-add (U S each at most, whatever the order), the NQ - 1
    codebook rows of e1 are added before (U of their magnitudes each, carried through |p_ac|); + (n + 2) TINY.
embmean  y = (sum_q tab_q[id_q]) / NQ: (NQ + 2) U S / NQ + U |y| + (NQ + 2) TINY, S = sum_q |tab_q[id_q]|  (NQ - 1 adds; the division's
    rounding).
    NQ = 1 is exact (x / 1): bound 0, which is what lets a test choose an activation bit for bit.
    An id outside [0, CB) contributes zero to both.

attention  (voc_attn_kernel, voc_attn_tile_kernel, voc_attn_incr_kernel)  __expf / __sincosf / __powf are fast-math forms whose
    error is not derivable: the grade is the project's, max |yd - y| <= ATTN_TOL = 2e-4 of the output's scale
    (tests/test_gpu_attention.py::test_voc_attention_kernels), against tests/attn_ref.voc_attention.

Only numpy and torch (torch for erf, through voc_conv_ref).
"""
from __future__ import annotations

import numpy as np

from qwen3_tts_axera_russian_amd import weights as W
from tests import voc_conv_ref as C
from tests.attn_ref import voc_attention

U = C.U
TINY = 2.0 ** -126      # the smallest normal f32
ATTN_TOL = 2e-4
# measured on an MI355X by test_gpu_voc_ops.py::test_silu_probe (max over the grid), constant = 2 x measured rounded up to a power of two
SILU_MEASURED, SILU_ERR = 1.272e-6, 2.0 ** -18   # |silu (device) - float64|, |x| <= 16
SILU_LIP = 1.1
RES_SAVE, RES_ADD, SNAKE, GELU = W.VF_RES_SAVE, W.VF_RES_ADD, W.VF_SNAKE, W.VF_GELU


def loader_eps(eps_e9):
    """eps of a VOP_NORM row as voc_load forms it: op.eps = (float)((double)r[4] * 1e-9)"""
    return float(np.float32(np.float64(int(eps_e9)) * 1e-9))


def silu64(x):
    x = np.asarray(x, np.float64)
    return x / (1.0 + np.exp(-x))


def grid(lim, n, seed=11):
    """n f32 values: a dense linear grid over [-lim, lim], a geometric one towards zero, zero, subnormals, +-8, +-lim"""
    rng = np.random.default_rng(seed)
    spec = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1.17549435e-38, -1.17549435e-38, 6e-8, -6e-8, 6.1e-5, -6.1e-5, 1.0, -1.0,
                     8.0, -8.0, lim, -lim])
    geo = lim * 2.0 ** -rng.uniform(0, 40, size=n // 8) * rng.choice([-1.0, 1.0], size=n // 8)
    lin = np.linspace(-lim, lim, n - len(spec) - len(geo))
    g = np.concatenate([spec, geo, lin]).astype(np.float32)
    assert g.size == n
    return g


# ----------------------------------------------------------------------------------------------------------------------
# the ops in float64 (with the bound of the device's error) and in int64
# ----------------------------------------------------------------------------------------------------------------------
def _ids(tensors, codes):
    row = np.asarray(tensors["voc.program"])[0]
    nq, cb = int(row[1]), int(row[2])
    ids = np.asarray(codes, np.int64)[:, :, :nq]                 # the first nq of the 16 ids of a frame
    valid = (ids >= 0) & (ids < cb)
    return int(row[0]), nq, cb, np.where(valid, ids, 0), valid


def front_f64(tensors, codes):
    """op 0 of a table (VOP_EMBMEAN or VOP_RVQ) -> (x [B][C][T] float64, bound)"""
    op, nq, cb, idx, valid = _ids(tensors, codes)
    q = np.arange(nq)[None, None, :]
    if op == W.VOP_EMBMEAN:
        tab = np.asarray(tensors["voc.op0.embedding"], np.float64).reshape(nq, cb, -1)
        terms = tab[q, idx] * valid[..., None]                                   # [B][T][nq][dim]
        y = terms.sum(2) / nq
        e = np.zeros_like(y) if nq == 1 else (nq + 2) * U * np.abs(terms).sum(2) / nq + U * np.abs(y) + (nq + 2) * TINY
        return y.transpose(0, 2, 1), e.transpose(0, 2, 1)
    assert op == W.VOP_RVQ
    cbk = np.asarray(tensors["voc.op0.codebook"], np.float64)                    # [nq][cb][dim]
    ps, pa = np.asarray(tensors["voc.op0.proj_sem"], np.float64), np.asarray(tensors["voc.op0.proj_ac"], np.float64)
    terms = cbk[q, idx] * valid[..., None]
    e0, e1, a1 = terms[:, :, 0], terms[:, :, 1:].sum(2), np.abs(terms[:, :, 1:]).sum(2)
    y = e0 @ ps.T + e1 @ pa.T                                                    # [B][T][out]
    S = np.abs(e0) @ np.abs(ps).T + a1 @ np.abs(pa).T
    n = 2 * cbk.shape[2] + nq - 1
    return y.transpose(0, 2, 1), ((n + 2) * (U * S + TINY)).transpose(0, 2, 1)


def front_int(tensors, codes):
    """-> (x int64 [B][C][T], the largest sum of magnitudes an output accumulates)"""
    op, nq, cb, idx, valid = _ids(tensors, codes)
    q = np.arange(nq)[None, None, :]

    def ints(a):
        a = np.asarray(a)
        assert np.all(a == np.round(a))
        return a.astype(np.int64)
    if op == W.VOP_EMBMEAN:
        tab = ints(tensors["voc.op0.embedding"]).reshape(nq, cb, -1)
        terms = tab[q, idx] * valid[..., None]
        s = terms.sum(2)
        assert nq & (nq - 1) == 0 and np.all(s % nq == 0)      # a power of two divides exactly; the tables hold multiples of nq
        return (s // nq).transpose(0, 2, 1), int(np.abs(terms).sum(2).max())
    assert op == W.VOP_RVQ
    cbk, ps, pa = ints(tensors["voc.op0.codebook"]), ints(tensors["voc.op0.proj_sem"]), ints(tensors["voc.op0.proj_ac"])
    terms = cbk[q, idx] * valid[..., None]
    e0, e1, a1 = terms[:, :, 0], terms[:, :, 1:].sum(2), np.abs(terms[:, :, 1:]).sum(2)
    y = e0 @ ps.T + e1 @ pa.T
    mag = np.abs(e0) @ np.abs(ps).T + a1 @ np.abs(pa).T
    return y.transpose(0, 2, 1), int(mag.max())


def dwconv(x, w, bias):
    """x [B][C][L], w [C][K], bias [C] or None -> y[c][l] = bias[c] + sum_k w[c][k] x[c][l - (K - 1 - k)] (any dtype)"""
    L, K = x.shape[2], w.shape[1]
    y = np.zeros_like(x)
    for k in range(K):
        sh = K - 1 - k
        if sh < L:
            y[:, :, sh:] += w[None, :, k, None] * x[:, :, :L - sh]
    return y if bias is None else y + bias[None, :, None]


def dwconv_f64(tensors, i, row, x, ex):
    p, K = f"voc.op{i}.", int(row[3])
    w = np.asarray(tensors[p + "weight"], np.float64).reshape(x.shape[1], K)
    b = np.asarray(tensors[p + "bias"], np.float64) if (p + "bias") in tensors else None
    S = dwconv(np.abs(x) + ex, np.abs(w), None if b is None else np.abs(b))
    return dwconv(x, w, b), dwconv(ex, np.abs(w), None) + (2 * K + 2) * (U * S + TINY)


def dwconv_int(tensors, i, row, x):
    p, K = f"voc.op{i}.", int(row[3])
    w = np.asarray(tensors[p + "weight"]).reshape(x.shape[1], K)
    b = np.asarray(tensors[p + "bias"]) if (p + "bias") in tensors else None
    assert np.all(w == np.round(w)) and (b is None or np.all(b == np.round(b)))
    w, b = w.astype(np.int64), None if b is None else b.astype(np.int64)
    return dwconv(x, w, b), dwconv(np.abs(x), np.abs(w), None if b is None else np.abs(b))


def norm_f64(tensors, i, row, x, ex, eps=None):
    """VOP_NORM over the channels of every column; eps None: the loader's f32 value"""
    p, kind, Cn = f"voc.op{i}.", int(row[3]), x.shape[1]
    eps = loader_eps(row[4]) if eps is None else eps
    w = np.asarray(tensors[p + "weight"], np.float64)[None, :, None]
    b = np.asarray(tensors[p + "bias"], np.float64)[None, :, None] if (p + "bias") in tensors else 0.0
    if kind == 1:
        mu = x.mean(1, keepdims=True)
        d_mu = (Cn + 1) * U * np.abs(x).mean(1, keepdims=True) + ex.mean(1, keepdims=True)
    else:
        mu, d_mu = 0.0, 0.0
    d = x - mu
    dd = d_mu + (U * np.abs(d) if kind == 1 else 0.0) + ex
    ss = (d * d).sum(1, keepdims=True)
    d_ss = (2 * np.abs(d) * dd + dd * dd).sum(1, keepdims=True) + (Cn + 2) * U * ((np.abs(d) + dd) ** 2).sum(1, keepdims=True) \
        + (Cn + 1) * 2.0 ** -126
    v = ss / Cn + eps
    d_v = d_ss / Cn + 2 * U * v
    assert np.all(d_v < v / 2), "the variance is not resolved: no bound"
    inv = 1.0 / np.sqrt(v)
    r = d_v / (2 * (v - d_v)) + 2 * U * (1 + 2.0 ** -20)
    y = d * inv * w + b
    e = np.abs(w) * inv * (np.abs(d) * r + dd * (1 + r)) + 2 * U * np.abs(d * inv * w) + U * np.abs(y) + 3 * TINY
    return y, e


def glu_f64(row, x, ex):
    c, kind = int(row[2]), int(row[3])
    g, u, eg, eu = x[:, :c], x[:, c:], ex[:, :c], ex[:, c:]
    if kind == 0:
        a, d_act, lip = silu64(g), SILU_ERR * np.maximum(1.0, np.abs(g) / 16.0), SILU_LIP
    else:
        a, d_act, lip = C.gelu64(g), C.GELU_ERR * np.maximum(1.0, np.abs(g) / 8.0), C.GELU_LIP
    y = a * u
    return y, (np.abs(u) + eu) * (d_act + lip * eg) + np.abs(a) * eu + 2 * U * np.abs(y) + 2 * TINY


def reference_f64(tensors, codes, n_ops, arith=None, table_eps=False):
    """float64 evaluation of the first n_ops ops -> y [B][C][L]; arith "exact" / "split": -> (y, bound) with the module docstring's
    bound of the device's error propagated through the chain (behind an attention op: ATTN_TOL of its output's scale, a grade, not
    a bound).  table_eps: a norm's eps is eps_e9 * 1e-9 in double, as oracle/voc_ref.py takes it, not the loader's f32 value."""
    prog = np.asarray(tensors["voc.program"])
    x, ex = front_f64(tensors, codes)
    res = eres = None
    for i in range(1, n_ops):
        row = prog[i]
        op, flags = int(row[0]), int(row[5])
        if flags & RES_SAVE:
            res, eres = x, ex                      # the residual is this op's input, whatever the op
        if op in (W.VOP_CONV, W.VOP_CONVT):
            x, ex = C.conv_f64(tensors, i, row, x, ex, res, eres, arith)
        elif op == W.VOP_DWCONV:
            x, ex = dwconv_f64(tensors, i, row, x, ex)
        elif op == W.VOP_NORM:
            x, ex = norm_f64(tensors, i, row, x, ex, int(row[4]) * 1e-9 if table_eps else None)
        elif op == W.VOP_GLU:
            x, ex = glu_f64(row, x, ex)
        elif op == W.VOP_ATTN:
            x = voc_attention(x, int(row[3]), int(row[4]), int(row[6]), float(row[7]))
            ex = np.full_like(x, ATTN_TOL * np.abs(x).max())
        else:
            raise ValueError(f"op {op} inside a table")
    return (x, ex) if arith else x


def reference_int(tensors, codes, n_ops):
    """int64 evaluation of an integer table (fronts, dwconv, the conv rows under voc_conv_ref.conv_int's conditions)
    -> (y int64 [B][C][L], the largest sum of magnitudes any output accumulates: < 2^24 keeps f32 exact in any order)"""
    prog = np.asarray(tensors["voc.program"])
    x, peak = front_int(tensors, codes)
    res = None
    for i in range(1, n_ops):
        row = prog[i]
        op = int(row[0])
        if int(row[5]) & RES_SAVE:
            res = x
        if op in (W.VOP_CONV, W.VOP_CONVT):
            x, mag = C.conv_int(tensors, i, row, x, res)
        elif op == W.VOP_DWCONV:
            x, mag = dwconv_int(tensors, i, row, x)
        else:
            raise ValueError(f"op {op} has no integer form")
        peak = max(peak, int(mag.max()))
    return x, peak


# ----------------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------------
def dw(k, flags=0, bias=True):
    return dict(op=W.VOP_DWCONV, k=k, flags=flags, bias=bias)


def norm(kind, eps_e9=1000, flags=0):
    return dict(op=W.VOP_NORM, kind=kind, eps_e9=eps_e9, flags=flags)


def glu(kind):
    return dict(op=W.VOP_GLU, kind=kind)


def attn(H, D, window, theta=10000):
    return dict(op=W.VOP_ATTN, H=H, D=D, window=window, theta=theta)


def perm_codes(T, seed, B=3):
    """codes[b][t][0] = a permutation of 0 .. T - 1 per chunk; the 15 unused ids of a frame hold values that must not matter"""
    codes = np.zeros((B, T, 16), np.int64)
    rng = np.random.default_rng(seed + 999)
    codes[:, :, 1:] = rng.choice(np.array([-7, 0, 1, 2, T, 2 ** 40, -2 ** 40], np.int64), size=(B, T, 15))
    for b in range(B):
        codes[b, :, 0] = np.random.default_rng(seed + 1000 + b).permutation(T)
    return codes


def real_x(T, cin, rng):
    """as voc_conv_ref.build_table's "real": 2.5 N clipped to |x| <= 8, the extremes, zero and tiny values planted"""
    x = np.clip(2.5 * rng.standard_normal((T, cin)), -8.0, 8.0).astype(np.float32)
    flat = x.reshape(-1)
    for j, v in enumerate((8.0, -8.0, 0.0, 3e-6, -1e-40)):
        flat[(7 * j + 3) % flat.size] = v
    return x


def build_table(ops, x, data, seed):
    """[VOP_EMBMEAN nq = 1, cb = T, table = x [T][Cin]] -> ops -> voc_conv_ref._tail -> (tensors, n_ops of the last op under test).
    data "int": integer weights in [-2, 2] (times a conv's `scale`), integer bias, identity Snake; "real": as
    weights.make_synthetic_voc draws them (conv rows as voc_conv_ref.build_table; dwconv 0.7 N / sqrt K, bias 0.02 N; norm weight
    1 + 0.1 N, LayerNorm bias 0.02 N)."""
    rng = np.random.default_rng(seed)
    T, Cc = x.shape
    prog = [[W.VOP_EMBMEAN, 1, T, Cc, 0, 0, 0, 0]]
    t = {"voc.op0.embedding": np.ascontiguousarray(x, np.float32)}
    for o in ops:
        i = len(prog)
        p = f"voc.op{i}."
        if o["op"] in (W.VOP_CONV, W.VOP_CONVT):
            assert o["op"] == W.VOP_CONV
            prog.append([o["op"], Cc, o["cout"], o["k"], o["p0"], o["flags"], 0, 0])
            shp = (o["cout"], Cc, o["k"])
            if data == "int":
                t[p + "weight"] = (o["scale"] * rng.integers(-2, 3, size=shp)).astype(np.float32)
                if o["bias"]:
                    t[p + "bias"] = (o["scale"] * rng.integers(-4, 5, size=o["cout"])).astype(np.float32)
                if o["flags"] & SNAKE:
                    t[p + "alpha"] = np.full(Cc, C.NO_SNAKE[0], np.float32)
                    t[p + "beta"] = np.full(Cc, C.NO_SNAKE[1], np.float32)
            else:
                gain = 0.25 if (o["flags"] & RES_ADD) else 0.7
                t[p + "weight"] = (gain * rng.standard_normal(shp) / np.sqrt(Cc * o["k"])).astype(np.float32)
                if o["bias"]:
                    t[p + "bias"] = (0.02 * rng.standard_normal(o["cout"])).astype(np.float32)
                if o["flags"] & SNAKE:
                    t[p + "alpha"] = np.minimum(0.3 * rng.standard_normal(Cc), np.log(2.0)).astype(np.float32)
                    t[p + "beta"] = (0.3 * rng.standard_normal(Cc)).astype(np.float32)
            Cc = o["cout"]
        elif o["op"] == W.VOP_DWCONV:
            prog.append([W.VOP_DWCONV, Cc, Cc, o["k"], 1, o["flags"], 0, 0])
            if data == "int":
                t[p + "weight"] = rng.integers(-2, 3, size=(Cc, 1, o["k"])).astype(np.float32)
                if o["bias"]:
                    t[p + "bias"] = rng.integers(-4, 5, size=Cc).astype(np.float32)
            else:
                t[p + "weight"] = (0.7 * rng.standard_normal((Cc, 1, o["k"])) / np.sqrt(o["k"])).astype(np.float32)
                if o["bias"]:
                    t[p + "bias"] = (0.02 * rng.standard_normal(Cc)).astype(np.float32)
        elif o["op"] == W.VOP_NORM:
            prog.append([W.VOP_NORM, Cc, Cc, o["kind"], o["eps_e9"], o["flags"], 0, 0])
            t[p + "weight"] = (1.0 + 0.1 * rng.standard_normal(Cc)).astype(np.float32)
            if o["kind"] == 1:
                t[p + "bias"] = (0.02 * rng.standard_normal(Cc)).astype(np.float32)
        elif o["op"] == W.VOP_GLU:
            prog.append([W.VOP_GLU, Cc, Cc // 2, o["kind"], 0, 0, 0, 0])
            Cc //= 2
        elif o["op"] == W.VOP_ATTN:
            assert Cc == 3 * o["H"] * o["D"]
            prog.append([W.VOP_ATTN, Cc, Cc // 3, o["H"], o["D"], 0, o["window"], o["theta"]])
            Cc //= 3
        else:
            raise ValueError(o)
    n_ops = len(prog)
    for row, tens in C._tail(Cc):
        for n, a in tens.items():
            t[f"voc.op{len(prog)}.{n}"] = a
        prog.append(row)
    t["voc.program"] = np.asarray(prog, np.int32)
    return t, n_ops


EDGE_IDS = (-1, None, 2 ** 40, -2 ** 40)      # None: CB itself


def front_codes(T, nq, cb, seed, B=3):
    """ids in [0, cb) with -1, cb, 2^40 and -2^40 planted in used slots; the unused slots nq .. 15 hold large out-of-range and
    in-range values alike (none of them may reach the result)"""
    rng = np.random.default_rng(seed + 500)
    codes = rng.choice(np.array([2 ** 40, -2 ** 40, 2 ** 62, -5, cb, 0, 1, cb - 1], np.int64), size=(B, T, 16))
    codes[:, :, :nq] = rng.integers(0, cb, size=(B, T, nq))
    used = codes[:, :, :nq].reshape(-1)
    slots = rng.permutation(used.size)[:max(1, min(used.size // 2, 8))]
    for j, sl in enumerate(slots):
        e = EDGE_IDS[j % 4]
        used[sl] = cb if e is None else e
    codes[:, :, :nq] = used.reshape(B, T, nq)
    return codes


def build_front_table(kind, nq, cb, T, data, seed, dim=8, out=8):
    """op 0 under test: VOP_RVQ (codebook [nq][cb][dim], two [out][dim] projections) or VOP_EMBMEAN (table [nq * cb][out]) -> _tail.
    "int": small integers (embmean: multiples of nq, so that the mean is an integer); "real": N(0, 1) codebooks, 0.7 N / sqrt(dim)
    projections.  -> (tensors, 1, codes)"""
    rng = np.random.default_rng(seed)
    if kind == "rvq":
        prog = [[W.VOP_RVQ, nq, cb, dim, out, 0, 0, 0]]
        if data == "int":
            t = {"voc.op0.codebook": rng.integers(-3, 4, size=(nq, cb, dim)), "voc.op0.proj_sem": rng.integers(-2, 3, size=(out, dim)),
                 "voc.op0.proj_ac": rng.integers(-2, 3, size=(out, dim))}
        else:
            t = {"voc.op0.codebook": rng.standard_normal((nq, cb, dim)), "voc.op0.proj_sem": 0.7 * rng.standard_normal((out, dim)) / np.sqrt(dim),
                 "voc.op0.proj_ac": 0.7 * rng.standard_normal((out, dim)) / np.sqrt(dim)}
    else:
        prog = [[W.VOP_EMBMEAN, nq, cb, out, 0, 0, 0, 0]]
        tab = nq * rng.integers(-3, 4, size=(nq * cb, out)) if data == "int" else rng.standard_normal((nq * cb, out))
        t = {"voc.op0.embedding": tab}
    t = {n: np.ascontiguousarray(a, np.float32) for n, a in t.items()}
    for row, tens in C._tail(out):
        for n, a in tens.items():
            t[f"voc.op{len(prog)}.{n}"] = a
        prog.append(row)
    t["voc.program"] = np.asarray(prog, np.int32)
    return t, 1, front_codes(T, nq, cb, seed)


# ----------------------------------------------------------------------------------------------------------------------
# cases of the full-chunk ops (tests/test_gpu_voc_ops.py); make(name, data) -> (tensors, n_ops, codes [3][T][16])
# ----------------------------------------------------------------------------------------------------------------------
CASES = {}


def _case(name, **kw):
    assert name not in CASES, name
    CASES[name] = dict(kw, name=name, seed=7000 + 13 * len(CASES))


def norm_x(T, Cn, rng, special):
    """real_x with the norm's edge columns planted: `special` of ("const": every channel the integer 7 -- LayerNorm returns its
    bias bit for bit; "offset": 1000 + N(0, 1) -- a one-pass variance loses every digit here; "tiny": +-1e-20 -- eps dominates)"""
    x = real_x(T, Cn, rng)
    for col, what in enumerate(special):
        if what == "const":
            x[col] = 7.0
        elif what == "offset":
            x[col] = (1000.0 + rng.standard_normal(Cn)).astype(np.float32)
        else:
            x[col] = (1e-20 * rng.choice([-1.0, 1.0], size=Cn) * rng.uniform(0.5, 1.0, size=Cn)).astype(np.float32)
    return x


_n = 0
for _ci, _C in enumerate((8, 24, 40, 64, 520)):       # below the 16 channel lanes, uneven lanes, exactly 4 rounds, many rounds
    for _ti, _T in enumerate((1, 63, 64, 65, 130)):   # one column; a partly filled 64-column tile; one tile; one column into the next; three
        for _kind in (0, 1):
            _sp = ("const", "offset", "tiny") if _T >= 3 else (("const", "offset", "tiny")[_ci % 3],)   # (C = 64, T = 1: const)
            _case(f"norm{_kind}_C{_C}_T{_T}", family="norm", C=_C, T=_T, ops=[norm(_kind, (1000, 10000)[(_n // 2 + _n) % 2])], special=_sp,
                  data=("real",))
            _n += 1
_n = 0
for _K in (1, 2, 7):
    for _T in (1, 3, 6, 7, 255, 256, 257):            # L < K, L = K - 1, L = K; one thread short of / exactly / one past a 256-column block
        _case(f"dw_k{_K}_T{_T}", family="dwconv", C=(8, 24)[_n % 2], T=_T, ops=[dw(_K)], data=("int", "real"))
        _n += 1
_case("dw_k7_T3_nobias", family="dwconv", C=8, T=3, ops=[dw(7, bias=False)], data=("int", "real"))
_case("dw_k2_T257_nobias", family="dwconv", C=24, T=257, ops=[dw(2, bias=False)], data=("int", "real"))
for _kind in (0, 1):
    for _C in (8, 24):
        for _T in (1, 255, 257):
            _case(f"glu{_kind}_C{_C}_T{_T}", family="glu", C=2 * _C, T=_T, ops=[glu(_kind)], data=("real",))
_n = 0
for _NQ in (1, 2, 16):
    for _DIM in (8, 40):
        for _OUT in (8, 264):                         # 264: a second round of the 256 threads
            _case(f"rvq_q{_NQ}_d{_DIM}_o{_OUT}", family="rvq", nq=_NQ, dim=_DIM, out=_OUT, T=(1, 5)[_n % 2], cb=5, data=("int", "real"))
            _n += 1
_case("rvq_q2_d8_o8_T5", family="rvq", nq=2, dim=8, out=8, T=5, cb=5, data=("int", "real"))
_case("rvq_q16_d40_o264_T1", family="rvq", nq=16, dim=40, out=264, T=1, cb=5, data=("int", "real"))
for _NQ in (1, 2, 3, 16):
    for _T, _W in ((1, 24), (5, 8)):
        _case(f"emb_q{_NQ}_T{_T}", family="embmean", nq=_NQ, out=_W, T=_T, cb=6, data=("real",) if _NQ == 3 else ("int", "real"))
# attention through the table: the dispatch's tile-vs-wave rule at the 84 / 85-column LDS limit of D = 64, D = 128 (wave only),
# and 2-wide heads; windows 1, 4, 72 and one that never closes; both thetas a table can name
ATTN_VARIANT = {(2, 64, 84): "attn_tile", (2, 64, 85): "attn", (1, 128, 40): "attn", (3, 2, 9): None}
_n = 0
for (_H, _D, _T) in ATTN_VARIANT:
    for _w in (1, 4, 72, _T + 3):
        _case(f"attn_h{_H}_d{_D}_T{_T}_w{_w}", family="attn", C=3 * _H * _D, T=_T, ops=[attn(_H, _D, _w, (10000, 500)[_n % 2])], data=("real",),
              variant=ATTN_VARIANT[(_H, _D, _T)])
        _n += 1
    _case(f"attn_h{_H}_d{_D}_T{_T}_w4_theta", family="attn", C=3 * _H * _D, T=_T, ops=[attn(_H, _D, 4, 500)], data=("real",),
          variant=ATTN_VARIANT[(_H, _D, _T)])
    _case(f"attn_h{_H}_d{_D}_T{_T}_w72_theta", family="attn", C=3 * _H * _D, T=_T, ops=[attn(_H, _D, 72, 10000 if _n % 2 else 500)], data=("real",),
          variant=ATTN_VARIANT[(_H, _D, _T)])
# one ConvNeXt block: depthwise k7 (saves the residual: its input) -> LayerNorm -> 1-tap conv x 4 -> 1-tap conv (GELU, adds it back)
for _T in (5, 130):
    _case(f"convnext_T{_T}", family="convnext", C=8, T=_T, data=("real",),
          ops=[dw(7, RES_SAVE), norm(1, 1000), C.conv(32, 1, 1, 0), C.conv(8, 1, 1, GELU | RES_ADD)])

GLU_GATES = (0.0, 16.0, -16.0, 88.0, -88.0, 1e-40, -0.0, 8.0)     # +-88: the edge of __expf's range; 1e-40: an f32 subnormal


def make(name, data):
    """-> (tensors, n_ops, codes)"""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"] + (0 if data == "int" else 1))
    fam, T = c["family"], c["T"]
    if fam in ("rvq", "embmean"):
        return build_front_table(fam, c["nq"], c["cb"], T, data, c["seed"], dim=c.get("dim", 8), out=c["out"])
    if fam == "norm":
        x = norm_x(T, c["C"], rng, c["special"])
    elif fam == "glu":
        x = real_x(T, c["C"], rng)
        x[:, c["C"] // 2:] = rng.standard_normal((T, c["C"] // 2)).astype(np.float32)     # the up half
        x[0, :8] = GLU_GATES
    elif fam == "attn":
        x = rng.standard_normal((T, c["C"])).astype(np.float32)
    elif data == "int":
        x = rng.integers(-3, 4, size=(T, c["C"])).astype(np.float32)
    else:
        x = real_x(T, c["C"], rng)
    t, n_ops = build_table(c["ops"], x, data, c["seed"])
    return t, n_ops, perm_codes(T, c["seed"])


# ----------------------------------------------------------------------------------------------------------------------
# cases of the carry-state kernels (tests/test_gpu_voc_incr_ops.py): a stream of N columns per chunk row, pushed in pieces
# ----------------------------------------------------------------------------------------------------------------------
PUSH_PATTERNS = {"1": (1,), "7": (7,), "64": (64,), "mixed": (1, 2, 64, 5, 1, 40), "6": (6,)}
INCR_CASES = {}


def _icase(name, **kw):
    assert name not in INCR_CASES, name
    INCR_CASES[name] = dict(dict(N=300, C=16, x="real", arith=(0, 1), patterns=("1", "7", "64", "mixed")), **kw, name=name,
                            seed=9000 + 17 * len(INCR_CASES))


# dwconv K = 7 carries H = 6 columns: pushes of 1 (n < H), 6 (n = H), 7 and 64 (n > H); arithmetic 1 moves the history between two
# buffers by the stream's parity, arithmetic 0 moves it on in place
for _d in ("int", "real"):
    _icase(f"i_dw7_{_d}", ops=[dw(7)], data=_d, patterns=("1", "6", "7", "64", "mixed"))
# conv k = 3, dil = 2 (H = 4) and k = 7, dil = 9 (H = 54) at Cin = 16: voc_incr_prepend on the exact arithmetic,
# voc_incr_prepend_split (planes with the consumer's Snake / GELU, dst only for the RES_SAVE unit) on the split one
for _k, _dil in ((3, 2), (7, 9)):
    for _d in ("int", "real"):
        _icase(f"i_conv_k{_k}d{_dil}_snake_{_d}", ops=[C.conv(16, _k, _dil, SNAKE)], data=_d)
        _icase(f"i_conv_k{_k}d{_dil}_unit_{_d}", ops=[C.conv(16, _k, _dil, SNAKE | RES_SAVE), C.conv(16, 1, 1, SNAKE | RES_ADD)], data=_d)
    _icase(f"i_conv_k{_k}d{_dil}_gelu_real", ops=[C.conv(16, _k, _dil, GELU)], data="real")
    # integer GELU: inputs 0 or |x| >= 16, where GELU is ReLU exactly -- GELU(-16) = 0 != -16, so a residual (the f32 copy) or a
    # history that had the activation applied shows bit for bit
    _icase(f"i_conv_k{_k}d{_dil}_gelu_unit_int", ops=[C.conv(16, _k, _dil, GELU | RES_SAVE), C.conv(16, 1, 1, RES_ADD)], data="int", x="int16")
# attention: (heads, head_dim, window); D = 128 is the widest head, window 1 carries no history, 2-wide heads leave 63 lanes idle
for _H, _D, _w in ((2, 64, 72), (1, 128, 24), (3, 2, 4), (2, 16, 1)):
    # (arithmetic 1 changes no attention arithmetic: it moves the k | v history between two buffers by the stream's parity)
    _icase(f"i_attn_h{_H}_d{_D}_w{_w}", ops=[attn(_H, _D, _w)], data="real", C=3 * _H * _D, x="normal")
_icase("i_attn_long", ops=[attn(2, 64, 72)], data="real", C=3 * 2 * 64, x="normal", N=2200, arith=(0,), patterns=("64",))


def make_incr(name):
    """-> (tensors, n_ops, codes [3][N][16]): the table is loaded with chunk_tokens = 64 and driven N columns per stream"""
    c = INCR_CASES[name]
    rng = np.random.default_rng(c["seed"])
    N = c["N"]
    if c["x"] == "normal":
        x = rng.standard_normal((N, c["C"])).astype(np.float32)
    elif c["x"] == "int16":
        x = (16.0 * rng.integers(-2, 3, size=(N, c["C"]))).astype(np.float32)
    elif c["data"] == "int":
        x = rng.integers(-3, 4, size=(N, c["C"])).astype(np.float32)
    else:
        x = real_x(N, c["C"], rng)
    t, n_ops = build_table(c["ops"], x, c["data"], c["seed"])
    return t, n_ops, perm_codes(N, c["seed"])


def push_plan(N, pattern, stream):
    """the push sizes of one stream: stream 1 starts with a push of 3 (another phase: its later pushes share the others' launch
    group at other positions, its last one does not), a mixed pattern is also rotated by the stream's number"""
    pat = PUSH_PATTERNS[pattern]
    pat = pat[stream % len(pat):] + pat[:stream % len(pat)]
    sizes, left, i = ([3] if stream == 1 else []), N - (3 if stream == 1 else 0), 0
    while left > 0:
        n = min(pat[i % len(pat)], left)
        sizes.append(n)
        left -= n
        i += 1
    return sizes
