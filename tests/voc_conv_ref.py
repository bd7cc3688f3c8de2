"""One-op vocoder tables for the conv kernels, their float64 / int64 references and derived error bounds.

A case table is  [VOP_EMBMEAN nq=1, cb=T, width=Cin] -> the op(s) under test -> a tail that ends in one channel,
loaded with chunk_tokens = T and driven with codes[b][t][0] = perm_b[t]: the front then writes x[b][:, t] =
table[perm_b[t]] exactly, so the test chooses the input activation bit for bit and voc_debug_run(h, codes, B, n_ops)
returns the output of the op under test.  Every launch goes through voc_load / voc_run: pitches, zeroed pads, weight
packing and LDS sizes are the product's own.  (tests/test_gpu_voc_conv.py runs the tables, tests/test_voc_conv_reference.py
pins this file's float64 reference to oracle/voc_ref.py on every one of them.)

Only numpy and torch (torch for erf).

Error bounds (float64 reference y, device value yd; all per output element)
---------------------------------------------------------------------------
n = input channels x taps summed per output, U = 2^-24, S = sum |w| |h| + |bias| + |res| over the output's terms.

exact path   |yd - y| <= (2n + 4) U S + sum |w| d_act
    every product is rounded once (U each; the fp32 MFMA and fmaf round less often), every partial sum once
    (n - 1 adds, each at most U S whatever the order), bias, residual and the final store four more: (2n + 4) U S.
    d_act is the error of the staged activation h = act(x), below.

split path   add 3 * 2^-22 * sum |w| |h|  +  2^-36 * sum (|w| + |h|)
    an operand v is carried as hi = fp16(v), lo = fp16((v - hi) * 2048).  |v - hi| <= 2^-11 |v|, so |lo| <= |v| and, lo
    normal, |v - hi - lo / 2048| <= 2^-11 * 2^-11 |v| = 2^-22 |v|: two 22-bit operands give 2 * 2^-22 |w| |h| (+ 2^-44).
    The product lo_w lo_h / 2048^2 is dropped: <= 2^-22 |w| |h|.  Together 3 * 2^-22 |w| |h|.
    fp16-subnormal floor: below 2^-14 the spacing of fp16 is 2^-24, so rounding lo (or a hi below 2^-14, whose lo is then
    below 2^-14 too) costs at most 2^-25 absolute, i.e. 2^-25 / 2048 = 2^-36 on the operand: 2^-36 (|w| + |h|) per term.
    The three fp16 MFMAs accumulate exact products in f32 (the (2n + 4) U S above), acc + accx / 2048 is one more rounding
    of the same sum (inside the + 4).

chains       an input that already carries an error e_x reaches the conv as Lip(act) * e_x + d_act: Snake's Lipschitz
    constant is 1 + a * inv_beta (d/dx [x + ib sin^2(a x)] = 1 + a ib sin(2 a x)), exact GELU's 1.13, ELU's and the
    clamp's 1.  A residual adds its own error.  |h| in S is taken as |h| + that error.

d_act        Snake h = x + ib * sin^2(a x), a = expf(alpha), ib = 1 / (expf(beta) + 1e-9) computed in f32 at load:
    the argument a x is off by |a x| (2^-23 + 2^-24) (a one ulp off, the product rounded); |d sin^2 / d arg| <= 1;
    ib one ulp off and ib * s2 rounded: 3 U ib; the last add U |h|:
        d_snake = ib * (SIN2_ERR + 3 U |a x| + 3 U) + U |h|            (|a x| <= 16 is asserted)
    SIN2_ERR bounds what is not derivable, the device's fast sine squared (plus one add at |t| <= 17); GELU_ERR the
    device's 0.5 x (1 + erff(x / sqrt 2)) for |x| <= 8 (scaled by |x| / 8 beyond); ELU_ERR expm1f for x < 0.  They were
    measured with the activation probe of tests/test_gpu_voc_conv.py (a 1-tap identity conv returns the kernel's own
    activation) against float64 on a dense grid, doubled because the grid is finite and rounded up to a power of two;
    the probe test asserts measured <= constant on every run.
"""
from __future__ import annotations

import numpy as np
import torch

from qwen3_tts_axera_russian_amd import weights as W

U = 2.0 ** -24
# measured on an MI355X by test_activation_probe (max over the grid), constant = 2 x measured rounded up to a power of two
SIN2_MEASURED, SIN2_ERR = 1.780e-6, 2.0 ** -18   # |t + sin^2 t (device) - float64|, |t| <= 16, a = ib = 1
GELU_MEASURED, GELU_ERR = 4.450e-7, 2.0 ** -20   # |gelu (device) - float64|, |x| <= 8
ELU_MEASURED, ELU_ERR = 3.869e-8, 2.0 ** -23     # |elu (device) - float64|, |x| <= 8
GELU_LIP = 1.13

NO_SNAKE = (0.0, 100.0)     # alpha, beta (log scale): expf(100) = inf in f32, inv_beta = 0, Snake is the identity


# ----------------------------------------------------------------------------------------------------------------------
# plain references (numpy; the same code in float64 and int64)
# ----------------------------------------------------------------------------------------------------------------------
def causal_conv(h, w, dil):
    """h [B][Cin][L], w [Cout][Cin][K] (torch Conv1d) -> [B][Cout][L]: y[l] = sum_k w[k] h[l - (K - 1 - k) dil]"""
    B, _, L = h.shape
    K = w.shape[2]
    y = np.zeros((B, w.shape[0], L), h.dtype)
    for k in range(K):
        sh = (K - 1 - k) * dil
        if sh < L:
            y[:, :, sh:] += np.einsum("oc,bcl->bol", w[:, :, k], h[:, :, :L - sh])
    return y


def transposed_conv(h, w, s, lt, rt):
    """h [B][Cin][L], w [Cin][Cout][K] (torch ConvTranspose1d): input column l, tap k lands at l s + k; lt / rt trimmed"""
    B, _, L = h.shape
    K = w.shape[2]
    full = np.zeros((B, w.shape[1], (L - 1) * s + K), h.dtype)
    for k in range(K):
        full[:, :, k:k + (L - 1) * s + 1:s] += np.einsum("co,bcl->bol", w[:, :, k], h)
    return full[:, :, lt:full.shape[2] - rt]


def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


def gelu64(x):
    return 0.5 * x * (1.0 + _erf(x / np.sqrt(2.0)))


def snake64(x, alpha, beta):
    a = np.exp(np.asarray(alpha, np.float64))[None, :, None]
    ib = 1.0 / (np.exp(np.asarray(beta, np.float64))[None, :, None] + 1e-9)
    return x + ib * np.sin(a * x) ** 2


def elu64(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))


def _conv_like(row, h, w, xp=np):
    """the linear part of a VOP_CONV / VOP_CONVT row on h (any dtype)"""
    if int(row[0]) == W.VOP_CONV:
        return causal_conv(h, w, int(row[4]))
    return transposed_conv(h, w, int(row[4]), int(row[6]), int(row[7]))


def _front(tensors, codes, dtype):
    prog = np.asarray(tensors["voc.program"])
    assert int(prog[0][0]) == W.VOP_EMBMEAN and int(prog[0][1]) == 1
    tab = np.asarray(tensors["voc.op0.embedding"])
    x = tab[np.asarray(codes)[:, :, 0]]                       # [B][T][Cin]
    if dtype == np.int64:
        assert np.all(x == np.round(x))
    return np.ascontiguousarray(x.transpose(0, 2, 1)).astype(dtype)


def conv_int(tensors, i, row, x, res):
    """one VOP_CONV / VOP_CONVT row of an integer case on x (int64) -> (y, the sum of magnitudes each output accumulates)"""
    p = f"voc.op{i}."
    flags = int(row[5])
    if flags & W.VF_SNAKE:
        assert np.all(np.asarray(tensors[p + "alpha"]) == NO_SNAKE[0]) and np.all(np.asarray(tensors[p + "beta"]) == NO_SNAKE[1])
    h = x
    if flags & W.VF_GELU:
        assert np.all((h == 0) | (np.abs(h) >= 16))
        h = np.maximum(h, 0)
    w = np.asarray(tensors[p + "weight"])
    assert np.all(w == np.round(w))
    w = w.astype(np.int64)
    y = _conv_like(row, h, w)
    mag = _conv_like(row, np.abs(h), np.abs(w))
    if (p + "bias") in tensors:
        b = np.asarray(tensors[p + "bias"])
        assert np.all(b == np.round(b))
        y = y + b.astype(np.int64)[None, :, None]
        mag = mag + np.abs(b.astype(np.int64))[None, :, None]
    if flags & W.VF_RES_ADD:
        y = y + res
        mag = mag + np.abs(res)
    if flags & W.VF_CLAMP:
        y = np.clip(y, -1, 1)
    return y, mag


def reference_int(tensors, codes, n_ops):
    """int64 evaluation of an integer case: identity Snake (NO_SNAKE), GELU only on inputs that are 0 or |v| >= 16 (where
    exact GELU is ReLU to the last bit of f32 and of float64's 0.5 x (1 + erf): erf(16 / sqrt 2) = 1 - 6e-58).
    -> (y int64 [B][C][L], the largest sum of magnitudes any output accumulates: < 2^24 keeps f32 exact in any order)"""
    prog = np.asarray(tensors["voc.program"])
    x = _front(tensors, codes, np.int64)
    res, peak = None, 0
    for i in range(1, n_ops):
        row = prog[i]
        assert int(row[0]) in (W.VOP_CONV, W.VOP_CONVT)
        if int(row[5]) & W.VF_RES_SAVE:
            res = x
        x, mag = conv_int(tensors, i, row, x, res)
        peak = max(peak, int(mag.max()))
    return x, peak


def conv_f64(tensors, i, row, x, ex, res, eres, arith):
    """one VOP_CONV / VOP_CONVT row in float64 on x, whose device value is off by at most ex -> (y, the bound of the device's
    error on y: the module docstring's, arith "exact" / "split"; None: as "exact", the Snake range not asserted)"""
    p = f"voc.op{i}."
    flags = int(row[5])
    h, dh = x, ex
    if flags & W.VF_SNAKE:
        al, be = np.asarray(tensors[p + "alpha"], np.float64), np.asarray(tensors[p + "beta"], np.float64)
        a = np.exp(al)[None, :, None]
        ib = 1.0 / (np.exp(be)[None, :, None] + 1e-9)
        h = snake64(x, al, be)
        arg = np.abs(a * x) + a * ex
        live = ib > 2.0 ** -100          # (an inv_beta that is 0 in f32 takes the sine out of the result)
        assert arith is None or float((arg * live).max()) <= 16.0 * (1 + 2.0 ** -20), "Snake argument beyond the probed range"
        dh = (1.0 + a * ib) * ex + ib * (SIN2_ERR + 3 * U * arg + 3 * U) * live + U * np.abs(h)
    if flags & W.VF_GELU:
        g = gelu64(h)
        dh = GELU_LIP * dh + GELU_ERR * np.maximum(1.0, np.abs(h) / 8.0)
        h = g
    w = np.asarray(tensors[p + "weight"], np.float64)
    y = _conv_like(row, h, w)
    habs = np.abs(h) + dh
    Sw = _conv_like(row, habs, np.abs(w))
    S = Sw.copy()
    e = _conv_like(row, dh, np.abs(w))
    if (p + "bias") in tensors:
        b = np.asarray(tensors[p + "bias"], np.float64)[None, :, None]
        y = y + b
        S = S + np.abs(b)
    if flags & W.VF_RES_ADD:
        y = y + res
        S = S + np.abs(res) + eres
        e = e + eres
    taps = int(row[3]) if int(row[0]) == W.VOP_CONV else int(row[3]) // int(row[4])
    n = int(row[1]) * taps
    e = e + (2 * n + 4) * U * S
    if arith == "split" and int(row[1]) % 16 == 0:
        ones_h, ones_w = np.ones_like(habs), np.ones_like(w)
        e = e + 3 * 2.0 ** -22 * Sw + 2.0 ** -36 * (_conv_like(row, ones_h, np.abs(w)) + _conv_like(row, habs, ones_w))
    if flags & W.VF_CLAMP:
        y = np.clip(y, -1.0, 1.0)
    return y, e


def reference_f64(tensors, codes, n_ops, arith=None):
    """float64 evaluation -> y [B][C][L]; arith "exact" / "split": -> (y, bound [B][C][L]) with the module docstring's
    bound of the device's error, propagated through the chain"""
    prog = np.asarray(tensors["voc.program"])
    x = _front(tensors, codes, np.float64)
    ex = np.zeros_like(x)
    res = eres = None
    for i in range(1, n_ops):
        row = prog[i]
        assert int(row[0]) in (W.VOP_CONV, W.VOP_CONVT)
        if int(row[5]) & W.VF_RES_SAVE:
            res, eres = x, ex
        x, ex = conv_f64(tensors, i, row, x, ex, res, eres, arith)
    return (x, ex) if arith else x


# ----------------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------------
def conv(cout, k=1, dil=1, flags=0, bias=True, scale=1):
    return dict(op=W.VOP_CONV, cout=cout, k=k, p0=dil, flags=flags, lt=0, rt=0, bias=bias, scale=scale)


def convt(cout, s, J=1, trim="both", flags=0, bias=True):
    """ConvTranspose1d, k = J s.  trim: "both" (k - s at either end, the decoder family), "right" (0, k - s: strictly
    causal), or an explicit (lt, rt)"""
    k = J * s
    lt, rt = (k - s, k - s) if trim == "both" else (0, k - s) if trim == "right" else trim
    return dict(op=W.VOP_CONVT, cout=cout, k=k, p0=s, flags=flags, lt=lt, rt=rt, bias=bias, scale=1)


def _tail(C):
    """rows that bring C channels down to one with ops the loader takes at that width: a 1-tap conv where 8 | C, else
    attention with 2-wide heads (3 H D -> H D) and GLUs (2 C -> C)"""
    rows = []
    while C != 1:
        if C % 8 == 0:
            rows.append(([W.VOP_CONV, C, 1, 1, 1, 0, 0, 0], {"weight": np.ones((1, C, 1), np.float32)}))
            C = 1
        elif C % 6 == 0:
            rows.append(([W.VOP_ATTN, C, C // 3, C // 6, 2, 0, 4, 10000], {}))
            C //= 3
        elif C % 2 == 0:
            rows.append(([W.VOP_GLU, C, C // 2, 0, 0, 0, 0, 0], {}))
            C //= 2
        else:
            raise ValueError(f"no tail for {C} channels")
    return rows


def build_table(ops, T, cin, data, seed, big=None):
    """-> (tensors, n_ops of the op under test's output, codes int64 [3][T][16]).  data: "int" (x in [-3, 3], weights in
    [-2, 2] times the op's `scale`, integer bias, identity Snake) or "real" (as weights.make_synthetic_voc draws them:
    weights 0.7 N / sqrt(fan_in), bias 0.02 N, alpha, beta 0.3 N -- alpha capped at log 2 so that |a x| <= 16 --,
    x = 2.5 N clipped to |x| <= 8 with the extremes, zero and an fp16 subnormal planted).  big: a value planted at
    x[0][0] (the split path's overflow case)."""
    rng = np.random.default_rng(seed)
    if data == "int":
        x = rng.integers(-3, 4, size=(T, cin)).astype(np.float32)
    else:
        x = np.clip(2.5 * rng.standard_normal((T, cin)), -8.0, 8.0).astype(np.float32)
        flat = x.reshape(-1)
        for j, v in enumerate((8.0, -8.0, 0.0, 3e-6, -1e-40)):
            flat[(7 * j + 3) % flat.size] = v
    if big is not None:
        x[0, 0] = big
    prog = [[W.VOP_EMBMEAN, 1, T, cin, 0, 0, 0, 0]]
    t = {"voc.op0.embedding": x}
    C = cin
    for o in ops:
        i = len(prog)
        p = f"voc.op{i}."
        prog.append([o["op"], C, o["cout"], o["k"], o["p0"], o["flags"], o["lt"], o["rt"]])
        shp = (o["cout"], C, o["k"]) if o["op"] == W.VOP_CONV else (C, o["cout"], o["k"])
        taps = o["k"] if o["op"] == W.VOP_CONV else o["k"] // o["p0"]
        if data == "int":
            t[p + "weight"] = (o["scale"] * rng.integers(-2, 3, size=shp)).astype(np.float32)
            if o["bias"]:
                t[p + "bias"] = (o["scale"] * rng.integers(-4, 5, size=o["cout"])).astype(np.float32)
            if o["flags"] & W.VF_SNAKE:
                t[p + "alpha"] = np.full(C, NO_SNAKE[0], np.float32)
                t[p + "beta"] = np.full(C, NO_SNAKE[1], np.float32)
        else:
            gain = 0.25 if (o["flags"] & W.VF_RES_ADD) else 0.7
            t[p + "weight"] = (gain * rng.standard_normal(shp) / np.sqrt(C * taps)).astype(np.float32)
            if o["bias"]:
                t[p + "bias"] = (0.02 * rng.standard_normal(o["cout"])).astype(np.float32)
            if o["flags"] & W.VF_SNAKE:
                t[p + "alpha"] = np.minimum(0.3 * rng.standard_normal(C), np.log(2.0)).astype(np.float32)
                t[p + "beta"] = (0.3 * rng.standard_normal(C)).astype(np.float32)
        C = o["cout"]
    n_ops = len(prog)
    for row, tens in _tail(C):
        for n, a in tens.items():
            t[f"voc.op{len(prog)}.{n}"] = a
        prog.append(row)
    t["voc.program"] = np.asarray(prog, np.int32)
    codes = np.zeros((3, T, 16), np.int64)
    for b in range(3):
        codes[b, :, 0] = np.random.default_rng(seed + 1000 + b).permutation(T)
    return t, n_ops, codes


# ----------------------------------------------------------------------------------------------------------------------
# cases: one per instantiation the launchers can select (DESIGN.md "Vocoder conv kernels: per-variant tests"), each at an
# edge shape.  `exact` / `split`: the instantiation the op under test must reach in that arithmetic (None: not asserted
# there, only recorded).  Knobs: fill (voc_set_fill), narrow (voc_set_narrow_k1), fused (voc_set_fused_units).
# ----------------------------------------------------------------------------------------------------------------------
SNAKE, RES_ADD, RES_SAVE, CLAMP, GELU = W.VF_SNAKE, W.VF_RES_ADD, W.VF_RES_SAVE, W.VF_CLAMP, W.VF_GELU
T_EDGES = (1, 3, 4, 127, 128, 129, 131, 257)
CASES = {}


def _case(name, ops, T, cin, exact=None, split=None, fill=None, narrow=1, fused=1, fill_changes=False, data=("int", "real")):
    assert name not in CASES, name
    if T == 1 and any(o["op"] == W.VOP_CONVT and o["k"] - o["lt"] - o["rt"] <= 0 for o in ops):
        T = 3      # (one input column and both ends trimmed leaves no output: the loader refuses the table)
    CASES[name] = dict(name=name, ops=ops, T=T, cin=cin, exact=exact, split=split, fill=fill, narrow=narrow, fused=fused,
                       fill_changes=fill_changes, data=data, seed=1 + len(CASES))


def _exact_cases():
    n = 0
    # stride-1 convs: conv<MT,KT,KC,ct0,act3>.  Row counts per tile height (fill 0: the height follows divisibility of the
    # 32-row tile count; the default target takes 32-row tiles at these column counts): partial tiles and zeroed pad rows
    m_of = {1: (32, 8, 4, 12, 1), 2: (64, 40, 56), 3: (96, 192, 72), 4: (128, 160, 104)}
    fam = [(1, 8, 24), (1, 16, 48), (1, 32, 32), (2, 8, 8), (2, 16, 16), (2, 32, 96), (3, 8, 24), (3, 16, 32), (7, 8, 16)]
    for KT, KC, cin in fam:
        for MT in (1, 2, 3, 4):
            M = m_of[MT][n % len(m_of[MT])]
            T = T_EDGES[n % len(T_EDGES)]
            dil = (1, 3, 9)[n % 3] if KT > 1 else 1
            if KT == 7 and M == 1:
                M = 32     # (one row, 7 taps, no dilation is conv_out1's shape)
            flags = SNAKE if n % 2 else 0
            act = 3
            if (MT, KT, KC) == (4, 1, 16):
                act = 1 if flags else 0
            _case(f"x_mt{MT}_k{KT}_c{KC}", [conv(M, KT, dil, flags)], T, cin, exact=f"conv<{MT},{KT},{KC},ct0,act{act}>", fill=0)
            n += 1
    # the two further specialisations of the long 1 x 1 conv (no activation / Snake came out of the loop above; both and
    # GELU are named here so that none depends on the loop's parity)
    _case("x_mt4_k1_c16_plain", [conv(128, 1, 1, 0)], 129, 16, exact="conv<4,1,16,ct0,act0>", fill=0)
    _case("x_mt4_k1_c16_snake", [conv(160, 1, 1, SNAKE)], 131, 48, exact="conv<4,1,16,ct0,act1>", fill=0)
    _case("x_mt4_k1_c16_gelu", [conv(128, 1, 1, GELU)], 127, 16, exact="conv<4,1,16,ct0,act2>", fill=0, data=("real",))
    # default target: several 32-row tiles, the last one partial (M = 100 has no stride-1 table: see the transposed cases)
    _case("x_default_rows", [conv(104, 3, 3, SNAKE)], 131, 24, exact="conv<1,3,8,ct0,act3>", fill_changes=True)
    _case("x_default_k1", [conv(192, 1, 1, 0)], 257, 48, exact="conv<1,1,16,ct0,act3>", fill_changes=True)
    # transposed convs through the LDS slab: conv<MT,KT,KC,ct1,act3>, k = s (one tap) and k = 2 s (two), both trims
    ct_of = {1: ((1, 30), (8, 4), (1, 4)), 2: ((1, 33), (8, 8), (16, 4)), 3: ((8, 12), (24, 4), (16, 12)), 4: ((1, 100), (8, 16), (8, 20))}
    for KT, KC, cin in [(1, 8, 24), (1, 16, 16), (1, 32, 32), (2, 8, 8), (2, 16, 48), (2, 32, 96)]:
        for MT in (1, 2, 3, 4):
            cout, s = ct_of[MT][n % 3]
            T = T_EDGES[n % len(T_EDGES)]
            if s >= 30 and T > 131:
                T = 129
            _case(f"x_ct_mt{MT}_k{KT}_c{KC}", [convt(cout, s, KT, ("both", "right")[n % 2], SNAKE if n % 3 == 0 else 0)], T, cin,
                  exact=f"conv<{MT},{KT},{KC},ct1,act3>", fill=0)
            n += 1
    # k = 3 s: three taps, the strided epilogue of the plain kernel (trims: strictly causal, and one that cuts the left)
    _case("x_convt_j3_right", [convt(8, 4, 3, "right", SNAKE)], 129, 16, exact="conv<1,3,16,ct0,act3>", fill=0)
    _case("x_convt_j3_cut", [convt(1, 33, 3, (33, 66))], 131, 24, exact="conv<2,3,8,ct0,act3>", fill=0)
    # one output row: 7 taps without dilation is conv_out1 (exact arithmetic; the split path has its own form)
    for T in (1, 7, 8, 9, 2047, 2048, 2049):
        _case(f"x_out1_T{T}", [conv(1, 7, 1, SNAKE | CLAMP)], T, 16, exact="out1")
    _case("x_out1_plain", [conv(1, 7, 1, CLAMP)], 2049, 24, exact="out1", split="out1")
    _case("x_m1_general_k3", [conv(1, 3, 3, SNAKE)], 131, 24, exact="conv<1,3,8,ct0,act3>", split="conv<1,3,8,ct0,act3>")
    _case("x_m1_general_k7_dil", [conv(1, 7, 3, SNAKE)], 129, 16, exact="conv<1,7,8,ct0,act3>")
    # the residual unit k7(dil) + 1x1, fused and unfused
    for C, MT in ((96, 3), (192, 6)):
        for dil in (1, 3, 9):
            unit = [conv(C, 7, dil, SNAKE | RES_SAVE), conv(C, 1, 1, SNAKE | RES_ADD)]
            _case(f"x_resunit{MT}_d{dil}", unit, (131, 257, 127)[dil % 3], C, exact=f"resunit<{MT}>")
    _case("x_unit_unfused", [conv(96, 7, 3, SNAKE | RES_SAVE), conv(96, 1, 1, SNAKE | RES_ADD)], 131, 96,
          exact="conv<1,1,32,ct0,act3>", fused=0)


def _split_cases():
    n = 0
    cin_of = {3: (48, 96), 2: (32,), 1: (16,)}

    def T_of(NJ):
        e = T_EDGES + ((255, 256) if NJ == 2 else ())
        return e[n % len(e)]
    # one tap: split<1,KS,MW,NJ>
    for KS in (3, 2, 1):
        cin = cin_of[KS][n % len(cin_of[KS])]
        _case(f"s_k1_ks{KS}_mw3_nj1", [conv(96, 1, 1, SNAKE)], T_of(1), cin, split=f"snake_split+split<1,{KS},3,1>")
        n += 1
        _case(f"s_k1_ks{KS}_mw3_nj2", [conv(96, 1, 1, 0)], T_of(2), cin, split=f"snake_split+split<1,{KS},3,2>", narrow=0)
        n += 1
        M = (64, 160, 32)[KS - 1]
        _case(f"s_k1_ks{KS}_mw2_nj2", [conv(M, 1, 1, SNAKE)], T_of(2), cin,
              split=f"snake_split+split<1,{KS},2,2>" + ("/myfast" if M > 64 else ""))
        n += 1
    # two taps: a dilated k = 2 conv or a transposed conv with k = 2 s
    for KS, cin in ((2, 32), (1, 48)):
        _case(f"s_k2_ks{KS}_mw3_nj1", [convt(8, 12, 2, "both", SNAKE)], T_of(1), cin, split=f"snake_split+split<2,{KS},3,1>")
        n += 1
        _case(f"s_k2_ks{KS}_mw3_nj2", [conv(96, 2, 3, 0)], T_of(2), cin, split=f"snake_split+split<2,{KS},3,2>", narrow=0)
        n += 1
        _case(f"s_k2_ks{KS}_mw2_nj2", [convt(1, (30, 100)[KS - 1], 2, "right", SNAKE)], (131, 129)[KS - 1], cin,
              split=f"snake_split+split<2,{KS},2,2>" + ("/myfast" if KS == 2 else ""))
        n += 1
    # three taps
    _case("s_k3_ks2_mw2", [conv(64, 3, 9, SNAKE)], 257, 32, split="snake_split+split<3,2,2,2>")
    _case("s_k3_ks1_mw2", [conv(160, 3, 3, 0)], 255, 48, split="snake_split+split<3,1,2,2>/myfast")
    _case("s_k3_ks1_mw3", [convt(8, 12, 3, "right", SNAKE)], 131, 32, split="snake_split+split<3,1,3,2>")
    # seven taps
    _case("s_k7_mw2_nj1", [conv(64, 7, 9, SNAKE)], 129, 16, split="snake_split+split<7,1,2,1>")
    _case("s_k7_mw3_nj1", [conv(96, 7, 3, SNAKE)], 257, 96, split="snake_split+split<7,1,3,1>")
    _case("s_k7_mw2_nj2", [conv(128, 7, 1, 0)], 256, 32, split="snake_split+split<7,1,2,2>/myfast", narrow=0)
    _case("s_k7_mw3_nj2", [conv(96, 7, 9, SNAKE)], 255, 48, split="snake_split+split<7,1,3,2>", narrow=0)
    _case("s_m1_k7", [conv(1, 7, 1, SNAKE | CLAMP)], 257, 16, exact="out1", split="snake_split+split<7,1,2,1>")
    _case("s_m4_k1", [conv(4, 1, 1, 0)], 131, 16, split="snake_split+split<1,1,2,2>")
    # 192 rows: 64-row tiles under the default target, 96-row tiles once the target is 0 (both walk row tiles fastest)
    _case("s_m192_default", [conv(192, 7, 1, SNAKE)], 131, 96, split="snake_split+split<7,1,2,1>/myfast", fill_changes=True)
    _case("s_m192_fill0", [conv(192, 1, 1, SNAKE)], 257, 48, split="snake_split+split<1,3,3,1>/myfast", fill=0)
    # weights beyond 2 MiB: columns fastest, chunk next, row tile slowest
    _case("s_big_weights", [conv(896, 7, 1, SNAKE)], 131, 96, split="snake_split+split<7,1,2,1>", data=("int",))
    # chains: the second conv reads planes the first conv's epilogue wrote (with the second's Snake) -- no separate pass;
    # a GELU consumer takes the separate pass; the residual unit on the split path (the 1 x 1 adds the saved input)
    _case("s_chain_planes", [conv(32, 3, 3, SNAKE), conv(64, 1, 1, SNAKE)], 131, 16, exact="conv<1,1,32,ct0,act3>", split="split<1,2,2,2>")
    _case("s_chain_planes_k7", [conv(96, 1, 1, 0), conv(96, 7, 9, SNAKE)], 257, 32, split="split<7,1,3,1>")
    _case("s_chain_gelu", [conv(32, 1, 1, 0, scale=16), conv(64, 1, 1, GELU)], 129, 16, exact="conv<1,1,32,ct0,act3>",
          split="snake_split+split<1,2,2,2>")
    _case("s_unit", [conv(96, 7, 3, SNAKE | RES_SAVE), conv(96, 1, 1, SNAKE | RES_ADD)], 257, 96, exact="resunit<3>", split="split<1,3,3,1>")


_exact_cases()
_split_cases()

# Every instantiation the launchers can select (voc_launch_conv, launch_conv_mt, launch_conv_t, launch_resunit,
# launch_conv_split, launch_conv_split_m; "/myfast" is the tile order, not an instantiation).  ELU (act4) comes from the
# encoder cases of tests/test_gpu_voc_conv.py.  DESIGN.md names what the rules can never select.
REACHABLE = set()
for _mt in (1, 2, 3, 4):
    for _kt, _kc in ((1, 8), (1, 16), (1, 32), (2, 8), (2, 16), (2, 32), (3, 8), (3, 16), (7, 8)):
        REACHABLE.add(f"conv<{_mt},{_kt},{_kc},ct0,act3>")
    for _kt, _kc in ((1, 8), (1, 16), (1, 32), (2, 8), (2, 16), (2, 32)):
        REACHABLE.add(f"conv<{_mt},{_kt},{_kc},ct1,act3>")
    for _kt in (1, 3):
        REACHABLE.add(f"conv<{_mt},{_kt},16,ct0,act4>")
REACHABLE.discard("conv<4,1,16,ct0,act3>")      # the long 1 x 1 conv is compiled per activation instead
REACHABLE |= {"conv<4,1,16,ct0,act0>", "conv<4,1,16,ct0,act1>", "conv<4,1,16,ct0,act2>", "out1", "resunit<3>", "resunit<6>", "snake_split"}
for _ks in (1, 2, 3):
    REACHABLE |= {f"split<1,{_ks},3,1>", f"split<1,{_ks},3,2>", f"split<1,{_ks},2,2>"}
for _ks in (1, 2):
    REACHABLE |= {f"split<2,{_ks},3,1>", f"split<2,{_ks},3,2>", f"split<2,{_ks},2,2>"}
REACHABLE |= {"split<3,2,2,2>", "split<3,1,2,2>", "split<3,1,3,2>", "split<7,1,2,1>", "split<7,1,3,1>", "split<7,1,2,2>", "split<7,1,3,2>"}


# ----------------------------------------------------------------------------------------------------------------------
# encoder tables (the ELU instantiations): CONV_IN k = 1 -> one ELU conv -> the quantiser
# ----------------------------------------------------------------------------------------------------------------------
def build_enc_table(C, M, k, dil, data, seed, res=False):
    """x[c][l] = w_in[c] pcm[l] (+ b_in[c]) is exact in f32: "int": w_in in {1, 2, 3}, b_in in {0, 1, 2}, pcm in {0, 1, 2} -- x >= 0,
    where ELU is the identity; "real": w_in = +-2^j, no bias, pcm = 2 N clipped to +-4.  -> (tensors, pcm f32 [3][n] maker)"""
    rng = np.random.default_rng(seed)
    prog = [[W.EOP_CONV_IN, 1, C, 1, 0, 0, 0, 0], [W.EOP_CONV, C, M, k, dil, W.EF_ELU, 0, 0],
            [W.EOP_RVQ, M, 1, 1, M // 2, 0, 1, 0]]
    t = {"enc.program": np.asarray(prog, np.int32)}
    if data == "int":
        t["enc.op0.weight"] = rng.integers(1, 4, size=(C, 1, 1)).astype(np.float32)
        t["enc.op0.bias"] = rng.integers(0, 3, size=C).astype(np.float32)
        t["enc.op1.weight"] = rng.integers(-2, 3, size=(M, C, k)).astype(np.float32)
        t["enc.op1.bias"] = rng.integers(-4, 5, size=M).astype(np.float32)
    else:
        t["enc.op0.weight"] = (rng.choice([-1.0, 1.0], size=(C, 1, 1)) * 2.0 ** rng.integers(-2, 2, size=(C, 1, 1))).astype(np.float32)
        t["enc.op1.weight"] = (1.2 * rng.standard_normal((M, C, k)) / np.sqrt(C * k)).astype(np.float32)
        t["enc.op1.bias"] = (0.02 * rng.standard_normal(M)).astype(np.float32)
    t["enc.op2.codebook"] = np.zeros((1, 1, M // 2), np.float32)
    return t


def enc_pcm(n, data, seed):
    rng = np.random.default_rng(seed + 77)
    if data == "int":
        return rng.integers(0, 3, size=(3, n)).astype(np.float32)
    return np.clip(2.0 * rng.standard_normal((3, n)), -4.0, 4.0).astype(np.float32)


def enc_reference_f64(t, pcm, bound=False):
    """float64 evaluation of build_enc_table's ELU conv on clips pcm [B][n] -> y [B][M][n] (, bound)"""
    w0 = np.asarray(t["enc.op0.weight"], np.float64)[:, 0, 0]
    x = w0[None, :, None] * np.asarray(pcm, np.float64)[:, None, :]
    if "enc.op0.bias" in t:
        x = x + np.asarray(t["enc.op0.bias"], np.float64)[None, :, None]
    row = np.asarray(t["enc.program"])[1]
    w = np.asarray(t["enc.op1.weight"], np.float64)
    h = elu64(x)
    b = np.asarray(t["enc.op1.bias"], np.float64)[None, :, None]
    y = causal_conv(h, w, int(row[4])) + b
    if not bound:
        return y
    dh = ELU_ERR * (x < 0)
    S = causal_conv(np.abs(h) + dh, np.abs(w), int(row[4])) + np.abs(b)
    n = int(row[1]) * int(row[3])
    return y, (2 * n + 4) * U * S + causal_conv(dh, np.abs(w), int(row[4]))


# (MT, KT) -> (C, M, dil, n samples); fill 0 (default target: 32-row tiles at these lengths)
ENC_CASES = {}
for _i, (_mt, _M) in enumerate(((1, 8), (2, 40), (3, 96), (4, 160))):
    for _kt in (1, 3):
        ENC_CASES[f"e_mt{_mt}_k{_kt}"] = dict(C=(16, 48)[_i % 2], M=_M, k=_kt, dil=(1, 2, 3, 9)[_i] if _kt == 3 else 1,
                                              n=(131, 257, 129, 3)[_i], variant=f"conv<{_mt},{_kt},16,ct0,act4>", seed=500 + 2 * _i + _kt)
