"""Every linear / GEMM kernel instantiation behind launch_linear against the float64 restatement of its contract
(tests/linear_ref.py), one launch at a time through the hook q3t_linear_case (csrc/q3_test_api.hip).

Coverage is part of the assertion: VARIANTS below is the literal list of instantiations (a CPU test compares it with the
Q3_LIN_MT lines and the launch_linear_narrow_t / launch_gemm_t calls of csrc/q3_linear.hip), every GPU case asserts the
name launch_linear reports for the kernel it picked, and a final check asserts that every entry was observed.

Tolerances are derived, never tuned.  fp16 x fp16 products are exact in f32, so against the float64 product of the fp16
operands the kernel read (B = sum_k |x_k| |w_k|, u = 2^-24):
  * accumulator: |acc - ref| <= K u B, element by element (K f32 additions in any order);
  * norm prologue: post = 16 / sqrt(sum(ssq) / K + eps) from the DEVICE's partials to 8 u relative (64 additions, divide,
    sqrt, two multiplies), one more u for the final multiply;
  * residual epilogue: h to the accumulator bound plus half an f32 ulp of the result; the new partials to 2^-20 relative
    of the float64 sums of squares of the device's own h; xh bit-equal to pre_scaled(device h, gamma);
  * SwiGLU: the bounds of g and u propagated through silu(g) * u (|silu'| <= 1.1), 2^-20 relative for the hardware exp
    and reciprocal, one fp16 ulp of the reference.
Small-integer operands make every product and sum exact: those cases have no tolerance at all on the accumulators.
The hook fills every output with a NaN sentinel over its padded extent and fails (-3) if anything outside rows
[m_begin, M) x columns [0, N) changed; padding rows of the inputs hold finite poison.

ERR records, per variant, the largest measured error as a multiple of its bound (printed by the last test; the table in
DESIGN.md 8 is a copy of one run)."""
import contextlib
import functools
import itertools
import os
import re

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import linear_ref as L

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "qwen3_tts_axera_russian_amd", "csrc", "q3_linear.hip")
PRO = {"F16": 0, "NORM": 1}
EPI = {"STORE": 0, "RESID": 1, "SWIGLU": 2}
U = L.U24

# ---- the literal table: (NB16, KBW, NW, PRO, EPI) lines of linear_kernel, each for MT16 in 1, 2, 4 and both load kinds ----
LINEAR_LINES = [
    (1, 8, 4, "NORM", "STORE"), (1, 4, 8, "NORM", "STORE"), (2, 8, 4, "NORM", "SWIGLU"), (2, 4, 8, "NORM", "SWIGLU"),
    (1, 8, 4, "F16", "STORE"), (2, 4, 8, "NORM", "STORE"), (2, 4, 8, "F16", "STORE"), (1, 4, 8, "F16", "STORE"),
    (1, 8, 8, "F16", "RESID"), (1, 4, 16, "F16", "RESID"), (1, 16, 4, "F16", "RESID"),
    (1, 6, 16, "F16", "RESID"), (1, 12, 8, "F16", "RESID"),
]
NARROW = [(16, 4), (12, 8)]                       # linear_narrow_kernel<KBW, NW>
GEMM_TILES = [                                    # launch_gemm_t<BM, BN, PRO, EPI>
    (128, 128, "NORM", "STORE"), (128, 192, "NORM", "SWIGLU"), (128, 128, "NORM", "SWIGLU"), (64, 64, "F16", "RESID"),
    (128, 128, "F16", "RESID"), (64, 64, "F16", "STORE"), (128, 128, "F16", "STORE"),
]


def linear_name(nb16, mt16, kbw, nw, pro, epi, nt):
    return f"linear<{nb16},{mt16},{kbw},{nw},{pro},{epi},{'nt' if nt else 't'}>"


def narrow_name(kbw, nw, nt):
    return f"narrow<{kbw},{nw},{'nt' if nt else 't'}>"


def gemm_name(bm, bn, pro, epi, glds):
    if glds:   # ring depth and k-blocks per stage as launch_gemm_t derives them from the tile
        return f"gemm_glds<{bm},{bn},{3 if bm + bn > 256 else 4},{pro},{epi},{4 if bm + bn <= 128 else 2}>"
    return f"gemm<{bm},{bn},{1024 // (bm + bn)},{pro},{epi}>"


def all_variants():
    v = [linear_name(nb, mt, kbw, nw, p, e, nt) for nb, kbw, nw, p, e in LINEAR_LINES for mt in (1, 2, 4) for nt in (0, 1)]
    v += [narrow_name(kbw, nw, nt) for kbw, nw in NARROW for nt in (0, 1)]
    # the 128 x 192 tile exists as an LDS-DMA ring only
    v += [gemm_name(bm, bn, p, e, g) for bm, bn, p, e in GEMM_TILES for g in (1, 0) if g or bm + bn <= 256]
    return v


VARIANTS = all_variants()
SEEN = set()
ERR = {}          # variant -> largest error / bound


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the table is the source's table; the bound tells a dropped k-block from round-off
# ---------------------------------------------------------------------------------------------------------------------
def test_variant_table_matches_the_source():
    src = open(KERNELS).read()
    src = re.sub(r"//[^\n]*", "", src)
    body = src[src.index("int launch_linear(hipStream_t s, const LinArgs& a, int pro, int epi)"):]
    lines = [(int(a), int(b), int(c), p, e) for a, b, c, p, e in
             re.findall(r"Q3_LIN_MT\((\d+), (\d+), (\d+), PRO_(\w+), EPI_(\w+)\)", body)]
    assert sorted(lines) == sorted(LINEAR_LINES) and len(set(lines)) == len(lines)
    mt = re.search(r"#define Q3_LIN_MT\(.*?\n\n", src, re.S).group(0)
    assert sorted(int(m) for m in re.findall(r"Q3_LIN_CASE\(NB16_, (\d+),", mt)) == [1, 2, 4]
    assert "launch_linear_nt<NB16, MT16, KBW, NW, PRO, EPI, true>" in src and \
        "launch_linear_nt<NB16, MT16, KBW, NW, PRO, EPI, false>" in src
    narrow = [(int(a), int(b)) for a, b in re.findall(r"launch_linear_narrow_t<(\d+), (\d+)>\(s, a\)", src)]
    assert sorted(narrow) == sorted(NARROW)
    tiles = [(int(a), int(b), p, e) for a, b, p, e in
             re.findall(r"launch_gemm_t<(\d+), (\d+), PRO_(\w+), EPI_(\w+)>\(s, a\)", src)]
    assert sorted(tiles) == sorted(GEMM_TILES) and len(set(tiles)) == len(tiles)
    assert len(VARIANTS) == len(set(VARIANTS)) == 13 * 6 + 4 + 13
    covered = {c[0] for c in LINEAR_CASES} | {c[0] for c in NARROW_CASES} | {c[0] for c in GEMM_CASES}
    assert covered == set(VARIANTS), sorted(set(VARIANTS) ^ covered)


@pytest.mark.parametrize("K,sx", [(1024, 1.0), (2048, 1.0), (3072, 1.0), (1024, 3.0 / 16)])
def test_the_bound_separates_a_dropped_k_block_from_round_off(K, sx):
    """At the operand scales of the random cases (x ~ N(0, sx), W ~ N(0, 0.05)) dropping one 32-wide k-block moves a
    typical output by more than ten times the accumulator bound K 2^-24 sum |x w|."""
    rng = np.random.default_rng(K)
    x = (sx * rng.standard_normal((16, K))).astype(np.float16)
    W = (0.05 * rng.standard_normal((256, K))).astype(np.float16)
    ref, ab = L.linear(x, W)
    drop, _ = L.linear(x[:, 32:], W[:, 32:])
    ratio = np.abs(drop - ref) / L.acc_bound(ab, K)
    assert np.sqrt((ratio ** 2).mean()) > 10 and np.median(ratio) > 6, (np.sqrt((ratio ** 2).mean()), np.median(ratio))
    assert (ratio > 1).mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------------
# the hook
# ---------------------------------------------------------------------------------------------------------------------
def _u16(a):
    return None if a is None else a.view(np.uint16).ctypes.data_as(hiplib.u16p)


def _f32(a):
    return None if a is None else hiplib.fptr(a)


@contextlib.contextmanager
def knobs(lib, tuning=(), split=None, narrow8=None, wide=None, min_rows=None, glds=None):
    """Process-wide dispatch knobs for one case; every one of them is put back whatever happens."""
    try:
        for K, mt16, kbw in tuning:
            assert lib.q3t_set_linear_tuning(K, mt16, kbw) == 0
        if split is not None:
            lib.q3t_set_linear_split_rows(split)
        if narrow8 is not None:
            lib.q3t_set_linear_narrow8(narrow8)
        if wide is not None:
            lib.q3t_set_linear_wide_tiles(wide)
        if min_rows is not None:
            lib.q3t_set_gemm_min_rows(min_rows)
        if glds is not None:
            lib.q3t_set_gemm_glds(glds)
        yield
    finally:
        lib.q3t_reset_linear_knobs()


def call(lib, M, m_begin, N, K, W, gateup, pro, epi, nt, eps=1e-6, ldy=None, x16=None, h=None, gamma=None,
         gamma_next=None, h_io=None, want_xh=None):
    """-> (rc, variant, outputs).  Host arrays cover rows [0, M); rows below m_begin keep the fill they get here."""
    ldy = N if ldy is None else ldy
    o = {}
    if pro == 1:
        o["pro_h"] = np.zeros((M, K), np.float32)
        o["pro_ssq"] = np.zeros((M, K // 16), np.float32)
        o["pro_xh"] = np.zeros((M, K), np.float16)
    if epi == 0:
        o["y"] = np.full((M, ldy), np.nan, np.float32)
    elif epi == 1:
        o["h"] = np.ascontiguousarray(h_io, np.float32).copy()
        o["ssq"] = np.full((M, N // 16), np.nan, np.float32)
        if (gamma_next is not None) if want_xh is None else want_xh:
            o["xh"] = np.full((M, N), np.nan, np.float16)
    else:
        o["act"] = np.full((M, N // 2), np.nan, np.float16)
    rc = lib.q3t_linear_case(M, m_begin, N, K, _u16(W), gateup, pro, epi, nt, eps, ldy, _u16(x16), _f32(h), _f32(gamma),
                             _f32(gamma_next), _f32(o.get("pro_h")), _f32(o.get("pro_ssq")), _u16(o.get("pro_xh")),
                             _f32(o.get("y")), _f32(o.get("h")), _f32(o.get("ssq")), _u16(o.get("xh")), _u16(o.get("act")))
    return rc, lib.q3t_last_linear_variant().decode(), o


@functools.lru_cache(maxsize=6)
def weights(N, K, mode, seed):
    rng = np.random.default_rng(seed)
    if mode == "exact":
        return rng.integers(-3, 4, size=(N, K)).astype(np.float16)
    return ((10.0 if mode == "sat" else 0.05) * rng.standard_normal((N, K))).astype(np.float16)


def record(variant, err, tol, what):
    """err <= tol element by element (tol == 0: equality); the worst ratio goes into ERR."""
    err, tol = np.asarray(err, np.float64), np.asarray(tol, np.float64)
    assert np.isfinite(err).all(), f"{variant}: {what}: non-finite error"
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    ERR[variant] = max(ERR.get(variant, 0.0), worst)
    if worst > 1.0:
        bad = np.argwhere(ratio > 1.0)
        i = tuple(bad[0])
        raise AssertionError(f"{variant}: {what}: {len(bad)} of {ratio.size} values beyond the bound, worst {worst:.3g} x; "
                             f"first at {i}: error {err[i]:.6g}, bound {tol[i]:.6g}")


def run_case(lib, variant, M, m_begin, N, K, pro, epi, nt, mode, eps=1e-6, ldy=None, seed=0):
    """One launch, graded.  mode: exact (small integers), random, eps (tiny / zero rows), sat (values beyond fp16)."""
    pro_i, epi_i = PRO[pro], EPI[epi]
    rng = np.random.default_rng(seed * 7919 + M * 31 + m_begin + N + K)
    gateup = 1 if epi == "SWIGLU" else 0
    W = weights(N, K, "sat" if (mode == "sat" and epi == "SWIGLU") else "exact" if mode == "exact" else "random", seed)
    R = slice(m_begin, M)
    kw = {}
    if pro == "F16":
        if mode == "exact":
            x16 = rng.integers(-2, 3, size=(M, K)).astype(np.float16)
        else:
            x16 = rng.standard_normal((M, K)).astype(np.float16)
        kw["x16"] = x16
    else:
        if mode == "exact":      # xh = (h * gamma) / 16 is a small integer
            h = (16.0 * rng.integers(-2, 3, size=(M, K))).astype(np.float32)
            gamma = rng.choice([1.0, 2.0], size=K).astype(np.float32)
        elif mode == "eps":      # rows of rms ~1e-4 (xh in the fp16 subnormals), all-zero rows, ordinary rows
            scale = np.array([1e-4, 0.0, 3.0])[np.arange(M) % 3][:, None]
            h = (scale * rng.standard_normal((M, K))).astype(np.float32)
            gamma = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        else:
            h = (3.0 * rng.standard_normal((M, K))).astype(np.float32)
            gamma = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        kw.update(h=h, gamma=gamma)
    if epi == "RESID":
        if mode == "exact":
            h0 = rng.integers(-5, 8, size=(M, N)).astype(np.float32)
            gn = rng.choice([1.0, 2.0, 16.0], size=N).astype(np.float32)
        elif mode == "sat":      # |h * gamma| / 16 far beyond 65504 on every eighth column
            h0 = rng.standard_normal((M, N)).astype(np.float32)
            h0[:, ::8] = (3e6 * np.sign(h0[:, ::8])).astype(np.float32)
            gn = np.ones(N, np.float32)
        else:
            h0 = rng.standard_normal((M, N)).astype(np.float32)
            gn = (1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32)
        kw.update(h_io=h0, gamma_next=gn)
    rc, got_variant, o = call(lib, M, m_begin, N, K, W, gateup, pro_i, epi_i, nt, eps=eps, ldy=ldy, **kw)
    assert rc == 0, f"{variant} M={M} m_begin={m_begin} N={N} K={K}: hook returned {rc} (ran {got_variant!r})"
    assert got_variant == variant, f"M={M} m_begin={m_begin} N={N} K={K}: launch_linear picked {got_variant}, the case was written for {variant}"
    SEEN.add(got_variant)
    what = f"{mode} M={M} m_begin={m_begin} N={N} K={K}"

    # ---- the producer of the norm prologue, on its own; the GEMM is graded from what it left on the device ----
    post = None
    if pro == "NORM":
        np.testing.assert_array_equal(o["pro_h"].view(np.uint32), h.view(np.uint32), err_msg="ssq_rows: h in fragment order")
        np.testing.assert_array_equal(o["pro_xh"].view(np.uint16), L.pre_scaled(h, gamma).view(np.uint16), err_msg="ssq_rows: xh")
        p64 = L.ssq_partials(h)
        assert (np.abs(o["pro_ssq"] - p64) <= 2.0 ** -20 * p64).all(), "ssq_rows: partials"
        if mode == "eps":
            tiny = np.abs(o["pro_xh"][0::3].astype(np.float32))
            assert ((tiny > 0) & (tiny < 2.0 ** -14)).mean() > 0.5, "the tiny rows do not reach the fp16 subnormals"
        x16 = o["pro_xh"]
        post = L.post_scale(o["pro_ssq"], K, eps)[R]
    acc, ab = L.linear(x16[R], W)
    accb = np.zeros_like(ab) if mode == "exact" else L.acc_bound(ab, K)
    if mode == "exact":
        assert np.abs(acc).max() < 2 ** 24 and ab.max() < 2 ** 24      # every partial sum is an exact f32 integer

    if epi == "STORE":
        got = o["y"][R, :N].astype(np.float64)
        ref = L.store(acc, post)
        if pro == "F16":
            if mode == "exact":
                np.testing.assert_array_equal(got, ref, err_msg=f"{variant}: {what}")
            record(variant, np.abs(got - ref), accb, what)
        else:
            record(variant, np.abs(got - ref), (accb * post[:, None] + 9 * U * np.abs(ref)) * (1 + 2.0 ** -20), what)
    elif epi == "RESID":
        got = o["h"][R].astype(np.float64)
        ref = L.resid(h0[R], acc)
        if mode == "exact":
            np.testing.assert_array_equal(got, ref, err_msg=f"{variant}: {what}")
        record(variant, np.abs(got - ref), accb + 0.5 * L.ulp32(got), what + " h")
        np.testing.assert_array_equal(o["h"][:m_begin].view(np.uint32), h0[:m_begin].view(np.uint32))
        s64 = L.ssq_partials(got)
        if mode == "exact" and s64.max() <= 2 ** 24:
            np.testing.assert_array_equal(o["ssq"][R].astype(np.float64), s64, err_msg=f"{variant}: {what} ssq")
        assert (np.abs(o["ssq"][R] - s64) <= 2.0 ** -20 * s64).all(), f"{variant}: {what}: ssq_out"
        want_xh = L.pre_scaled(o["h"][R], gn)
        np.testing.assert_array_equal(o["xh"][R].view(np.uint16), want_xh.view(np.uint16), err_msg=f"{variant}: {what} xh_out")
        if mode == "sat":
            big = np.abs(h0[R].astype(np.float64)) > 1e6
            assert big.any() and (np.abs(o["xh"][R][big].astype(np.float32)) == 65504.0).all(), "xh_out does not saturate"
            assert np.isfinite(o["h"][R]).all() and np.abs(o["h"][R][big]).min() > 2e6       # h itself stays f32
    else:
        want, g, u = L.swiglu(acc, post)
        half = N // 2
        if pro == "NORM":
            bg = (accb[:, :half] * post[:, None] + 9 * U * np.abs(g)) * (1 + 2.0 ** -20)
            bu = (accb[:, half:] * post[:, None] + 9 * U * np.abs(u)) * (1 + 2.0 ** -20)
        else:
            bg, bu = accb[:, :half], accb[:, half:]
        clipped = np.clip(want, -L.F16_MAX, L.F16_MAX)
        tol = 1.1 * bg * (np.abs(u) + bu) + np.abs(L.silu(g)) * bu + 2.0 ** -20 * np.abs(want) + L.ulp16(clipped)
        got = o["act"][R].astype(np.float64)
        assert np.isfinite(got).all(), f"{variant}: {what}: non-finite SwiGLU output"
        record(variant, np.abs(got - clipped), tol, what)
        if mode == "sat":
            over = np.abs(want) > 70000.0
            assert over.mean() > 0.001 and (np.abs(got[over]) == L.F16_MAX).all(), "SwiGLU does not saturate"
    return o


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
BIG = 1 << 20      # set_gemm_min_rows: keeps the weight-streaming kernel at any row count


def shapes_linear(K, pro, epi):
    """(N, K) the product launches through this kind of kernel (head vocabularies: q3_common.h talker 3072, cp 2048)."""
    if epi == "SWIGLU":
        return [6144]
    if epi == "RESID":
        return [1024, 2048] if K == 2048 else [1024]        # o, text fc1 / fc2; down
    return [4096, 3072, 2048] if pro == "NORM" else [3072, 2048, 4096]


def linear_cases():
    out = []
    for (nb, kbw, nw, pro, epi), mt, nt in itertools.product(LINEAR_LINES, (1, 2, 4), (0, 1)):
        K = kbw * nw * 32
        name = linear_name(nb, mt, kbw, nw, pro, epi, nt)
        wide = nb == 2 and epi == "STORE"
        base = dict(tuning=((K, mt, kbw),), narrow8=0, wide=1 if wide else 0)
        # (m_begin, rows, extra knobs)
        if mt == 1:
            rows = [] if wide else [(0, r, dict(split=1)) for r in (1, 8, 9, 15, 16)] + [(16, 9, {}), (48, 15, {})]
            rows += [(0, r, dict(split=2)) for r in (17, 31, 32)] + [(16, 21, dict(split=2))]
        elif mt == 2:
            rows = [(0, r, dict(split=0)) for r in (17, 31, 32)] + [(16, 25, dict(split=0)), (48, 19, dict(split=0))]
        else:
            rows = [(0, r, {}) for r in (33, 48, 63, 64)] + [(16, 45, {}), (0, 129, dict(min_rows=BIG)),
                                                            (0, 200, dict(min_rows=BIG)), (48, 150, dict(min_rows=BIG))]
        Ns = shapes_linear(K, pro, epi)
        for i, (mb, r, extra) in enumerate(rows):
            for j, mode in enumerate(("exact", "random")):
                N = Ns[(i + j) % len(Ns)]
                ldy = N + 96 if (epi == "STORE" and mb == 16) else None
                out.append((name, mb + r, mb, N, K, pro, epi, nt, mode, {**base, **extra}, ldy))
        # edges, once per variant
        r, extra = {1: (21, dict(split=2)) if wide else (15, dict(split=1)), 2: (21, dict(split=0)), 4: (45, {})}[mt]
        if pro == "NORM":
            for eps in (1e-6, 1e-3):
                out.append((name, r, 0, Ns[0], K, pro, epi, nt, "eps", {**base, **extra}, eps))
        if epi in ("RESID", "SWIGLU"):
            out.append((name, r, 0, Ns[0], K, pro, epi, nt, "sat", {**base, **extra}, None))
    return out


def narrow_cases():
    out = []
    for (kbw, nw), nt in itertools.product(NARROW, (0, 1)):
        K, name = kbw * nw * 32, narrow_name(kbw, nw, nt)
        rows = [(0, r) for r in (1, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64)] + [(16, 9), (48, 13), (16, 43)]
        for i, (mb, r) in enumerate(rows):
            out.append((name, mb + r, mb, 1024, K, "F16", "RESID", nt, ("exact", "random")[i % 2], {}, None))
            if r in (8, 17, 64) or mb:
                out.append((name, mb + r, mb, 1024, K, "F16", "RESID", nt, ("random", "exact")[i % 2], {}, None))
        out.append((name, 21, 0, 1024, K, "F16", "RESID", nt, "sat", {}, None))
    return out


GEMM_SHAPES = {   # (BM, BN, PRO, EPI) -> [(N, K)]; the first takes the 971-row case
    (128, 128, "NORM", "STORE"): [(4096, 1024), (3072, 1024), (2048, 1024)],
    (128, 192, "NORM", "SWIGLU"): [(6144, 1024)],
    (128, 128, "NORM", "SWIGLU"): [(6144, 1024)],
    (64, 64, "F16", "RESID"): [(1024, 2048), (1024, 3072), (2048, 2048)],
    (128, 128, "F16", "RESID"): [(4096, 1024)],           # N > 2048: no product shape, reached through launch_linear
    (64, 64, "F16", "STORE"): [(2048, 1024), (1024, 2048)],
    (128, 128, "F16", "STORE"): [(3072, 1024), (4096, 1024)],
}


def gemm_cases():
    out = []
    for (bm, bn, pro, epi), glds in itertools.product(GEMM_TILES, (1, 0)):
        if not glds and bm + bn > 256:
            continue
        name = gemm_name(bm, bn, pro, epi, glds)
        shapes = GEMM_SHAPES[(bm, bn, pro, epi)]
        if (bm, bn, epi, glds) == (128, 128, "SWIGLU", 1):
            shapes = [(4096, 1024)]        # with the ring on, 6144 columns take the 192-column tile
        rows = [(0, 971), (0, 65), (0, 127), (0, 128), (0, 129), (0, 200), (16, 100), (48, 130)]
        for i, (mb, r) in enumerate(rows):
            N, K = shapes[0] if r == 971 else shapes[i % len(shapes)]
            modes = ("exact",) if r == 971 else ("random",) if r in (127, 128) else ("exact", "random")
            for mode in modes:
                ldy = N + 96 if (epi == "STORE" and mb == 16) else None
                out.append((name, mb + r, mb, N, K, pro, epi, i % 2, mode, dict(glds=glds), ldy))
        N, K = shapes[0]
        out.append((name, 971, 0, N, K, pro, epi, 0, "random", dict(glds=glds), None))
        if pro == "NORM":
            for eps in (1e-6, 1e-3):
                out.append((name, 70, 0, N, K, pro, epi, 0, "eps", dict(glds=glds), eps))
        if epi in ("RESID", "SWIGLU"):
            out.append((name, 16 + 77, 16, N, K, pro, epi, 1, "sat", dict(glds=glds), None))
    return out


LINEAR_CASES, NARROW_CASES, GEMM_CASES = linear_cases(), narrow_cases(), gemm_cases()


def _id(c):
    name, M, mb, N, K, pro, epi, nt, mode, kn, extra = c
    return f"{name}-M{M}-b{mb}-{N}x{K}-{mode}" + (f"-{extra}" if extra is not None else "")


def _run(lib, c):
    name, M, mb, N, K, pro, epi, nt, mode, kn, extra = c
    with knobs(lib, **kn):
        if mode == "eps":
            return run_case(lib, name, M, mb, N, K, pro, epi, nt, mode, eps=extra)
        return run_case(lib, name, M, mb, N, K, pro, epi, nt, mode, ldy=extra)


def _by_variant(cases):
    d = {}
    for c in cases:
        d.setdefault(c[0], []).append(c)
    return sorted(d.items())


@gpu
@pytest.mark.parametrize("name,cases", _by_variant(LINEAR_CASES), ids=[n for n, _ in _by_variant(LINEAR_CASES)])
def test_linear_kernel_variant(test_lib, name, cases):
    outs = {}
    for c in cases:
        o = _run(test_lib, c)
        if c[8] == "eps":
            outs[c[10]] = (o, c)
    if outs:
        _eps_matters(outs)


@gpu
@pytest.mark.parametrize("name,cases", _by_variant(NARROW_CASES), ids=[n for n, _ in _by_variant(NARROW_CASES)])
def test_linear_narrow_kernel_variant(test_lib, name, cases):
    for c in cases:
        _run(test_lib, c)


@gpu
@pytest.mark.parametrize("name,cases", _by_variant(GEMM_CASES), ids=[n for n, _ in _by_variant(GEMM_CASES)])
def test_gemm_kernel_variant(test_lib, name, cases):
    outs = {}
    for c in cases:
        o = _run(test_lib, c)
        if c[8] == "eps":
            outs[c[10]] = (o, c)
    if outs:
        _eps_matters(outs)


def _eps_matters(outs):
    """The two eps values give different outputs on the tiny rows, by the factor the reference says (each was graded
    against its own reference already; this makes the difference itself explicit), and finite zeros on the zero rows."""
    (oa, c), (ob, _) = outs[1e-6], outs[1e-3]
    key = "y" if "y" in oa else "act"
    a, b = oa[key].astype(np.float64), ob[key].astype(np.float64)
    N = c[3]
    a, b = a[:, :N] if key == "y" else a, b[:, :N] if key == "y" else b
    assert (a[1::3] == 0).all() and (b[1::3] == 0).all(), "all-zero rows: eps must keep the output a finite zero"
    if key == "y":
        ms = (oa["pro_ssq"].astype(np.float64).sum(-1) / c[4])[0::3]
        want = np.sqrt((ms + 1e-3) / (ms + 1e-6))[:, None]          # ~30
        big = np.abs(a[0::3]) > 1e-2
        ratio = a[0::3][big] / b[0::3][big]
        # the same accumulators under two scales, each within 8 u of its float64 value, and two final multiplies
        assert big.any() and np.abs(ratio / np.broadcast_to(want, big.shape)[big] - 1).max() < 32 * U
    else:
        assert np.abs(a[0::3]).max() > 10 * np.abs(b[0::3]).max() > 0


@gpu
def test_hook_refuses_what_callers_never_pass(test_lib):
    lib = test_lib
    rng = np.random.default_rng(1)
    N, K = 1024, 2048
    W = weights(N, K, "random", 0)
    x = rng.standard_normal((40, K)).astype(np.float16)
    h0 = np.zeros((40, N), np.float32)
    g = np.ones(N, np.float32)
    ok = dict(M=40, m_begin=16, N=N, K=K, W=W, gateup=0, pro=0, epi=1, nt=0, x16=x, h_io=h0, gamma_next=g)
    assert call(lib, **ok)[0] == 0
    assert call(lib, **{**ok, "m_begin": 8})[0] == -2
    assert call(lib, **{**ok, "m_begin": 48})[0] == -2             # m_begin >= M
    assert call(lib, **{**ok, "gamma_next": None, "want_xh": True})[0] == -2      # xh_out without gamma
    assert call(lib, **{**ok, "K": 512})[0] == -2
    assert call(lib, **{**ok, "epi": 0, "ldy": N - 16})[0] == -2
    # SwiGLU on fp16 input has no instantiation, neither streaming nor tiled: refused before the launch
    assert call(lib, 40, 16, N, K, W, 1, 0, 2, 0, x16=x)[:2] == (-2, "")
    assert call(lib, 100, 0, N, K, W, 1, 0, 2, 0, x16=rng.standard_normal((100, K)).astype(np.float16))[:2] == (-2, "")
    # the norm prologue needs 64 partials per row (K = 1024)
    hh = rng.standard_normal((8, K)).astype(np.float32)
    assert call(lib, 8, 0, N, K, W, 0, 1, 0, 0, h=hh, gamma=np.ones(K, np.float32))[0] == -2
    # a knob combination without an instantiation (two column tiles per workgroup with 8 k-blocks per wave)
    W1 = weights(2048, 1024, "random", 0)
    with knobs(lib, tuning=((1024, 2, 8),), wide=1, split=0):
        assert call(lib, 20, 0, 2048, 1024, W1, 0, 0, 0, 0, x16=rng.standard_normal((20, 1024)).astype(np.float16))[:2] == (-2, "")


@gpu
def test_zz_every_variant_was_observed_and_the_knobs_are_back(test_lib):
    """Last test of the module: the coverage of the table, the per-variant error table, and the default dispatch."""
    print("\nvariant: largest error / derived bound")
    for v in VARIANTS:
        if v in ERR:
            print(f"  {v:44s} {ERR[v]:.3f}")
    missing = [v for v in VARIANTS if v not in SEEN]
    assert not missing, f"variants of the table no case reached: {missing}"
    assert not (SEEN - set(VARIANTS)), SEEN - set(VARIANTS)
    assert max(ERR.values()) <= 1.0
    lib = test_lib
    lib.q3t_reset_linear_knobs()
    narrow8 = int(os.environ.get("Q3_LINEAR_NARROW8", "1")) != 0
    glds = int(os.environ.get("Q3_GEMM_GLDS", "1")) != 0
    run_case(lib, "linear<1,1,4,8,NORM,STORE,t>", 8, 0, 4096, 1024, "NORM", "STORE", 0, "random")
    run_case(lib, "linear<2,2,4,8,NORM,SWIGLU,nt>", 20, 0, 6144, 1024, "NORM", "SWIGLU", 1, "random")
    run_case(lib, "narrow<16,4,t>" if narrow8 else "linear<1,1,16,4,F16,RESID,t>", 8, 0, 1024, 2048, "F16", "RESID", 0, "exact")
    run_case(lib, "linear<1,4,4,8,F16,STORE,t>", 64, 0, 3072, 1024, "F16", "STORE", 0, "exact")
    run_case(lib, gemm_name(64, 64, "F16", "RESID", glds), 65, 0, 1024, 3072, "F16", "RESID", 0, "exact")
