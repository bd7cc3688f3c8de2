"""The speaker encoder's own kernels (csrc/q3_spk.hip: spk_unfold, spk_place, spk_rowmean, spk_matvec, spk_se_apply, spk_rowstat,
spk_att_act, spk_attnpool), one launch each through the hooks q3t_spk_*_case, against tests/spk_ops_ref.py (pinned on the CPU
by tests/test_glue_ops_reference.py).

  data movement (unfold, place)            bit for bit, no tolerance
  integer rows / integer matvec            every product and sum is exact in f32: the int64 reference bit for bit
  real data                                |y - float64| <= the derived bound, element by element
  edge rows                                a constant row, a mean large against the spread, an outlier; one-hot, uniform and
                                           +80 / -1e4 softmax rows
  every case                               clip b alone, and a row alone (C = 1), give the bits they have inside the batch
  tanhf / sigmoid                          the dense-grid probes behind TANH_ERR and SIGMOID_ERR

Lengths are 5, 6, 63, 64, 65, 129, 300 in ragged batches of 3 (NaN past each clip's own length and in the pad columns: a read
past the clip shows), channel counts 1, 4, 5, 6, 130 (a workgroup is 4 one-wave rows).  The hooks guard every word the
kernel is not to write (-3)."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import spk_ops_ref as R

pytestmark = pytest.mark.gpu

WORST = {}      # kernel -> (error / bound, case)
SINGLES = tuple((L,) for L in R.LENGTHS)


@pytest.fixture(scope="module")
def tl(test_lib):
    yield test_lib
    print("worst error / bound per kernel:", {k: (float(f"{v[0]:.3g}"), v[1]) for k, v in sorted(WORST.items())})


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def i32(a):
    return np.ascontiguousarray(a, np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def grade(key, y, ref, bound, case):
    """element-wise |y - ref| <= bound; notes the worst ratio"""
    assert np.isfinite(y).all(), f"{key} {case}: a non-finite output"
    err = np.abs(y.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(ratio.max())
    if worst > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (worst, case)
    assert worst <= 1.0, f"{key} {case}: error {worst:.3g} x the bound at {np.unravel_index(ratio.argmax(), ratio.shape)}"


# ---- the hooks -----------------------------------------------------------------------------------------------------------
def unfold(tl, x, c0, x2, c02, n_f, C, K, dil, rc=0):
    B, Cx, Lmax = x.shape
    y = np.full((B, C * K, R.pitch(Lmax)), np.nan, np.float32)
    got = tl.q3t_spk_unfold_case(hiplib.fptr(f32(x)), Cx, c0, hiplib.fptr(f32(x2)) if x2 is not None else None,
                                 x2.shape[1] if x2 is not None else 0, c02, hiplib.iptr(i32(n_f)), B, C, K, dil, hiplib.fptr(y))
    assert got == rc, f"q3t_spk_unfold_case -> {got}"
    return y


def place(tl, x, c0x, Cy, c0y, C, L, relu, rc=0):
    B, Cx, ld = x.shape
    y = np.full((B, C, ld), np.nan, np.float32)
    got = tl.q3t_spk_place_case(hiplib.fptr(f32(x)), Cx, c0x, Cy, c0y, C, L, relu, B, hiplib.fptr(y))
    assert got == rc, f"q3t_spk_place_case -> {got}"
    return y


def reduce(tl, which, x, n_f, z=None, rc=0):
    B, C, _ = x.shape
    out = np.full((B, C if which == "rowmean" else 2 * C), np.nan, np.float32)
    if which == "attnpool":
        got = tl.q3t_spk_attnpool_case(hiplib.fptr(f32(z)), hiplib.fptr(f32(x)), C, hiplib.iptr(i32(n_f)), B, hiplib.fptr(out))
    else:
        got = getattr(tl, f"q3t_spk_{which}_case")(hiplib.fptr(f32(x)), C, hiplib.iptr(i32(n_f)), B, hiplib.fptr(out))
    assert got == rc, f"q3t_spk_{which}_case -> {got}"
    return out


def matvec(tl, w, bias, x, act, rc=0):
    O, I = w.shape
    B = x.shape[0]
    out = np.full((B, O), np.nan, np.float32)
    got = tl.q3t_spk_matvec_case(hiplib.fptr(f32(w)), hiplib.fptr(f32(bias)) if bias is not None else None, hiplib.fptr(f32(x)), I, O,
                                 act, B, hiplib.fptr(out))
    assert got == rc, f"q3t_spk_matvec_case -> {got}"
    return out


def se_apply(tl, h, gate, res, L, Cy2, c02, rc=0):
    B, C, ld = h.shape
    y1, y2 = np.full((B, C, ld), np.nan, np.float32), np.full((B, C, ld), np.nan, np.float32)
    got = tl.q3t_spk_se_apply_case(hiplib.fptr(f32(h)), hiplib.fptr(f32(gate)), hiplib.fptr(f32(res)), C, L, Cy2, c02, B,
                                   hiplib.fptr(y1), hiplib.fptr(y2))
    assert got == rc, f"q3t_spk_se_apply_case -> {got}"
    return y1, y2


def att_act(tl, x, bias, L, rc=0):
    B, C, ld = x.shape
    y = np.full((B, C, ld), np.nan, np.float32)
    got = tl.q3t_spk_att_act_case(hiplib.fptr(f32(x)), hiplib.fptr(f32(bias)), C, L, B, hiplib.fptr(y))
    assert got == rc, f"q3t_spk_att_act_case -> {got}"
    return y


def alone(x, lens, b):
    """clip b of a ragged batch as a batch of one, at its own length"""
    return np.ascontiguousarray(x[b:b + 1, :, :lens[b]])


def odd_values(x, r):
    """-0, +0 and subnormals of both signs sprinkled over the finite entries"""
    x = x.copy()
    flat = x.reshape(-1)
    idx = np.flatnonzero(np.isfinite(flat))
    pick = r.choice(idx, size=min(len(idx), max(4, len(idx) // 7)), replace=False)
    specials = np.array([0x80000000, 0x00000000, 0x00000001, 0x807fffff, 0x00400000], np.uint32).view(np.float32)
    flat[pick] = specials[np.arange(len(pick)) % len(specials)]
    return x


# ---- data movement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dil", [(5, 1), (3, 2), (3, 3), (3, 4), (1, 1)])
def test_unfold(tl, K, dil):
    r = np.random.default_rng([K, dil])
    Cx, c0, C, Cx2, c02 = 7, 2, 3, 5, 1
    for lens in R.BATCHES + SINGLES:
        x = odd_values(R.rows(lens, Cx, "real", 1), r)
        x2 = odd_values(R.rows(lens, Cx2, "real", 2), r)
        for second in (None, x2):
            y = unfold(tl, x, c0, second, c02, lens, C, K, dil)
            want = R.unfold(x, c0, C, K, dil, lens, second, c02)
            assert not np.isnan(y).any(), f"{lens}: a NaN of the input's pad or of another clip's columns came through"
            bad = np.argwhere(bits(y) != bits(want))
            assert bad.size == 0, f"K={K} dil={dil} {lens} x2={second is not None}: {len(bad)} words differ, first at {bad[0]}"
            for b, L in enumerate(lens):
                assert not bits(y[b, :, L:]).any(), "columns past the clip's own length are +0 up to the pitch"


@pytest.mark.parametrize("relu", [0, 1])
def test_place(tl, relu):
    r = np.random.default_rng(relu)
    Cx, c0x, Cy, c0y, C = 7, 2, 9, 4, 3
    for L in R.LENGTHS:
        x = odd_values(r.standard_normal((3, Cx, R.pitch(L))).astype(np.float32), r)
        y = place(tl, x, c0x, Cy, c0y, C, L, relu)
        want = R.place(x, c0x, C, relu)
        assert np.isfinite(y).all()
        if relu:
            assert np.array_equal(y, want), f"L={L}"          # values: -0 and +0 are one
            assert not (y < 0).any()
        else:
            assert np.array_equal(bits(y), bits(want)), f"L={L}"
    # a slice at either end of the destination
    x = r.standard_normal((2, 4, 32)).astype(np.float32)
    assert np.array_equal(bits(place(tl, x, 0, 6, 0, 4, 5, 0)), bits(x))
    assert np.array_equal(bits(place(tl, x, 1, 6, 3, 3, 5, 0)), bits(x[:, 1:]))


@pytest.mark.parametrize("C", [1, 5])
def test_se_apply(tl, C):
    for L in R.LENGTHS:
        h, gate, res = R.se_case(L, C, 3)
        Cy2, c02 = 3 * C + 1, C + 1
        y1, y2 = se_apply(tl, h, gate, res, L, Cy2, c02)
        ref, bound = R.se_apply(h, gate, res)
        grade("se_apply", y1, ref, bound, f"L={L} C={C}")
        assert np.array_equal(bits(y1), bits(y2)), "the aggregate's slice is the next block's input, bit for bit"
        for b in range(3):
            a1, _ = se_apply(tl, h[b:b + 1], gate[b:b + 1], res[b:b + 1], L, Cy2, 0)
            assert np.array_equal(bits(a1[0]), bits(y1[b]))


@pytest.mark.parametrize("C", [1, 5])
def test_att_act(tl, C):
    for L in R.LENGTHS:
        x, bias = R.att_case(L, C, 3)
        y = att_act(tl, x, bias, L)
        ref, bound, zero = R.att_act(x, bias)
        assert zero.any() and (y[zero] == 0).all(), "exactly 0 wherever the rounded sum is <= 0"
        grade("att_act", y, ref, bound, f"L={L} C={C}")
        for b in range(3):
            assert np.array_equal(bits(att_act(tl, x[b:b + 1], bias[b:b + 1], L)[0]), bits(y[b]))


# ---- reductions ------------------------------------------------------------------------------------------------------------
def independent(tl, which, x, lens, y, z=None):
    """clip b alone, and its first and last rows alone (C = 1): the bits of the batch"""
    B, C, _ = x.shape
    half = lambda o, c, n: o[:, [c]] if which == "rowmean" else o[:, [c, n + c]]
    for b in range(B):
        one = reduce(tl, which, alone(x, lens, b), lens[b:b + 1], None if z is None else alone(z, lens, b))
        assert np.array_equal(bits(one[0]), bits(y[b])), f"{which} {lens}: clip {b} alone differs from clip {b} in the batch"
        for c in {0, C - 1}:
            row = reduce(tl, which, alone(x, lens, b)[:, c:c + 1], lens[b:b + 1], None if z is None else alone(z, lens, b)[:, c:c + 1])
            assert np.array_equal(bits(row), bits(half(y[b:b + 1], c, C))), f"{which} {lens}: row {c} of clip {b} alone differs"


@pytest.mark.parametrize("C", R.CHANNELS)
def test_rowmean_and_rowstat(tl, C):
    for lens in R.BATCHES:
        x = R.rows(lens, C, "real")
        for which, fn in (("rowmean", R.rowmean), ("rowstat", R.rowstat)):
            y = reduce(tl, which, x, lens)
            ref, bound = fn(x, lens)
            grade(which, y, ref, bound, f"{lens} C={C}")
            independent(tl, which, x, lens, y)


@pytest.mark.parametrize("C", R.CHANNELS)
def test_attnpool(tl, C):
    for lens in R.BATCHES:
        x = R.rows(lens, C, "real")
        z = R.attn_logits(lens, C, "normal")
        y = reduce(tl, "attnpool", x, lens, z)
        ref, bound = R.attnpool(z, x, lens)
        grade("attnpool", y, ref, bound, f"normal {lens} C={C}")
        independent(tl, "attnpool", x, lens, y, z)
        # all logits equal: the softmax is 1 / L and the result is spk_rowstat's; +80 stays finite under the max subtraction
        stat, _ = R.rowstat(x, lens)
        for kind in ("zero", "p80", "m1e4"):
            z = R.attn_logits(lens, C, kind)
            y = reduce(tl, "attnpool", x, lens, z)
            _, bound = R.attnpool(z, x, lens)
            grade("attnpool", y, stat, bound, f"{kind} {lens} C={C}")
        # one column ahead of the rest by 120 or more: the weights are one-hot
        clamp = np.sqrt(np.float32(1e-12), dtype=np.float32)
        for kind in ("hot0", "hotlast", "hot63"):
            z = R.attn_logits(lens, C, kind)
            y = reduce(tl, "attnpool", x, lens, z)
            for b, L in enumerate(lens):
                col = R.hot_column(kind, L)
                assert (z[b, :, col, None] - np.delete(z[b, :, :L], col, axis=1) >= 120).all()
                assert np.array_equal(bits(y[b, :C]), bits(x[b, :, col])), f"{kind} {lens} clip {b}: the mean is that column's x"
                assert (np.abs(bits(y[b, C:]).astype(np.int64) - int(clamp.view(np.uint32))) <= 1).all(), f"{kind} {lens} clip {b}: the std is the clamp"


@pytest.mark.parametrize("L", R.LENGTHS)
def test_rowstat_edge_rows(tl, L):
    x, names = R.rowstat_edge_rows(L)
    y = reduce(tl, "rowstat", x, [L])
    ref, bound = R.rowstat(x, [L])
    for c in (1, 2, 3):
        grade("rowstat", y[:, [c, 4 + c]], ref[:, [c, 4 + c]], bound[:, [c, 4 + c]], f"{names[c]} L={L}")
    if L == 64:      # 1 / 64 and every partial sum are exact: the mean is the constant, d = 0 and the std is the clamp
        clamp = np.sqrt(np.float32(1e-12), dtype=np.float32)
        assert y[0, 0] == np.float32(0.25)
        assert abs(int(bits(y[0, 4:5])[0]) - int(clamp.view(np.uint32))) <= 1
    else:            # elsewhere the constant row is within a rounding of 1 / L of it (and the clamp of what that leaves)
        assert abs(float(y[0, 0]) - 0.25) <= bound[0, 0]


@pytest.mark.parametrize("L", [64, 128])
def test_integer_rows_are_exact(tl, L):
    lens = (L, L, L)
    for C in R.CHANNELS:
        x = R.rows(lens, C, "int")
        want = (x.astype(np.int64).sum(2) / L).astype(np.float32)
        assert np.array_equal(want.astype(np.float64) * L, x.astype(np.int64).sum(2))
        assert np.array_equal(bits(reduce(tl, "rowmean", x, lens)), bits(want)), f"rowmean L={L} C={C}"
        x = R.rows(lens, C, "intstat")
        xi = x.astype(np.int64)
        assert np.abs(xi).max() <= 16 and not (xi.sum(2) % L).any()
        mean = xi.sum(2) // L
        var = ((xi - mean[:, :, None]) ** 2).sum(2) / L           # a multiple of 1 / L below 2^10: exact in f32
        want = np.concatenate([mean, np.sqrt(np.maximum(var, R.STD_FLOOR))], axis=1).astype(np.float32)
        assert np.array_equal(bits(reduce(tl, "rowstat", x, lens)), bits(want)), f"rowstat L={L} C={C}"
        z = R.attn_logits(lens, C, "zero")       # expf(0) = 1, the denominator is L and 1 / L is exact: spk_rowstat's numbers
        assert np.array_equal(bits(reduce(tl, "attnpool", x, lens, z)), bits(want)), f"attnpool L={L} C={C}"


# ---- the matvec ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", R.MATVEC_I)
def test_matvec(tl, I):
    r = np.random.default_rng(I)
    for O in R.CHANNELS:
        for with_bias in (False, True):
            w, bias, x = R.matvec_case(I, O, 3, with_bias)
            for act in (0, 1, 2):
                y = matvec(tl, w, bias, x, act)
                ref, bound = R.matvec(w, bias, x, act)
                grade(f"matvec act {act}", y, ref, bound, f"I={I} O={O} bias={with_bias}")
                if act == 1 and with_bias and O > 1:
                    assert (y[:, 1::2] == 0).all() and (y[:, 0::2] > 0).all()       # the ReLU clips the odd outputs
                for b in range(3):
                    assert np.array_equal(bits(matvec(tl, w, bias, x[b:b + 1], act)[0]), bits(y[b]))
                o = O - 1
                assert np.array_equal(bits(matvec(tl, w[o:o + 1], None if bias is None else bias[o:o + 1], x, act)[:, 0]), bits(y[:, o]))
        # integers: every product and partial sum is exact
        w = r.integers(-8, 9, (O, I))
        x = r.integers(-8, 9, (3, I))
        bias = r.integers(-64, 65, O)
        want = (x @ w.T + bias).astype(np.float32)
        assert ((np.abs(x) @ np.abs(w).T + 64) < 2 ** 24).all()
        assert np.array_equal(bits(matvec(tl, w, bias, x, 0)), bits(want)), f"integer matvec I={I} O={O}"
        assert np.array_equal(bits(matvec(tl, w, None, x, 0)), bits((x @ w.T).astype(np.float32)))


# ---- the device functions no bound derives ---------------------------------------------------------------------------------
def test_device_function_probes(tl):
    """TANH_ERR / SIGMOID_ERR of tests/spk_ops_ref.py: the hooks in their identity setting over a dense grid, against float64.
    tanhf: spk_att_act with a zero bias over [0, 12].  The sigmoid: spk_matvec with I = 1, act = 2 and the input 1, the grid over
    [-30, 30] as the weights (fma(w, 1, 0) = w exactly)."""
    n = 1 << 17
    g = R.grid(0.0, 12.0, n).reshape(1, 128, 1024)
    y = att_act(tl, g, np.zeros((1, 128), np.float32), 1024)
    tanh = float(np.abs(y.astype(np.float64) - np.tanh(g.astype(np.float64))).max())
    g = R.grid(-30.0, 30.0, n)
    y = matvec(tl, g.reshape(n, 1), None, np.ones((1, 1), np.float32), 2)[0]
    sig = float(np.abs(y.astype(np.float64) - R.sigmoid64(g)).max())
    print(f"PROBE tanhf [0, 12]: {tanh:.3e}  constant {R.TANH_ERR:.3e}  recorded {R.TANH_MEASURED:.3e}")
    print(f"PROBE sigmoid [-30, 30]: {sig:.3e}  constant {R.SIGMOID_ERR:.3e}  recorded {R.SIGMOID_MEASURED:.3e}")
    assert R.TANH_ERR <= R.PROBE_CEILING and R.SIGMOID_ERR <= R.PROBE_CEILING
    assert tanh <= R.TANH_ERR and sig <= R.SIGMOID_ERR


# ---- refusals: on the host, before any launch ------------------------------------------------------------------------------
def test_hook_refusals(tl):
    x = R.rows((5, 9), 4, "real")
    assert unfold(tl, x, 0, None, 0, (5, 9), 4, 3, 1).shape == (2, 12, 32)
    unfold(tl, x, 2, None, 0, (5, 9), 3, 3, 1, rc=-2)          # the slice leaves x
    unfold(tl, x, 0, x, 2, (5, 9), 3, 3, 1, rc=-2)             # the slice leaves x2
    unfold(tl, x, 0, None, 0, (5, 9), 4, 4, 1, rc=-2)          # an even tap count
    unfold(tl, x, 0, None, 0, (4, 9), 4, 3, 4, rc=-2)          # a clip shorter than the reflection needs
    unfold(tl, x, 0, None, 0, (0, 9), 4, 1, 1, rc=-2)
    xp = np.zeros((2, 4, 32), np.float32)
    place(tl, xp, 2, 6, 0, 3, 5, 0, rc=-2)
    place(tl, xp, 0, 6, 4, 3, 5, 0, rc=-2)
    place(tl, xp, 0, 6, 0, 3, 5, 2, rc=-2)
    place(tl, xp, 0, 6, 0, 3, 0, 0, rc=-2)
    for which in ("rowmean", "rowstat"):
        reduce(tl, which, x, (5, 0), rc=-2)
        reduce(tl, which, x[:, :0], (5, 9), rc=-2)
    reduce(tl, "attnpool", x, (5, -1), x, rc=-2)
    w = np.zeros((4, 8), np.float32)
    matvec(tl, w, None, np.zeros((2, 8), np.float32), 3, rc=-2)
    matvec(tl, w, None, np.zeros((0, 8), np.float32), 0, rc=-2)
    se_apply(tl, xp, np.zeros((2, 4), np.float32), xp, 5, 6, 3, rc=-2)      # the slice leaves the aggregate
    se_apply(tl, xp, np.zeros((2, 4), np.float32), xp, 0, 6, 0, rc=-2)
    att_act(tl, xp, np.zeros((2, 4), np.float32), 0, rc=-2)
