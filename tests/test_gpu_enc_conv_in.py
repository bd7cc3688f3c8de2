"""enc_conv_in_kernel (csrc/q3_enc.hip), the encoder's one-channel first conv, one launch at a time through the test hook
q3t_enc_conv_in_case, at every tap count class the loader admits (1..16; the product's tables run 7 and 5), in both forms:
a whole clip (zeros left of column 0) and a stream's push (the k - 1 carried samples, rolled on by the same launch).

Exact-integer data (multiples of 1/4, sums far below 2^24 / 16): y equals float64 exactly.  Real data: within
(k + 1) * 2^-24 * (|bias| + sum |w||x|) per output -- k fma roundings on top of the bias.  The history afterwards is the last
k - 1 samples of [history | new] bit for bit, and a stream the call does not name keeps its history.  The hook holds NaN in
the pad columns of x and guards the pads of y and the words behind the history block (-3)."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import rvq_ref as R

pytestmark = pytest.mark.gpu

MAX_STREAMS = 4
STREAMS = np.array([2, 0, 3], np.int32)      # B = 3 entries over a permuted map; stream 1 is not named


@pytest.fixture(scope="module")
def tl(test_lib):
    return test_lib


def run(tl, x, w, bias, hist=None, streams=None, rc=0):
    """-> (y [B][cout][n], the history block after the call)"""
    x, w = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32)
    B, n = x.shape
    cout, k = w.shape
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    y = np.full((B, cout, n), np.nan, np.float32)
    h = None
    if hist is not None:
        h = np.ascontiguousarray(hist, np.float32).copy()
        buf = h if h.size else np.zeros(1, np.float32)      # (k = 1 carries nothing: the pointer only says "a stream")
    got = tl.q3t_enc_conv_in_case(hiplib.fptr(x), B, n, hiplib.fptr(w), hiplib.fptr(b) if b is not None else None, cout, k,
                                  hiplib.fptr(buf) if hist is not None else None, MAX_STREAMS if hist is not None else 0,
                                  hiplib.iptr(np.ascontiguousarray(streams, np.int32)) if streams is not None else None,
                                  hiplib.fptr(y))
    assert got == rc, f"q3t_enc_conv_in_case -> {got}"
    return y, h


def lengths(k):
    """1, a push shorter than the history (k - 2), both sides of the 256-column workgroup edge, several workgroups"""
    return sorted({n for n in (1, k - 2, 255, 256, 257, 600) if n >= 1})


def quarters(r, shape, lim):
    return (r.integers(-lim, lim + 1, shape) / 4).astype(np.float32)


@pytest.mark.parametrize("cout", [1, 5, 32])
@pytest.mark.parametrize("k", [1, 2, 7, 16])
def test_conv_in(tl, k, cout):
    r = np.random.default_rng(100 * k + cout)
    H = k - 1
    worst = 0.0
    for n in lengths(k):
        for with_bias in (False, True):
            for exact in (True, False):
                if exact:
                    x, w = quarters(r, (3, n), 8), quarters(r, (cout, k), 4)
                    bias = quarters(r, cout, 8) if with_bias else None
                    hist = quarters(r, (MAX_STREAMS, H), 8)
                else:
                    x = (0.3 * r.standard_normal((3, n))).astype(np.float32)
                    w = (r.standard_normal((cout, k)) / np.sqrt(k)).astype(np.float32)
                    bias = (0.02 * r.standard_normal(cout)).astype(np.float32) if with_bias else None
                    hist = (0.3 * r.standard_normal((MAX_STREAMS, H))).astype(np.float32)
                for form in ("clip", "stream"):
                    left = hist[STREAMS] if form == "stream" else None
                    want, mag, carry = R.conv_in_reference(x, w, bias, left)
                    if form == "clip":
                        y, _ = run(tl, x, w, bias)
                    else:
                        y, h = run(tl, x, w, bias, hist, STREAMS)
                        assert np.array_equal(h[1].view(np.uint32), hist[1].view(np.uint32)), "an unnamed stream's history moved"
                        assert np.array_equal(h[STREAMS].view(np.uint32), carry.astype(np.float32).view(np.uint32)), \
                            f"k={k} n={n}: the history is not the last k - 1 samples of [history | new]"
                    what = f"k={k} cout={cout} n={n} bias={with_bias} {form}"
                    if exact:
                        assert mag.max() * 16 < 2 ** 24
                        assert np.array_equal(y.astype(np.float64), want), f"{what}: exact data, {int((y != want).sum())} outputs differ"
                    else:
                        err = np.abs(y.astype(np.float64) - want)
                        bound = (k + 1) * R.U32 * mag
                        worst = max(worst, float((err / bound).max()))
                        assert (err <= bound).all(), f"{what}: {float((err / bound).max()):.2f} of the bound"
    print(f"k={k} cout={cout}: worst real-data error {worst:.3f} of the bound")


def test_a_split_clip_is_the_whole_clip(tl):
    """pushes of every kind (shorter than the history, across the workgroup edge) joined are the whole clip, bit for bit"""
    r = np.random.default_rng(9)
    k, cout, n = 16, 5, 900
    x = (0.3 * r.standard_normal((3, n))).astype(np.float32)
    w = (r.standard_normal((cout, k)) / 4).astype(np.float32)
    bias = (0.1 * r.standard_normal(cout)).astype(np.float32)
    whole, _ = run(tl, x, w, bias)
    hist = np.zeros((MAX_STREAMS, k - 1), np.float32)
    hist[1] = 7.5
    parts, at = [], 0
    for m in (1, 3, 14, 15, 16, 257, 594):
        y, hist = run(tl, x[:, at:at + m], w, bias, hist, STREAMS)
        parts.append(y)
        at += m
    assert at == n and (hist[1] == 7.5).all()
    assert np.array_equal(np.concatenate(parts, 2).view(np.uint32), whole.view(np.uint32))


def test_hook_refusals(tl):
    x, w = np.zeros((3, 8), np.float32), np.zeros((4, 7), np.float32)
    y = np.zeros((3, 4, 8), np.float32)
    hist = np.zeros((MAX_STREAMS, 6), np.float32)
    call = lambda B, n, cout, k, h, ms, st: tl.q3t_enc_conv_in_case(
        hiplib.fptr(x), B, n, hiplib.fptr(w), None, cout, k, hiplib.fptr(hist) if h else None, ms,
        hiplib.iptr(np.asarray(st, np.int32)) if st is not None else None, hiplib.fptr(y))
    assert call(3, 8, 4, 7, False, 0, None) == 0
    assert call(3, 8, 4, 7, True, 4, [2, 0, 3]) == 0
    assert call(3, 8, 4, 0, False, 0, None) == -2 and call(3, 8, 4, 17, False, 0, None) == -2      # 1..16 taps
    assert call(0, 8, 4, 7, False, 0, None) == -2 and call(3, 0, 4, 7, False, 0, None) == -2
    assert call(3, 8, 0, 7, False, 0, None) == -2
    assert call(3, 8, 4, 7, True, 4, None) == -2 and call(3, 8, 4, 7, False, 4, [2, 0, 3]) == -2   # history and map go together
    assert call(3, 8, 4, 7, True, 4, [2, 0, 4]) == -2 and call(3, 8, 4, 7, True, 4, [2, 0, 2]) == -2
