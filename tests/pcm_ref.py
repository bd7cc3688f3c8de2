"""Float64 restatement of the encoder's PCM front-end (csrc/q3_enc_pcm.hip, csrc/q3_enc_pcm_host.h) in numpy, without scipy:
sample decode, downmix, scipy.signal.resample_poly's rules with its defaults.

    s16: v / 32768; f32: as is.  mono = the mean of the C channels, in float64
    g = gcd(R, 24000), up = 24000 / g, down = R / g; up == down == 1: no filter
    mr = max(up, down), half = 10 mr, N = 2 half + 1
    h[k] = up w[k] / sum(w),  w[k] = (1 / mr) sinc((k - half) / mr) I0(5 sqrt(1 - ((k - half) / half)^2)) / I0(5)
    n_out = ceil(n up / down),  y[m] = sum_i x[i] h[m down + half - i up],  0 <= i < n, tap index in [0, N)

tests/test_pcm_reference.py holds it against scipy; the GPU tests grade the device against it."""
from __future__ import annotations

import math

import numpy as np

RATE = 24000
MAX_FACTOR = 640


def factors(rate):
    g = math.gcd(int(rate), RATE)
    return RATE // g, int(rate) // g


def out_len(n, up, down):
    return -(-(int(n) * up) // down)


def taps(up, down):
    """-> (h float64 [N], half); up == down == 1: ([1.0], 0)"""
    mr = max(up, down)
    if mr == 1:
        return np.ones(1), 0
    half = 10 * mr
    m = np.arange(-half, half + 1, dtype=np.float64)
    w = (1.0 / mr) * np.sinc(m / mr) * np.i0(5.0 * np.sqrt(np.maximum(1.0 - (m / half) ** 2, 0.0))) / np.i0(5.0)
    return up * w / w.sum(), half


def decode(x, channels=1):
    """int16 / float32 array [n] or [n][C] -> float64 mono [n]"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        v = x.astype(np.float64) / 32768.0
    elif x.dtype == np.float32:
        v = x.astype(np.float64)
    else:
        raise TypeError(x.dtype)
    v = v.reshape(-1, channels)
    acc = np.zeros(v.shape[0])
    for c in range(channels):          # (in channel order, as the kernel adds them)
        acc = acc + v[:, c]
    return acc / channels


def resample(x, rate, want_mag=False):
    """float64 mono at `rate` -> float64 y [n_out] (want_mag: also sum |x_i| over each output's support)"""
    x = np.asarray(x, np.float64)
    up, down = factors(rate)
    n = x.size
    n_out = out_len(n, up, down)
    h, half = taps(up, down)
    N = h.size
    J = -(-N // up)
    a = np.arange(n_out, dtype=np.int64) * down + half
    i0, p = a // up, a % up
    y, mag = np.zeros(n_out), np.zeros(n_out)
    for j in range(J):
        t, i = p + j * up, i0 - j
        ok = (t < N) & (i >= 0) & (i < n)
        xv = np.where(ok, x[np.clip(i, 0, n - 1)], 0.0)
        y += xv * np.where(ok, h[np.minimum(t, N - 1)], 0.0)
        mag += np.abs(xv)
    return (y, mag) if want_mag else y


def prepare(x, rate, channels=1, want_mag=False):
    """what the front-end computes for one clip, before the rounding to float32"""
    return resample(decode(x, channels), rate, want_mag)
