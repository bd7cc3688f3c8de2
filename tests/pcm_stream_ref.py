"""Float64 restatement of the streaming encode's PCM front-end (csrc/q3_enc_stream_pcm_host.h, csrc/q3_enc_stream_pcm.hip) in
numpy, over tests/pcm_ref.py's taps and factors:

    ready(n) = 0 if n up - 1 - half < 0 else (n up - 1 - half) // down + 1      samples settled by n frames of a running stream
    total(n, finished) = ceil(n up / down) if finished else ready(n)
    a push from n0 to n1 frames computes outputs ready(n0) .. total(n1, finish) - 1 from [carry | new], frames >= n1 as zeros;
    carry = the last J - 1 frames (zeros before the clip's start), J = ceil(N / up)

tests/test_enc_stream_pcm_contract.py holds it against pcm_ref.resample of the whole clip; the GPU tests take their counts
from it."""
from __future__ import annotations

import numpy as np

from tests import pcm_ref as P


def geometry(rate):
    """-> (up, down, half, J)"""
    up, down = P.factors(rate)
    h, half = P.taps(up, down)
    return up, down, half, -(-h.size // up)


def ready(n, rate):
    up, down, half, _ = geometry(rate)
    a = int(n) * up - 1 - half
    return 0 if a < 0 else a // down + 1


def total(n, rate, finished):
    up, down, _, _ = geometry(rate)
    return P.out_len(n, up, down) if finished else ready(n, rate)


def max_frames_in(max_push, rate):
    """a sufficient per-entry frame count of one push: (n up + half) / down <= max_push"""
    up, down, half, _ = geometry(rate)
    return max((int(max_push) * down - half) // up, 0)


class Stream:
    """one stream's carry-state resample of float64 mono frames at `rate`"""

    def __init__(self, rate):
        self.rate = rate
        self.up, self.down, self.half, self.J = geometry(rate)
        self.h = P.taps(self.up, self.down)[0]
        self.carry = np.zeros(self.J - 1)
        self.n0 = 0

    def push(self, x, finish=False):
        """-> the float64 samples this push settles"""
        x = np.asarray(x, np.float64)
        J, up, down, N = self.J, self.up, self.down, self.h.size
        n0, n1 = self.n0, self.n0 + x.size
        v = np.concatenate([self.carry, x])              # frames n0 - (J - 1) .. n1 - 1
        base = n0 - (J - 1)
        m = np.arange(ready(n0, self.rate), total(n1, self.rate, finish), dtype=np.int64)
        a = m * down + self.half
        i0, p = a // up, a % up
        assert finish or m.size == 0 or int(i0.max()) <= n1 - 1
        y = np.zeros(m.size)
        for j in range(J):
            t, i = p + j * up, i0 - j
            ok = (t < N) & (i >= 0) & (i < n1)
            assert not ok.any() or int((i - base)[ok].min()) >= 0, "a push reads behind its carry"
            xv = np.where(ok, v[np.clip(i - base, 0, max(v.size - 1, 0))], 0.0) if v.size else np.zeros(m.size)
            y += xv * np.where(ok, self.h[np.minimum(t, N - 1)], 0.0)
        self.carry = v[v.size - (J - 1):] if J > 1 else v[:0]
        self.n0 = n1
        return y


def splits(n, J, kind, seed=0):
    """-> [(frames of the push, finish)]: how a clip of n input frames reaches its stream.  one: a single finishing push;
    frames: one frame per push for the first 2 J frames, then ragged; short: every push shorter than J - 1, zero-frame pushes
    in between; finish_alone: ragged, the finish with 0 new frames"""
    r = np.random.default_rng(seed)
    if kind == "one":
        return [(n, True)]
    sizes, left = [], n
    while left > 0:
        if kind == "frames":
            s = 1 if len(sizes) < 2 * J else int(r.integers(1, 6 * J + 40))
        elif kind == "short":
            s = 0 if len(sizes) % 3 == 1 else int(r.integers(1, max(J - 1, 2)))
        else:
            s = int(r.integers(0, 8 * J + 60))
        s = min(s, left)
        sizes.append(s)
        left -= s
    if kind == "finish_alone" or not sizes:
        return [(s, False) for s in sizes] + [(0, True)]
    return [(s, i == len(sizes) - 1) for i, s in enumerate(sizes)]
