"""Plain numpy statements of the encoder's strided-conv input kernels (enc_unfold_kernel, csrc/q3_enc.hip;
enc_stream_unfold_kernel and enc_stream_emit_kernel, csrc/q3_enc_stream.hip) -- test infrastructure for
tests/test_gpu_enc_unfold.py, pinned on the CPU by tests/test_glue_ops_reference.py: the clip unfold followed by a float64
matmul is tests/enc_ref.py's strided conv, and the streaming unfold (pushes plus carry) concatenates to the clip unfold bit
for bit for every split below.

All three are data movement: the functions return the float32 values moved (bit for bit what the kernel must write without
ELU).  With ELU the kernel applies expm1f to values < 0: elu64 is the float64 function, voc_conv_ref.ELU_ERR the device's
measured distance from it for x < 0, and +-0 passes through unchanged (expm1(+-0) = +-0)."""
from __future__ import annotations

import numpy as np

# (k, s, replicate, elu): Mimi's strided ops and two more pairs of flags
GEOMETRIES = ((4, 2, 1, 0), (8, 4, 0, 1), (10, 5, 0, 1), (12, 6, 0, 1), (16, 8, 0, 1), (8, 4, 0, 0))
STREAM_T = lambda s: sorted({1, max(1, s - 1), s, 2 * s + 1, 37, 300})
CLIP_LENS = lambda s: sorted({1, max(1, s - 1), s, s + 1, 2 * s + 1, 37, 600})


def pitch(L):
    return (int(L) + 31) & ~31


def elu64(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= 0, np.expm1(np.minimum(v, 0.0)), v)


def clip_unfold(x, lens, k, s, replicate):
    """x [B][Cin][Lmax] -> y [B][Cin * k][ceil(Lmax / s)] in x's dtype: row ci * k + j, column u < ceil(len_b / s) is
    xpad_b[ci][u * s + j - (k - s)], xpad_b = clip b's own columns with zeros (or, replicate, its first / last column) for
    every index < 0 or >= len_b; +0 from ceil(len_b / s) on"""
    B, Cin, Lmax = x.shape
    Lout = -(-Lmax // s)
    y = np.zeros((B, Cin * k, Lout), x.dtype)
    for b in range(B):
        n = int(lens[b])
        nout = -(-n // s)
        for j in range(k):
            i = np.arange(nout) * s + j - (k - s)
            inside = (i >= 0) & (i < n)
            v = x[b][:, np.clip(i, 0, n - 1)]
            if not replicate:
                v = np.where(inside[None, :], v, np.zeros((), x.dtype))
            y[b, j::k, :nout] = v
    return y


def stream_counts(before, n_in, finish, s):
    """-> the outputs of a push: whole strides while the stream runs, rounded up once it finishes"""
    after = before + n_in
    return (-(-after // s) if finish else after // s) - before // s


class StreamUnfold:
    """One stream of one strided op, a push at a time (MimiConv1d in its streaming form).  The carry [Cin][k - 1] starts as
    zeros (the causal padding); its first cnt = (k - s) + before % s columns are live: the left context of the next output and
    the columns no whole stride has consumed."""

    def __init__(self, Cin, k, s, replicate, dtype=np.float32):
        self.Cin, self.k, self.s, self.replicate = Cin, k, s, replicate
        self.carry = np.zeros((Cin, k - 1), dtype)
        self.before = 0

    def cnt(self):
        return (self.k - self.s) + self.before % self.s

    def push(self, x_new, finish):
        """x_new [Cin][n_in] -> y [Cin * k][n_out]; the carry and the column count move on unless the push finishes"""
        k, s = self.k, self.s
        n_in = x_new.shape[1]
        cnt = self.cnt()
        head = self.carry[:, :cnt]
        if self.before == 0 and self.replicate and n_in > 0:
            head = np.repeat(x_new[:, :1], cnt, axis=1)         # the stream's first column stands in for the left padding
        V = np.concatenate([head, x_new], axis=1)
        total = V.shape[1]
        n_out = stream_counts(self.before, n_in, finish, s)
        y = np.zeros((self.Cin * k, n_out), x_new.dtype)
        for t in range(k):
            i = np.arange(n_out) * s + t
            if total == 0:
                continue
            v = V[:, np.minimum(i, total - 1)]
            if not self.replicate:
                v = np.where((i < total)[None, :], v, np.zeros((), x_new.dtype))
            y[t::k] = v
        if not finish:
            cnt2 = (k - s) + (self.before + n_in) % s
            assert n_out * s + cnt2 == total
            self.carry[:, :cnt2] = V[:, n_out * s:]
            self.before += n_in
        return y


def splits(T, s, seed):
    """The pushes a stream of T columns is cut into: lists of (n_in, finish).  One push; one column a push; empty pushes first,
    in the middle and as the finishing push; a finishing empty push behind a total that is no multiple of s where T allows it
    (the last output then comes out of the carry alone); three seeded random cuts."""
    out = {"one": [(T, 1)], "single": [(1, 0)] * (T - 1) + [(1, 1)]}
    h = T // 2
    out["empty"] = [(0, 0), (h, 0), (0, 0), (T - h, 0), (0, 1)]
    r = np.random.default_rng([T, s, seed])
    for i in range(3):
        cuts = np.sort(r.integers(0, T + 1, int(r.integers(1, 6))))
        sizes = np.diff(np.concatenate([[0], cuts, [T]]))
        out[f"random{i}"] = [(int(n), 0) for n in sizes[:-1]] + [(int(sizes[-1]), 1)]
    return out


def emit(y, skip, n, off, rows, fill):
    """columns [skip, skip + n) of y [B][C][skip + n] -> out [rows][C], row off[b] + j; the other rows keep `fill` (uint32 bits)"""
    B, C, _ = y.shape
    out = np.full((rows, C), fill, np.uint32)
    for b in range(B):
        out[off[b]:off[b] + n] = y[b, :, skip:skip + n].T.view(np.uint32)
    return out
