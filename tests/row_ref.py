"""Plain-numpy reference of the frame loop's row kernels -- TEST INFRASTRUCTURE ONLY.

final_norm, gather_embed, feedback, prompt_rows and prefix_move (csrc/q3_kernels.h: FinalNormArgs, launch_gather_embed,
launch_feedback, PromptRowsArgs, PrefixMoveArgs), written from those comments.  The pieces a residual row is graded with
(feedback_row, gather_row, ssq_parts, xh_row, fp16_ulp) are tests/sample_ref.py's.

tests/test_row_reference.py pins this file; tests/test_gpu_row_kernels.py runs the kernels against it.
"""
from __future__ import annotations

import numpy as np

from tests import sample_ref as SR

U24 = 2.0 ** -24          # unit round-off of f32
F16_MAX = 65504.0


# ---- final norm --------------------------------------------------------------------------------------------------------
def final_norm_ref(h_row, ssq_row, gamma, eps, H):
    """float64: o = h * g / sqrt(sum(ssq) / H + eps), from the partials the producer stored (never from h itself)."""
    inv = 1.0 / np.sqrt(np.asarray(ssq_row, np.float64).sum() / H + float(np.float32(eps)))
    return np.asarray(h_row, np.float64) * inv * np.asarray(gamma, np.float64)


def final_norm_roundings(parts):
    """f32 operations between the inputs and one output element, in the kernel's order: a lane of the first wave adds
    its ceil(parts / 64) partials, six butterfly adds make the wave's sum, then divide by H, add eps, sqrt, reciprocal, and
    two multiplies (h * inv, * gamma)."""
    return -(-int(parts) // 64) + 6 + 6


def final_norm_bound(o, parts):
    """|out_f32 - o| allowed, first order in u = 2^-24 with one u per operation of final_norm_roundings.  Every term of
    the sum is a sum of squares (>= 0) and eps > 0, so no addition cancels and each operation's relative error carries to
    the result with a factor of at most 1 (1/2 through the square root, counted as 1).  The build has no fast-math:
    divide and sqrt are correctly rounded.  13 u at parts <= 64; + one f32 subnormal step for results down there."""
    return final_norm_roundings(parts) * U24 * np.abs(np.asarray(o, np.float64)) + 2.0 ** -149


def final_norm_f32(h_row, ssq_row, gamma, eps, H):
    """The same value in np.float32, operation for operation in the order final_norm_roundings counts: lane l of 64 adds
    partials l, l + 64, ...; the butterfly exchanges with lane ^ 32, 16, 8, 4, 2, 1."""
    f = np.float32
    ssq_row = np.asarray(ssq_row, f)
    lanes = np.zeros(64, f)
    for p in range(len(ssq_row)):
        lanes[p % 64] = lanes[p % 64] + ssq_row[p]
    idx = np.arange(64)
    for mask in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ mask]
    inv = f(1.0) / np.sqrt(lanes[0] / f(H) + f(eps))
    return (np.asarray(h_row, f) * inv) * np.asarray(gamma, f)


def f16_of(o):
    """The saturated value out_f16 rounds: o clipped to the fp16 range (float64)."""
    return np.clip(np.asarray(o, np.float64), -F16_MAX, F16_MAX)


def check_stored_row(h_row, ssq_row, xh_bits, gamma, what):
    """The contract of a stored residual row (store_row_ssq), graded against the row the device stored: ssq within
    (H + 4) * 2^-23 of the float64 sums of its blocks of 16, xh within one fp16 ulp of (h * gamma) / 16 saturated --
    check_cp's tolerances."""
    H = len(h_row)
    want = SR.ssq_parts(h_row)
    err = np.abs(np.asarray(ssq_row, np.float64) - want)
    assert (err <= (H + 4) * 2.0 ** -23 * want).all(), f"{what}: ssq off by {err.max()}"
    if xh_bits is not None:
        xw = SR.xh_row(h_row, gamma)
        err = np.abs(np.asarray(xh_bits, np.uint16).view(np.float16).astype(np.float64) - xw)
        assert (err <= SR.fp16_ulp(xw)).all(), f"{what}: xh off by {err.max()}"


# ---- gather ------------------------------------------------------------------------------------------------------------
def gather_token(tok, n_frames, frame_cap, col, forced, r):
    """The id row r gathers in the `codes` form of launch_gather_embed: column col of frame n_frames[r] - 1 clamped to
    [0, frame_cap); a teacher-forced id >= 0 replaces it, except that it does not revive an id that is negative (a
    finished row)."""
    f = min(max(int(n_frames[r]) - 1, 0), frame_cap - 1)
    t = int(tok[f, r, col])
    if forced is not None and forced[f, r, col] >= 0 and t >= 0:
        t = int(forced[f, r, col])
    return t


# ---- codec prompt ------------------------------------------------------------------------------------------------------
def prompt_ring(past, codes, T):
    """PromptRowsArgs: column 0 of the last min(T, 32) frames goes into the ring at i & 31; the other words stay;
    n_past = T."""
    ring = np.array(past, np.int32, copy=True)
    for i in range(max(0, T - SR.RING), T):
        ring[i & 31] = codes[i][0]
    return ring, T


# ---- prefix cache --------------------------------------------------------------------------------------------------------
def prefix_move_ref(kc, vc, pool, states, h, ssq, slot, entry, n_rows, h_row, restore):
    """PrefixMoveArgs on kc / vc [layer][slot][head][n_ctx][128], pool [entry][layer][2][head][max_rows][128], states
    [entry][H + H/16], h [rows][H], ssq [rows][H/16]: rows [0, n_rows) of K and V of every layer and head, and row h_row
    of h / ssq <-> the entry's state, slot -> entry (restore 0) or entry -> slot (1).  -> copies after the move."""
    kc, vc, pool, states, h, ssq = (np.array(a, copy=True) for a in (kc, vc, pool, states, h, ssq))
    H = h.shape[1]
    if restore:
        kc[:, slot, :, :n_rows] = pool[entry, :, 0, :, :n_rows]
        vc[:, slot, :, :n_rows] = pool[entry, :, 1, :, :n_rows]
        h[h_row] = states[entry, :H]
        ssq[h_row] = states[entry, H:]
    else:
        pool[entry, :, 0, :, :n_rows] = kc[:, slot, :, :n_rows]
        pool[entry, :, 1, :, :n_rows] = vc[:, slot, :, :n_rows]
        states[entry, :H] = h[h_row]
        states[entry, H:] = ssq[h_row]
    return kc, vc, pool, states, h, ssq
