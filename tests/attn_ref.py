"""Float64 restatement of the attention numerics contract (csrc/q3_kernels.h, DESIGN.md "Numerics"), numpy only.

Talker / code-predictor attention (launch_attn: 16 q heads, 8 kv heads, head_dim 128):
  * per-head RMSNorm of q and of k with their weights (q_norm / k_norm), then rotate-half RoPE on the pairs
    (i, i + 64) with the f32 cos / sin tables the kernels are given;
  * the new K / V rows are rounded to fp16 (saturating) into the cache; q stays in full precision;
  * GQA: q head h reads kv head h // 2, causal over the cache rows 0 .. pos of the row's slot;
  * the output is rounded to fp16 (saturating).

The sliding-window attention of the vocoder (voc_attention) is the op oracle/voc_ref.py pins: RoPE over the columns
of the chunk (inv_freq = theta^(-2j/D), pairs (j, j + D/2)), keys i - window < t <= i, scale 1/sqrt(D).

tests/test_attn_reference.py pins the talker form to transformers' Qwen3 attention; tests/test_gpu_attention.py grades
every kernel variant against both."""
from __future__ import annotations

import numpy as np

NH, NKV, D = 16, 8, 128
LD = (NH + 2 * NKV) * D        # one qkv row: q heads, then k heads, then v heads
OW = NH * D                    # one output row


def rope_tables(max_pos: int, theta: float = 1e6) -> tuple[np.ndarray, np.ndarray]:
    """f32 [max_pos][64] cos / sin tables computed like the model loader (q3_model.hip): f32 inv_freq and angles."""
    i = np.arange(D // 2, dtype=np.float32)
    inv = (np.float32(1.0) / np.power(np.float32(theta), (2 * i) / np.float32(D))).astype(np.float32)
    ang = (np.arange(max_pos, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def f16_sat(x) -> np.ndarray:
    """fp16 rounding with saturation to +-65504 (sat_half)."""
    return np.clip(np.asarray(x, np.float64), -65504.0, 65504.0).astype(np.float16)


def prep(qkv, q_norm, k_norm, eps, cos, sin, pos):
    """Phase A of every variant for rows qkv[R][4096] at positions pos[R]: -> q [R][16][128], k, v [R][8][128] (float64,
    k / v before their fp16 rounding)."""
    x = np.asarray(qkv, np.float64)
    R = x.shape[0]
    q = x[:, :NH * D].reshape(R, NH, D)
    k = x[:, NH * D:(NH + NKV) * D].reshape(R, NKV, D)
    v = x[:, (NH + NKV) * D:].reshape(R, NKV, D)
    c = np.asarray(cos, np.float64)[pos][:, None, :]
    s = np.asarray(sin, np.float64)[pos][:, None, :]

    def norm_rope(h, w):
        h = h / np.sqrt((h * h).mean(-1, keepdims=True) + eps) * np.asarray(w, np.float64)
        h0, h1 = h[..., :D // 2], h[..., D // 2:]
        return np.concatenate([h0 * c - h1 * s, h1 * c + h0 * s], -1)

    return norm_rope(q, q_norm), norm_rope(k, k_norm), v


def write_cache(kc, vc, k, v, slot, pos):
    """The cache after the rows' appends: copies of kc / vc with row (slot[r], :, pos[r]) = fp16(k[r]) / fp16(v[r])."""
    kc, vc = kc.copy(), vc.copy()
    for r in range(len(slot)):
        kc[slot[r], :, pos[r]] = f16_sat(k[r])
        vc[slot[r], :, pos[r]] = f16_sat(v[r])
    return kc, vc


def attend(q, kc, vc, slot, pos):
    """Causal GQA attention of rows q[R][16][128] over cache rows 0 .. pos[r] of slot[r] -> (out [R][2048] float64, before
    the fp16 rounding; vmax [R] = max |V| over the rows each output reads)."""
    R = q.shape[0]
    out = np.zeros((R, OW))
    vmax = np.zeros(R)
    scale = 1.0 / np.sqrt(D)
    # rows of one slot share their keys: one product per (slot, kv head) with a causal mask
    for s in sorted(set(int(x) for x in slot)):
        rows = np.array([r for r in range(R) if slot[r] == s])
        T = int(max(pos[r] for r in rows)) + 1
        K = kc[s, :, :T].astype(np.float64)          # [8][T][128]
        V = vc[s, :, :T].astype(np.float64)
        p = np.asarray([pos[r] for r in rows])
        mask = np.arange(T)[None, :] <= p[:, None]    # [n][T]
        absV = np.abs(V).max(-1).max(0)               # [T]
        for i, r in enumerate(rows):
            vmax[r] = absV[:p[i] + 1].max()
        for h in range(NH):
            g = h // 2
            sc = (q[rows, h] @ K[g].T) * scale        # [n][T]
            sc = np.where(mask, sc, -np.inf)
            w = np.exp(sc - sc.max(-1, keepdims=True))
            out[rows, h * D:(h + 1) * D] = (w @ V[g]) / w.sum(-1, keepdims=True)
    return out, vmax


def row_layout(R, row0, slot=None, pos=None, slot_base=0, slot_stride=0, pos_base=0, pos_stride=0, valid_mod=0,
               valid_n=0):
    """(slot, pos, active) of rows row0 .. row0+R-1 as launch_attn reads them (null arrays: *_base + r * *_stride with r
    the absolute row; rows with r % valid_mod >= valid_n are padding)."""
    r = np.arange(row0, row0 + R)
    sl = np.asarray(slot, np.int64) if slot is not None else slot_base + r * slot_stride
    ps = np.asarray(pos, np.int64) if pos is not None else pos_base + r * pos_stride
    active = np.ones(R, bool) if valid_mod <= 0 else (r % valid_mod) < valid_n
    return sl, ps, active


def output_rows(R, row0, sl, ps, active, tiles=None, n_tiles=0, slot_base=0, pos_base=0):
    """Which rows an ATTEND / FUSED call writes and the (slot, last key) each reads -> list of (row index 0..R-1, slot, pos).
    Explicit tiles {first row, rows, slot, first position}: tile row i reads pos0 + i; tiles == None with n_tiles > 0: one
    run of slot_base from pos_base; otherwise every active row reads its own (slot, pos)."""
    if tiles is not None:
        return [(t0 + i - row0, s, p0 + i) for t0, n, s, p0 in np.asarray(tiles).reshape(-1, 4) for i in range(n)]
    if n_tiles > 0:
        return [(i, slot_base, pos_base + i) for i in range(R)]
    return [(i, int(sl[i]), int(ps[i])) for i in range(R) if active[i]]


def voc_attention(x, H, Dh, window, theta):
    """x [B][3*H*Dh][L] (q | k | v head-major rows) -> y [B][H*Dh][L], float64."""
    x = np.asarray(x, np.float64)
    B, _, L = x.shape
    q, k, v = [z.reshape(B, H, Dh, L).transpose(0, 1, 3, 2) for z in np.split(x, 3, axis=1)]   # [B][H][L][Dh]
    inv = theta ** (-np.arange(0, Dh, 2, dtype=np.float64) / Dh)
    ang = np.arange(L, dtype=np.float64)[:, None] * inv[None, :]
    c, s = np.cos(ang), np.sin(ang)

    def rope(z):
        z0, z1 = z[..., :Dh // 2], z[..., Dh // 2:]
        return np.concatenate([z0 * c - z1 * s, z1 * c + z0 * s], -1)

    q, k = rope(q), rope(k)
    sc = q @ k.transpose(0, 1, 3, 2) / np.sqrt(Dh)
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    sc = np.where((j <= i) & (j > i - window), sc, -np.inf)
    w = np.exp(sc - sc.max(-1, keepdims=True))
    o = (w @ v) / w.sum(-1, keepdims=True)
    return o.transpose(0, 1, 3, 2).reshape(B, H * Dh, L)
