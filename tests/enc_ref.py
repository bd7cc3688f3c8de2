"""Independent torch-CPU evaluation of the encoder program (weights.enc_program) -- test infrastructure.

A restatement of the op table's semantics (DESIGN.md "Speech tokenizer encoder") in plain torch ops, one clip at a time,
in float32 or float64.  What pins it: tests/test_mimi_encode_golden.py feeds it the state_dict() of transformers'
MimiModel through weights.state_to_enc and requires every stage stored by tests/golden/make_mimi_encode_golden.py to
<= 1e-5 and every code.  The GPU tests compare the HIP encoder with it."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from qwen3_tts_axera_russian_amd import weights as W


def _rope(z, theta):
    """rotate-half RoPE over the last axis, positions = the columns (axis -2)"""
    L, hd = z.shape[-2], z.shape[-1]
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    ang = (torch.arange(L, dtype=torch.float64)[:, None] * inv[None, :]).to(z.dtype)
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)
    rot = torch.cat([-z[..., hd // 2:], z[..., :hd // 2]], -1)
    return z * cos + rot * sin


def enc_reference(tensors: dict, pcm: np.ndarray, n_ops: int = -1, dtype=torch.float32, stages: dict | None = None):
    """pcm f32 [n] -> codes int64 [frames][n_q] (n_ops < 0), or the activation [C][L] after the first n_ops ops.
    stages: {name: n_ops} -> also returns {name: activation [C][L]} for those op counts."""
    prog = np.asarray(tensors["enc.program"])
    t = lambda n: torch.from_numpy(np.array(tensors[n], dtype=np.float64)).to(dtype)
    x = torch.from_numpy(np.asarray(pcm, dtype=np.float64)).to(dtype)[None, None, :]
    res = None
    want = {v: k for k, v in (stages or {}).items()}
    got = {}
    torch.set_num_threads(8)
    with torch.no_grad():
        for i, row in enumerate(prog):
            if 0 <= n_ops <= i:
                break
            op, p, flags = int(row[0]), f"enc.op{i}.", int(row[5])
            bias = t(p + "bias") if (p + "bias") in tensors else None
            if flags & W.EF_RES_SAVE:
                res = x
            if op in (W.EOP_CONV_IN, W.EOP_CONV):
                k = int(row[3])
                dil = int(row[4]) if op == W.EOP_CONV else 1
                h = F.elu(x) if flags & W.EF_ELU else x
                if flags & W.EF_GELU:
                    h = F.gelu(h)
                y = F.conv1d(F.pad(h, ((k - 1) * dil, 0)), t(p + "weight"), bias, dilation=dil)
                if flags & W.EF_RES_ADD:
                    y = y + res
                if flags & W.EF_TO_RES:
                    res = y
                    continue
                x = y
            elif op == W.EOP_CONV_S:   # MimiConv1d: k - s on the left, the right padded to whole frames
                k, s = int(row[3]), int(row[4])
                L = x.shape[-1]
                extra = math.ceil(L / s) * s - L
                h = F.elu(x) if flags & W.EF_ELU else x
                mode = "replicate" if flags & W.EF_REPLICATE else "constant"
                x = F.conv1d(F.pad(h, (k - s, extra), mode=mode), t(p + "weight"), bias, stride=s)
            elif op == W.EOP_NORM:
                eps = int(row[4]) * 1e-9
                x = F.layer_norm(x.transpose(1, 2), (x.shape[1],), t(p + "weight"), bias, eps).transpose(1, 2)
            elif op == W.EOP_ATTN:
                nh, hd, window, theta = int(row[3]), int(row[4]), int(row[6]), float(row[7])
                L = x.shape[-1]
                q, k_, v = [z.reshape(1, nh, hd, L).transpose(2, 3) for z in x.split(nh * hd, dim=1)]   # [1,nh,L,hd]
                q, k_ = _rope(q, theta), _rope(k_, theta)
                sc = (q @ k_.transpose(2, 3)) / math.sqrt(hd)
                ii, jj = torch.arange(L)[:, None], torch.arange(L)[None, :]
                sc = sc.masked_fill(~((jj <= ii) & (jj > ii - window)), float("-inf"))
                x = (torch.softmax(sc, -1) @ v).transpose(2, 3).reshape(1, nh * hd, L)
            elif op == W.EOP_RVQ:
                return rvq_encode(x[0].numpy(), np.asarray(tensors[p + "codebook"]), int(row[6]))[0], got
            else:
                raise ValueError(f"unknown encoder op {op}")
            if i + 1 in want:
                got[want[i + 1]] = x[0].numpy().copy()
    return x[0].numpy(), got


def rvq_encode(z: np.ndarray, codebook: np.ndarray, n_sem: int, forced: np.ndarray | None = None):
    """Split RVQ encode of z [2 dim][T] (semantic | acoustic projections) in z's dtype (float64 for grading).
    -> (codes int64 [T][n_q], gap [T][n_q] = second-best minus best distance, dist_chosen / dist_best [T][n_q]).
    forced [T][n_q]: the residual of stage q is formed from forced[:, :q] (e.g. the GPU's own ids) and the ratios
    grade those ids."""
    nq, cb, dim = codebook.shape
    dt = z.dtype if z.dtype == np.float64 else np.float32
    E = codebook.astype(dt)
    T = z.shape[1]
    codes = np.zeros((T, nq), np.int64)
    gap = np.zeros((T, nq))
    ratio = np.ones((T, nq))
    r = None
    for q in range(nq):
        if q == 0 or q == n_sem:
            r = (z[:dim] if q == 0 else z[dim:2 * dim]).T.astype(dt).copy()      # [T][dim]
        if dt == np.float64:
            d = np.sqrt(np.maximum(((r[:, None, :] - E[q][None, :, :]) ** 2).sum(-1), 0.0))
        else:   # what MimiEuclideanCodebook.quantize runs
            d = torch.cdist(torch.from_numpy(r)[None], torch.from_numpy(E[q])[None], p=2)[0].numpy()
        idx = d.argmin(1)
        srt = np.sort(d, 1)
        gap[:, q] = srt[:, 1] - srt[:, 0] if cb > 1 else np.inf
        use = idx if forced is None else forced[:, q]
        ratio[:, q] = d[np.arange(T), use] / np.maximum(srt[:, 0], 1e-300)
        codes[:, q] = idx
        r = r - E[q][use]
    return codes, gap, ratio
