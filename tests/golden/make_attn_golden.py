#!/usr/bin/env python3
"""Generate tests/golden/attn_hf_golden.npz: transformers' Qwen3 attention (Qwen3RMSNorm on the q / k heads,
Qwen3RotaryEmbedding + apply_rotary_pos_emb, eager GQA attention with a causal mask) on seeded inputs, in float32.

The model's shape: 16 q heads, 8 kv heads, head_dim 128, rms_norm_eps 1e-6, rope_theta 1e6.  Every case is a causal
sequence of N rows whose RoPE positions start at `offset` (up to 4095); the q / k norm weights are random so that a norm
applied to the wrong operand, or after RoPE, changes the answer.  Stored per case: the rope tables HF used (cos / sin,
first half of the head), the attention output [N][16 * 128] before o_proj.  The inputs are regenerated from the seed
(make_inputs) and guarded by a digest.

tests/test_attn_reference.py asserts tests/attn_ref.py reproduces these outputs.

Usage:  python tests/golden/make_attn_golden.py      (needs transformers + torch; runs on CPU in a few seconds)
"""
import hashlib
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_hf_golden.npz")
CASES = [("start", 0, 20), ("mid", 977, 20), ("end", 4076, 20)]     # (name, first position, rows)
NH, NKV, D, EPS, THETA = 16, 8, 128, 1e-6, 1e6


def make_inputs(seed=20261016):
    """-> {name: (qkv [N][4096] f32, q_norm [128], k_norm [128], positions [N])} and a digest of them."""
    r = np.random.default_rng(seed)
    out, h = {}, hashlib.sha256()
    for name, off, n in CASES:
        qkv = r.standard_normal((n, (NH + 2 * NKV) * D)).astype(np.float32)
        qkv[:, :NH * D] *= 2.0
        q_norm = (1.0 + 0.25 * r.standard_normal(D)).astype(np.float32)
        k_norm = (1.0 + 0.25 * r.standard_normal(D)).astype(np.float32)
        pos = np.arange(off, off + n)
        out[name] = (qkv, q_norm, k_norm, pos)
        for a in (qkv, q_norm, k_norm, pos):
            h.update(np.ascontiguousarray(a).tobytes())
    return out, h.hexdigest()


def hf_attention(qkv, q_norm, k_norm, pos):
    """transformers' Qwen3 attention core -> (out [N][2048], cos [N][64], sin [N][64]) as float32 numpy."""
    import torch
    from transformers import Qwen3Config
    from transformers.models.qwen3.modeling_qwen3 import (Qwen3RMSNorm, Qwen3RotaryEmbedding, apply_rotary_pos_emb,
                                                          eager_attention_forward)
    cfg = Qwen3Config(hidden_size=1024, num_attention_heads=NH, num_key_value_heads=NKV, head_dim=D, rms_norm_eps=EPS,
                      rope_theta=THETA, max_position_embeddings=32768)
    n = qkv.shape[0]
    x = torch.from_numpy(qkv)
    q = x[:, :NH * D].reshape(1, n, NH, D)
    k = x[:, NH * D:(NH + NKV) * D].reshape(1, n, NKV, D)
    v = x[:, (NH + NKV) * D:].reshape(1, n, NKV, D)
    qn, kn = Qwen3RMSNorm(D, eps=EPS), Qwen3RMSNorm(D, eps=EPS)
    qn.weight.data = torch.from_numpy(q_norm)
    kn.weight.data = torch.from_numpy(k_norm)
    q, k, v = qn(q).transpose(1, 2), kn(k).transpose(1, 2), v.transpose(1, 2)     # [1][heads][n][D]
    rot = Qwen3RotaryEmbedding(cfg)
    cos, sin = rot(v, torch.from_numpy(pos)[None])
    q, k = apply_rotary_pos_emb(q, k, cos, sin)
    mask = torch.full((n, n), float("-inf")).triu(1)[None, None]
    mod = torch.nn.Module()
    mod.num_key_value_groups = NH // NKV
    mod.training = False
    o, _ = eager_attention_forward(mod, q, k, v, mask, scaling=D ** -0.5)       # [1][n][heads][D]
    return (o.reshape(n, NH * D).numpy().astype(np.float32), cos[0, :, :D // 2].numpy().astype(np.float32),
            sin[0, :, :D // 2].numpy().astype(np.float32))


def main():
    import torch
    with torch.no_grad():
        inputs, digest = make_inputs()
        arrays = {"inputs_sha256": np.frombuffer(digest.encode(), np.uint8)}
        for name, (qkv, qn, kn, pos) in inputs.items():
            o, c, s = hf_attention(qkv, qn, kn, pos)
            arrays[f"{name}_out"], arrays[f"{name}_cos"], arrays[f"{name}_sin"] = o, c, s
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
