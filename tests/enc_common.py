"""Shared by tests/golden/make_mimi_encode_golden.py (which runs transformers' MimiModel.encode on seeded weights and
stores its outputs) and the encoder tests (which rebuild the same weights from the seeds, map them through
weights.state_to_enc and run tests/enc_ref.py and the HIP encoder on them).

Nothing here is model code: the cases' MimiConfig parameters, the clip lengths, the seeded tensor and audio generators
(driven by the (key, shape) list the torch module reports; the list is stored in the fixture so the tests need no
transformers) and the column subset the fixture keeps of long activations."""
from __future__ import annotations

import hashlib

import numpy as np

# ---- the cases ----------------------------------------------------------------------------------------------------
# "mimi":  Mimi's ratios (8, 6, 5, 4) = 1920 samples per frame at reduced widths, window 16 (the longest clip's 21
#          columns at 25 Hz cross it), 20 quantizers of which 16 are kept.
# "other": other ratios (4, 3, 2) and kernel sizes (first 5, last 1), two residual layers (dilations 1 and 2) with conv
#          shortcuts, grouped-query attention (4 heads on 2 k/v heads), 18 quantizers.
# Lengths: 1, 1919, 1920, 1921 samples (the frame edges) and ones whose 25 Hz column count is odd (the replicate right
# edge of the downsample): 1 and 1921 in both cases, 2000 in "other".
CASES = {
    "mimi": dict(seed=501, lengths=(1, 1919, 1920, 1921, 5000, 20000), stage_clip=5,
                 cfg=dict(num_filters=32, upsampling_ratios=[8, 6, 5, 4], hidden_size=64, num_hidden_layers=2,
                          num_attention_heads=4, num_key_value_heads=4, intermediate_size=96, sliding_window=16,
                          codebook_size=64, codebook_dim=16, vector_quantization_hidden_dimension=16, num_quantizers=20,
                          num_semantic_quantizers=1, frame_rate=12.5, upsample_groups=64)),
    "other": dict(seed=502, lengths=(1, 1919, 1920, 1921, 2000), stage_clip=4,
                  cfg=dict(num_filters=32, upsampling_ratios=[4, 3, 2], kernel_size=5, last_kernel_size=1,
                           residual_kernel_size=3, num_residual_layers=2, dilation_growth_rate=2, use_conv_shortcut=True,
                           hidden_size=48, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                           intermediate_size=64, sliding_window=6, codebook_size=32, codebook_dim=8,
                           vector_quantization_hidden_dimension=8, num_quantizers=18, num_semantic_quantizers=1,
                           frame_rate=500.0, upsample_groups=48)),
}
N_Q = 16


def _rng(seed: int, key: str) -> np.random.Generator:
    h = hashlib.sha256(f"{seed}:{key}".encode()).digest()
    return np.random.default_rng(int.from_bytes(h[:8], "little"))


def seeded_tensor(seed: int, key: str, shape) -> np.ndarray:
    """One tensor of a MimiModel state dict.  Every vector that scales or shifts something is random (LayerNorm weight
    and bias, layer scales, cluster usage with one entry below the 1e-5 clamp) so that a misplaced one changes the
    codes; matrices keep activations O(1); codebooks sit at the scale of the residual they quantise."""
    r = _rng(seed, key)
    shape = tuple(int(x) for x in shape)
    n = lambda: r.standard_normal(shape).astype(np.float32)
    if key.endswith("initialized"):
        return np.ones(shape, np.float32)
    if key.endswith("cluster_usage"):
        u = (0.5 + r.random(shape)).astype(np.float32)
        u.flat[3 % u.size] = 1e-7            # below the clamp: embed = embed_sum / 1e-5 there
        return u
    if key.endswith("embed_sum"):
        e = (0.6 / np.sqrt(shape[1]) * n()).astype(np.float32)
        e[3 % e.shape[0]] *= 1e-5            # the row whose usage is clamped stays O(1) after the division
        return e
    if key.endswith("layer_scale.scale"):
        return (0.2 + 0.3 * r.random(shape)).astype(np.float32)
    if "layernorm.weight" in key:
        return (1.0 + 0.2 * n()).astype(np.float32)
    if key.endswith("bias"):
        return (0.1 * n() if "layernorm" in key else 0.05 * n()).astype(np.float32)
    if key.endswith("weight") and len(shape) >= 2:
        fan_in = int(np.prod(shape[1:]))
        gain = 1.2
        if ".block.3." in key:
            gain = 0.5
        if "mlp.fc2" in key or "o_proj" in key:
            gain = 0.8
        if "upsample" in key:                # ConvTranspose1d [cin, cout / groups, k] of the decode half
            fan_in = int(shape[1] * shape[2])
        return (gain * n() / np.sqrt(fan_in)).astype(np.float32)
    raise KeyError(f"seeded_tensor: no rule for {key} {shape}")


def seeded_state(seed: int, key_shapes) -> dict:
    return {k: seeded_tensor(seed, k, shp) for k, shp in key_shapes}


def digest(state: dict) -> str:
    h = hashlib.sha256()
    for k in sorted(state):
        h.update(k.encode())
        h.update(np.ascontiguousarray(state[k]).tobytes())
    return h.hexdigest()


def seeded_clip(seed: int, n: int) -> np.ndarray:
    """Speech-like test audio: a few drifting partials + noise, amplitude ~0.3, float32."""
    r = _rng(seed, f"clip{n}")
    t = np.arange(n) / 24000.0
    x = np.zeros(n)
    for _ in range(4):
        f0, df, a = 80 + 600 * r.random(), 200 * (r.random() - 0.5), 0.1 * r.random()
        x += a * np.sin(2 * np.pi * (f0 * t + 0.5 * df * t * t) + 6.28 * r.random())
    x += 0.03 * r.standard_normal(n)
    return x.astype(np.float32)


def column_subset(L: int) -> np.ndarray:
    """Columns of a long activation that the fixture keeps: both ends + a sparse comb."""
    if L <= 64:
        return np.arange(L)
    return np.unique(np.concatenate([np.arange(24), np.arange(24, L - 24, 97), np.arange(L - 24, L)]))


def mimi_config_dict(case: dict) -> dict:
    """What weights.state_to_enc reads of the case's MimiConfig (the fixture stores MimiConfig.to_dict() too)."""
    return dict(case["cfg"])
