"""Shared by tests/golden/make_spk_golden.py (which runs transformers' ECAPA_TimeDelayNet in float64 on seeded weights,
and float64 torch.stft + the slaney filter bank, and stores their outputs) and the speaker-encoder tests (which rebuild the
same weights and clips from the seeds, map them through weights.convert_speaker_encoder and run tests/spk_ref.py and the
HIP library on them).

Nothing here is model code: the cases' geometries, the clip lengths, the seeded audio generator and the row / column
subsets the fixture keeps of the activations.  The weights come from weights.synthetic_spk_state (torch's default Conv1d
scale); their digest is stored in the fixture."""
from __future__ import annotations

import hashlib

import numpy as np

from qwen3_tts_axera_russian_amd import weights as W

# ---- the cases ----------------------------------------------------------------------------------------------------
# "tiny": n_fft 64 / hop 16 / pad 24 / 16 mels, channels 32/32/32/32/96, scale 4, SE 8, attention 8, dim 32.
# "full": the recollected checkpoint geometry (weights.SpkConfig), dim 1024.
# Lengths: the minimum (5 frames: reflect pad 4 on 5 columns), minimum + hop (6 frames), a non-multiple of the hop, and --
# full only -- 10 s.
CASES = {
    "tiny": dict(seed=701, sc=W.tiny_spk_config(), lengths=(80, 96, 1501)),
    "full": dict(seed=702, sc=W.SpkConfig(), lengths=(1280, 1536, 24017, 240000)),
}
STAGES = ("block0", "block1", "block2", "block3", "mfa", "asp", "fc")   # q3t_spk_stage's indices 0..6 at these geometries


def _rng(seed: int, key: str) -> np.random.Generator:
    h = hashlib.sha256(f"{seed}:{key}".encode()).digest()
    return np.random.default_rng(int.from_bytes(h[:8], "little"))


def seeded_clip(seed: int, n: int) -> np.ndarray:
    """Speech-like test audio inside [-1, 1]: a few drifting partials + noise, float32."""
    r = _rng(seed, f"spkclip{n}")
    t = np.arange(n) / 24000.0
    x = np.zeros(n)
    for _ in range(5):
        f0, df, a = 90 + 2500 * r.random() ** 2, 300 * (r.random() - 0.5), 0.05 + 0.15 * r.random()
        x += a * np.sin(2 * np.pi * (f0 * t + 0.5 * df * t * t) + 6.28 * r.random())
    x += 0.04 * r.standard_normal(n)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def state(name: str) -> dict:
    """the case's ECAPA_TimeDelayNet state dict (float32 values)"""
    c = CASES[name]
    return W.synthetic_spk_state(c["sc"], c["seed"])


def digest(st: dict) -> str:
    h = hashlib.sha256()
    for k in sorted(st):
        h.update(k.encode())
        h.update(np.ascontiguousarray(st[k]).tobytes())
    return h.hexdigest()


def column_subset(L: int) -> np.ndarray:
    """Columns of an activation the fixture keeps: both ends (where the reflection acts) + a few inside."""
    if L <= 16:
        return np.arange(L)
    return np.unique(np.concatenate([np.arange(5), np.linspace(5, L - 6, 4).astype(int), np.arange(L - 5, L)]))


def row_subset(C: int) -> np.ndarray:
    """Channels the fixture keeps: all of a narrow activation, a comb of a wide one."""
    return np.arange(C) if C <= 128 else np.arange(0, C, 7)


def write_container(name: str, path: str):
    """the case's weights as a container for spk_load -> SpkConfig"""
    c = CASES[name]
    st = {"speaker_encoder." + k: v for k, v in state(name).items()}
    sc, meta, t = W.convert_speaker_encoder(st, sc=c["sc"], verbose=False)
    assert sc == c["sc"]
    W.write_pack(path, meta, t)
    return sc
