"""numpy float64 restatement of the speaker encoder: the log-mel front-end and the ECAPA-TDNN network, from the state
dict's own tensors (torch layout).  Checked against the committed fixture (transformers' ECAPA_TimeDelayNet and torch.stft
in float64) by tests/test_spk_reference.py; no torch, no transformers needed to run it."""
from __future__ import annotations

import numpy as np


def log_mel(pcm, sc, fb):
    """pcm [n] -> float64 [n_mels][frames]: reflect padding, periodic Hann, |DFT| with mag_eps, fb^T, log of the floor-clamped"""
    x = np.asarray(pcm, np.float64)
    xp = np.pad(x, (sc.pad, sc.pad), mode="reflect")
    F = 1 + (xp.size - sc.n_fft) // sc.hop
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(sc.win) / sc.win)
    frames = np.stack([xp[f * sc.hop:f * sc.hop + sc.n_fft] for f in range(F)], axis=0) * win
    spec = np.fft.rfft(frames, axis=1)
    mag = np.sqrt(spec.real ** 2 + spec.imag ** 2 + sc.mag_eps)
    mel = mag @ np.asarray(fb, np.float64)
    return np.log(np.maximum(mel, sc.mel_floor)).T


def _conv_same_reflect(x, w, b, dil):
    """torch Conv1d(padding="same", padding_mode="reflect"): x [cin][L], w [cout][cin][k] -> [cout][L]"""
    cout, cin, k = w.shape
    p = dil * (k - 1) // 2
    xp = np.pad(x, ((0, 0), (p, p)), mode="reflect") if p else x
    L = x.shape[1]
    y = np.zeros((cout, L))
    for j in range(k):
        y += w[:, :, j] @ xp[:, j * dil:j * dil + L]
    return y + b[:, None]


def network(mel, state, sc):
    """mel [n_mels][L] float64 -> dict of every stage (block0.., mfa [C][L]; asp [2 C]; fc [dim])"""
    T = {k: np.asarray(v, np.float64) for k, v in state.items()}
    relu = lambda a: np.maximum(a, 0.0)
    tdnn = lambda x, p, dil=1: relu(_conv_same_reflect(x, T[p + ".conv.weight"], T[p + ".conv.bias"], dil))
    out = {}
    x = tdnn(mel, "blocks.0", sc.dilations[0])
    out["block0"] = x
    feats = []
    nb = len(sc.channels)
    for i in range(1, nb - 1):
        res = x
        h = tdnn(x, f"blocks.{i}.tdnn1")
        parts, prev = [], None
        for j, chunk in enumerate(np.split(h, sc.res2net_scale, axis=0)):
            if j == 0:
                prev = chunk
            elif j == 1:
                prev = tdnn(chunk, f"blocks.{i}.res2net_block.blocks.{j - 1}", sc.dilations[i])
            else:
                prev = tdnn(chunk + prev, f"blocks.{i}.res2net_block.blocks.{j - 1}", sc.dilations[i])
            parts.append(prev)
        h = tdnn(np.concatenate(parts, axis=0), f"blocks.{i}.tdnn2")
        m = h.mean(axis=1)
        m = relu(T[f"blocks.{i}.se_block.conv1.weight"][:, :, 0] @ m + T[f"blocks.{i}.se_block.conv1.bias"])
        g = 1.0 / (1.0 + np.exp(-(T[f"blocks.{i}.se_block.conv2.weight"][:, :, 0] @ m + T[f"blocks.{i}.se_block.conv2.bias"])))
        x = h * g[:, None] + res
        out[f"block{i}"] = x
        feats.append(x)
    x = tdnn(np.concatenate(feats, axis=0), "mfa", sc.dilations[-1])
    out["mfa"] = x
    L = x.shape[1]

    def stats(x, m):
        mean = (m * x).sum(axis=1)
        return mean, np.sqrt(np.maximum((m * (x - mean[:, None]) ** 2).sum(axis=1), 1e-12))
    mean, std = stats(x, np.full((1, L), 1.0 / L))
    a = np.concatenate([x, np.repeat(mean[:, None], L, axis=1), np.repeat(std[:, None], L, axis=1)], axis=0)
    a = np.tanh(relu(T["asp.tdnn.conv.weight"][:, :, 0] @ a + T["asp.tdnn.conv.bias"][:, None]))   # ReLU then tanh: the class has both
    a = T["asp.conv.weight"][:, :, 0] @ a + T["asp.conv.bias"][:, None]
    a = np.exp(a - a.max(axis=1, keepdims=True))
    a /= a.sum(axis=1, keepdims=True)
    mean, std = stats(x, a)
    out["asp"] = np.concatenate([mean, std])
    out["fc"] = T["fc.weight"][:, :, 0] @ out["asp"] + T["fc.bias"]
    return out
