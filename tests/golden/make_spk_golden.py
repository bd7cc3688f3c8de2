"""Writes tests/golden/spk_golden.npz: transformers' ECAPA_TimeDelayNet (models/qwen2_5_omni) in float64 on the seeded
weights of tests/spk_common.py, fed by the float64 log-mel of torch.stft + transformers' slaney filter bank.

    python -m tests.golden.make_spk_golden

Per case and clip length n: `<case>.mel<n>` (rows x columns subsets of spk_common), every stage `<case>.<stage><n>`, the
embedding (`fc`), the scale of each full activation (`<case>.<stage><n>.scale`, max |value|) and `<case>.err32`
[clips][stages + 1]: the float32 forward (mel included, computed in float32 too) against the float64 one, over each
stage's scale.  Only outputs are stored: the tests regenerate weights and clips from the seeds (`<case>.sha`)."""
from __future__ import annotations

import os

import numpy as np
import torch

from tests import spk_common as C

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spk_golden.npz")


def torch_log_mel(x, sc, fb, dtype):
    x = torch.as_tensor(np.asarray(x), dtype=dtype)
    xp = torch.nn.functional.pad(x[None, None], (sc.pad, sc.pad), mode="reflect")[0, 0]
    win = torch.hann_window(sc.win, periodic=True, dtype=dtype)
    spec = torch.stft(xp, sc.n_fft, hop_length=sc.hop, win_length=sc.win, window=win, center=False, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + sc.mag_eps)
    mel = torch.as_tensor(fb, dtype=dtype).T @ mag
    return torch.log(torch.clamp(mel, min=sc.mel_floor))   # [n_mels][frames]


def build_module(sc, state, dtype):
    from transformers.models.qwen2_5_omni.configuration_qwen2_5_omni import Qwen2_5OmniDiTConfig
    from transformers.models.qwen2_5_omni.modeling_qwen2_5_omni import ECAPA_TimeDelayNet
    cfg = Qwen2_5OmniDiTConfig(mel_dim=sc.n_mels, enc_dim=sc.dim, enc_channels=list(sc.channels),
                               enc_kernel_sizes=list(sc.kernel_sizes), enc_dilations=list(sc.dilations),
                               enc_attention_channels=sc.attention_channels, enc_res2net_scale=sc.res2net_scale,
                               enc_se_channels=sc.se_channels)
    m = ECAPA_TimeDelayNet(cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in C.W.spk_state_shapes(sc)]
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return m.to(dtype).eval()


def run_stages(m, mel):
    """mel [n_mels][L] -> {stage: ndarray} through forward hooks (the module takes [B][L][mel])"""
    got = {}
    hooks = []
    for i, blk in enumerate(m.blocks):
        hooks.append(blk.register_forward_hook(lambda mod, a, o, i=i: got.__setitem__(f"block{i}", o[0])))
    hooks.append(m.mfa.register_forward_hook(lambda mod, a, o: got.__setitem__("mfa", o[0])))
    hooks.append(m.asp.register_forward_hook(lambda mod, a, o: got.__setitem__("asp", o[0, :, 0])))
    with torch.no_grad():
        got["fc"] = m(mel.T[None])[0]
    for h in hooks:
        h.remove()
    return {k: v.detach().numpy() for k, v in got.items()}


def main():
    out = {}
    for name, case in C.CASES.items():
        sc = case["sc"]
        state = C.state(name)
        out[f"{name}.sha"] = np.frombuffer(C.digest(state).encode(), np.uint8)
        fb = C.W.spk_mel_filter_bank(sc)
        m64, m32 = build_module(sc, state, torch.float64), build_module(sc, state, torch.float32)
        err32 = np.zeros((len(case["lengths"]), len(C.STAGES) + 1))
        for ci, n in enumerate(case["lengths"]):
            clip = C.seeded_clip(case["seed"], n)
            mel64, mel32 = torch_log_mel(clip, sc, fb, torch.float64), torch_log_mel(clip, sc, fb, torch.float32)
            s64, s32 = run_stages(m64, mel64), run_stages(m32, mel32)
            mel = mel64.numpy()
            cols = C.column_subset(mel.shape[1])
            out[f"{name}.mel{n}"] = mel[np.ix_(C.row_subset(mel.shape[0]), cols)]
            out[f"{name}.mel{n}.scale"] = np.float64(np.abs(mel).max())
            err32[ci, 0] = np.abs(mel32.numpy().astype(np.float64) - mel).max() / np.abs(mel).max()
            for si, st in enumerate(C.STAGES):
                a = s64[st]
                scale = float(np.abs(a).max())
                out[f"{name}.{st}{n}"] = a[np.ix_(C.row_subset(a.shape[0]), cols)] if a.ndim == 2 else a
                out[f"{name}.{st}{n}.scale"] = np.float64(scale)
                err32[ci, si + 1] = np.abs(s32[st].astype(np.float64) - a).max() / scale
            print(name, n, "frames", mel.shape[1], "err32", " ".join(f"{e:.1e}" for e in err32[ci]), flush=True)
        out[f"{name}.err32"] = err32
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
