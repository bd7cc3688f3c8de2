"""Host side of the speaker encoder (include/qwen3tts_spk.h): 24 kHz mono audio -> one x-vector [dim] per clip.

The second half of a cloned voice (the first: the codec prompt, encoder.py): the embedding goes into the prefix as one row
(frontend.py, build_prefix(..., speaker=)).  The embed runs in csrc/q3_spk.hip (float64 log-mel, exact-fp32 network, no
CPU path).  Pinned to transformers' ECAPA_TimeDelayNet by fixtures; that a TTS checkpoint's speaker encoder is that class
at this geometry, its mel parameters and the row's position are recollection.  No similarity claim."""
from __future__ import annotations

import numpy as np

from . import hiplib


class SpeakerEncoder:
    def __init__(self, weights_path, max_batch=8, max_samples=24000 * 30):
        self.lib = hiplib.load()
        self.h = self.lib.spk_load(str(weights_path).encode(), int(max_batch), int(max_samples))
        if not self.h:
            raise RuntimeError(f"spk_load({weights_path}) failed (no HIP device, or not a speaker-encoder container; see the log)")
        self.max_batch, self.max_samples = int(max_batch), int(max_samples)
        self.dim = self.lib.spk_dim(self.h)
        self.sample_rate = self.lib.spk_sample_rate(self.h)
        self.min_samples = self.lib.spk_min_samples(self.h)
        self.calls = 0                  # spk_embed calls so far (a server's cache shows its hits by it)

    def frames(self, n_samples):
        """log-mel frames a clip gives (< 0: refused -- too short for the reflect padding or for the network)"""
        return int(self.lib.spk_frames(self.h, int(n_samples)))

    def embed(self, clips):
        """list of float32 arrays (mono, at sample_rate) -> float32 [len(clips)][dim], max_batch clips per library call.
        Each clip gives the same bits alone and in any batch."""
        clips = [np.ascontiguousarray(np.asarray(c, dtype=np.float32).reshape(-1)) for c in clips]
        out = np.empty((len(clips), self.dim), np.float32)
        for i in range(0, len(clips), self.max_batch):
            part = clips[i:i + self.max_batch]
            n = np.array([c.size for c in part], np.int32)
            if (n < self.min_samples).any() or (n > self.max_samples).any():
                raise ValueError(f"clip lengths must be in {self.min_samples}..{self.max_samples} samples (got {n.tolist()})")
            pcm = np.concatenate(part)
            emb = np.empty((len(part), self.dim), np.float32)
            self.calls += 1
            rc = self.lib.spk_embed(self.h, hiplib.fptr(pcm), hiplib.iptr(n), len(part), hiplib.fptr(emb))
            if rc != 0:
                raise RuntimeError(f"spk_embed failed ({rc}); see the log")
            out[i:i + len(part)] = emb
        return out

    def last_ms(self):
        """GPU milliseconds of the last spk_embed"""
        return float(self.lib.spk_last_ms(self.h))

    def last_launches(self):
        return int(self.lib.spk_last_launches(self.h))

    def close(self):
        if self.h:
            self.lib.spk_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
