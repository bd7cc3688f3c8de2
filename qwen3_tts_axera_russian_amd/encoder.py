"""Host side of the speech-tokenizer encoder (include/qwen3tts_enc.h): 24 kHz mono audio -> [frames][16] codec ids.

Stands where the reference's scripts/encode_reference_audio.py calls qwen_tts's tokenizer on a CPU; the encode runs in
csrc/q3_enc.hip (exact fp32, no CPU path)."""
from __future__ import annotations

import numpy as np

from . import hiplib


class Encoder:
    def __init__(self, weights_path, max_batch=8, max_samples=24000 * 30):
        self.lib = hiplib.load()
        self.h = self.lib.enc_load(str(weights_path).encode(), int(max_batch), int(max_samples))
        if not self.h:
            raise RuntimeError(f"enc_load({weights_path}) failed (no HIP device, or not an encoder container; see the log)")
        self.max_batch, self.max_samples = int(max_batch), int(max_samples)
        self.n_q = self.lib.enc_num_quantizers(self.h)
        self.sample_rate = self.lib.enc_sample_rate(self.h)
        self.samples_per_frame = self.lib.enc_samples_per_frame(self.h)

    def frames(self, n_samples):
        return int(self.lib.enc_frames(self.h, int(n_samples)))

    def encode(self, clips):
        """list of float32 arrays (mono, at sample_rate) -> list of int64 [frames, n_q] (semantic id first), max_batch
        clips per library call.  Each clip gives the same ids alone and in any batch."""
        clips = [np.ascontiguousarray(np.asarray(c, dtype=np.float32).reshape(-1)) for c in clips]
        out = []
        for i in range(0, len(clips), self.max_batch):
            part = clips[i:i + self.max_batch]
            n = np.array([c.size for c in part], np.int32)
            if (n <= 0).any() or (n > self.max_samples).any():
                raise ValueError(f"clip lengths must be in 1..{self.max_samples} samples (got {n.tolist()})")
            pcm = np.concatenate(part)
            mf = max(self.frames(x) for x in n)
            codes = np.empty((len(part), mf, self.n_q), np.int64)
            nf = np.zeros(len(part), np.int32)
            rc = self.lib.enc_encode(self.h, hiplib.fptr(pcm), hiplib.iptr(n), len(part), codes.ctypes.data_as(hiplib.i64p),
                                     mf, hiplib.iptr(nf))
            if rc != 0:
                raise RuntimeError(f"enc_encode failed ({rc}); see the log")
            out += [codes[b, :nf[b]].copy() for b in range(len(part))]
        return out

    def last_ms(self):
        """GPU milliseconds of the last library call"""
        return float(self.lib.enc_last_ms(self.h))

    def close(self):
        if self.h:
            self.lib.enc_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
