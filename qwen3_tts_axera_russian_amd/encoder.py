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
        self.pcm_calls = 0              # enc_encode_pcm calls so far (a server's id cache shows its hits by it)

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

    def pcm_frames(self, n_in, rate):
        """frames a clip of n_in input frames at `rate` gives through encode_pcm (< 0: refused)"""
        return int(self.lib.enc_pcm_frames(self.h, int(n_in), int(rate)))

    @staticmethod
    def _pcm_payload(clips, channels):
        """numpy int16 / float32 clips [n] or [n][channels] -> (format, frame counts, the interleaved frames concatenated)"""
        channels = int(channels)
        if not clips:
            raise ValueError("no clips")
        arrs = [np.asarray(c) for c in clips]
        dt = arrs[0].dtype
        if dt not in (np.dtype(np.int16), np.dtype(np.float32)) or any(a.dtype != dt for a in arrs):
            raise TypeError("clips are int16 or float32 arrays, one dtype per call")
        for a in arrs:
            if not ((a.ndim == 1 and channels == 1) or (a.ndim == 2 and a.shape[1] == channels)):
                raise ValueError(f"a clip of shape {a.shape} is not [n] (mono) or [n][{channels}]")
        n = np.array([a.shape[0] for a in arrs], np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in arrs]))
        if flat.size == 0:
            flat = np.zeros(1, dt)
        return (0 if dt == np.dtype(np.int16) else 1), n, flat

    def encode_pcm(self, clips, rate, channels=1):
        """PCM as a client has it -> list of int64 [frames, n_q]: numpy int16 or float32 arrays of shape [n] or [n][channels]
        at `rate` Hz, decoded, downmixed and resampled to 24 kHz on the device (enc_encode_pcm: pinned to
        scipy.signal.resample_poly's float64 result, the same ids on every host), max_batch clips per library call."""
        fmt, n, flat = self._pcm_payload(clips, channels)
        channels = int(channels)
        out, at = [], 0
        for i in range(0, len(n), self.max_batch):
            part = n[i:i + self.max_batch]
            fr = [self.pcm_frames(x, rate) for x in part]
            if min(fr) < 0:
                raise ValueError(f"encode_pcm refused a clip of {part.tolist()} frames at {rate} Hz (see the log)")
            mf = max(fr)
            codes = np.empty((len(part), mf, self.n_q), np.int64)
            nf = np.zeros(len(part), np.int32)
            buf = flat[at:at + int(part.sum()) * channels]
            at += int(part.sum()) * channels
            self.pcm_calls += 1
            rc = self.lib.enc_encode_pcm(self.h, buf.ctypes.data, fmt, channels, int(rate),
                                         hiplib.iptr(np.ascontiguousarray(part)), len(part), codes.ctypes.data_as(hiplib.i64p), mf,
                                         hiplib.iptr(nf))
            if rc != 0:
                raise RuntimeError(f"enc_encode_pcm failed ({rc}); see the log")
            out += [codes[b, :nf[b]].copy() for b in range(len(part))]
        return out

    def resample_pcm(self, clips, rate, channels=1):
        """The front-end alone (enc_resample_pcm): the 24 kHz mono float32 samples encode_pcm encodes, bit for bit -> list
        of float32 arrays.  What the speaker encoder embeds, so that both halves of a voice come from one resampler."""
        fmt, n, flat = self._pcm_payload(clips, channels)
        channels = int(channels)
        out, at = [], 0
        for i in range(0, len(n), self.max_batch):
            part = np.ascontiguousarray(n[i:i + self.max_batch])
            buf = flat[at:at + int(part.sum()) * channels]
            at += int(part.sum()) * channels
            pcm = np.zeros((len(part), self.max_samples), np.float32)
            n_out = np.zeros(len(part), np.int32)
            rc = self.lib.enc_resample_pcm(self.h, buf.ctypes.data, fmt, channels, int(rate), hiplib.iptr(part), len(part),
                                           hiplib.fptr(pcm), self.max_samples, hiplib.iptr(n_out))
            if rc != 0:
                raise RuntimeError(f"enc_resample_pcm failed ({rc}); see the log")
            out += [pcm[b, :n_out[b]].copy() for b in range(len(part))]
        return out

    def last_ms(self):
        """GPU milliseconds of the last library call"""
        return float(self.lib.enc_last_ms(self.h))

    def stream(self, max_streams=1, max_push_samples=24000):
        """-> EncoderStream: max_streams clips of any length encoded as their samples arrive (enc_stream_*); close it before
        this encoder."""
        return EncoderStream(self, max_streams, max_push_samples)

    def encode_streaming(self, pcm, push_samples=24000):
        """One clip of any length (max_samples does not bound it) in pushes of push_samples samples -> int64 [frames, n_q]."""
        pcm = np.ascontiguousarray(np.asarray(pcm, dtype=np.float32).reshape(-1))
        push_samples = int(push_samples)
        if push_samples <= 0:
            raise ValueError("push_samples must be positive")
        st = self.stream(1, push_samples)
        try:
            parts = []
            for at in range(0, max(pcm.size, 1), push_samples):
                last = at + push_samples >= pcm.size
                parts.append(st.push([(0, pcm[at:at + push_samples], last)])[0])
            return np.concatenate(parts, axis=0)
        finally:
            st.close()

    def encode_streaming_pcm(self, x, rate, channels=1, push_frames=None, max_push_samples=24000):
        """One clip of any length as a client has it (int16 or float32, [n] or [n][channels], at `rate` Hz) through the
        streaming encode in pushes of push_frames input frames (default and cap: what one push of max_push_samples takes at
        this rate) -> int64 [frames, n_q].  The front-end runs on the device; max_samples does not bound the clip."""
        x = np.asarray(x)
        st = self.stream(1, int(max_push_samples))
        try:
            most = st.pcm_max_frames_in(rate)
            if most < 1:
                raise ValueError(f"encode_streaming_pcm: {rate} Hz is refused, or a push of {max_push_samples} samples is too short for it")
            push = most if push_frames is None else min(int(push_frames), most)
            if push <= 0:
                raise ValueError("push_frames must be positive")
            parts = []
            for at in range(0, max(x.shape[0], 1), push):
                parts.append(st.push_pcm([(0, x[at:at + push], at + push >= x.shape[0])], rate, channels)[0])
            return np.concatenate(parts, axis=0)
        finally:
            st.close()

    def close(self):
        if self.h:
            self.lib.enc_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EncoderStream:
    """The carry-state streaming encode, for up to max_streams clips at once (enc_stream_*): after pushes totalling n samples a
    stream has handed out floor(n / samples_per_frame) frames, and the finishing push brings that to frames(n).  Joined, a
    stream's ids are the same bits whatever the split.  Device memory is fixed at creation, whatever the clips' lengths."""

    def __init__(self, enc, max_streams, max_push_samples):
        self.lib, self.enc = enc.lib, enc
        self.max_streams, self.max_push_samples = int(max_streams), int(max_push_samples)
        self.h = self.lib.enc_stream_create(enc.h, self.max_streams, self.max_push_samples)
        if not self.h:
            raise RuntimeError("enc_stream_create failed (no memory, or a table that cannot be streamed; see the log)")
        self.n_q = enc.n_q
        self.state_bytes = int(self.lib.enc_stream_state_bytes(self.h))    # per stream, constant
        self.last_launches, self.last_ms = 0, 0.0                           # of the last push

    def device_bytes(self):
        """device memory the object holds (fixed at creation)"""
        return int(self.lib.enc_stream_device_bytes(self.h))

    def reset(self, k):
        """stream k starts a new clip"""
        if self.lib.enc_stream_reset(self.h, int(k)) != 0:
            raise RuntimeError("enc_stream_reset failed")

    def push(self, entries):
        """entries: (stream, new samples (float32, 0..max_push_samples of them), finish) -> per entry the int64 [frames, n_q]
        ids the push hands out (possibly 0 frames)."""
        st = np.array([e[0] for e in entries], np.int32)
        new = [np.ascontiguousarray(np.asarray(e[1], dtype=np.float32).reshape(-1)) for e in entries]
        n_new = np.array([x.size for x in new], np.int32)
        fin = np.array([int(bool(e[2])) for e in entries], np.int32)
        pcm = np.concatenate(new + [np.zeros(1, np.float32)])
        cap = int(self.lib.enc_stream_push_max_frames(self.h, len(st), hiplib.iptr(st), hiplib.iptr(n_new), hiplib.iptr(fin)))
        if cap < 0:
            raise RuntimeError("enc_stream_push: invalid push (see the log)")
        codes = np.empty((max(cap, 1), self.n_q), np.int64)
        off = np.zeros(len(st) + 1, np.int64)
        rc = self.lib.enc_stream_push(self.h, len(st), hiplib.iptr(st), hiplib.fptr(pcm), hiplib.iptr(n_new), hiplib.iptr(fin),
                                      codes.ctypes.data_as(hiplib.i64p), cap, off.ctypes.data_as(hiplib.i64p))
        if rc != 0:
            raise RuntimeError(f"enc_stream_push failed ({rc}); see the log")
        self.last_launches = int(self.lib.enc_stream_last_launches(self.h))
        self.last_ms = float(self.lib.enc_stream_last_ms(self.h))
        return [codes[off[i]:off[i + 1]].copy() for i in range(len(st))]

    def pcm_max_frames_in(self, rate):
        """the most input frames one entry of one push_pcm may bring at `rate` (< 0: a rate the front-end refuses)"""
        return int(self.lib.enc_stream_pcm_max_frames_in(self.h, int(rate)))

    def pcm_samples(self, rate, n_in_total, finished=False):
        """24 kHz samples a stream has handed to the encoder after n_in_total input frames at `rate`"""
        return int(self.lib.enc_stream_pcm_samples(self.h, int(rate), int(n_in_total), int(bool(finished))))

    def pcm_device_bytes(self):
        """device memory of the PCM front-end (carry rows; 0 until the first push_pcm, constant after it)"""
        return int(self.lib.enc_stream_pcm_device_bytes(self.h))

    def push_pcm(self, entries, rate, channels=1):
        """push() for PCM as a client has it: entries (stream, int16 or float32 array [n] or [n][channels] at `rate` Hz, finish),
        one dtype per call, at most pcm_max_frames_in(rate) frames each.  Decoded, downmixed and resampled on the device
        (enc_stream_push_pcm): joined, a stream's samples are the bits Encoder.encode_pcm prepares for the whole clip, whatever
        the split.  Returns what push returns."""
        channels = int(channels)
        st = np.array([e[0] for e in entries], np.int32)
        fin = np.array([int(bool(e[2])) for e in entries], np.int32)
        fmt, n_in, flat = Encoder._pcm_payload([e[1] for e in entries], channels)
        args = (self.h, len(st), hiplib.iptr(st))
        cap = int(self.lib.enc_stream_push_pcm_max_frames(*args, fmt, channels, int(rate), hiplib.iptr(n_in), hiplib.iptr(fin)))
        if cap < 0:
            raise RuntimeError("enc_stream_push_pcm: invalid push (see the log)")
        codes = np.empty((max(cap, 1), self.n_q), np.int64)
        off = np.zeros(len(st) + 1, np.int64)
        rc = self.lib.enc_stream_push_pcm(*args, flat.ctypes.data, fmt, channels, int(rate), hiplib.iptr(n_in), hiplib.iptr(fin),
                                          codes.ctypes.data_as(hiplib.i64p), cap, off.ctypes.data_as(hiplib.i64p))
        if rc != 0:
            raise RuntimeError(f"enc_stream_push_pcm failed ({rc}); see the log")
        self.last_launches = int(self.lib.enc_stream_last_launches(self.h))
        self.last_ms = float(self.lib.enc_stream_last_ms(self.h))
        return [codes[off[i]:off[i + 1]].copy() for i in range(len(st))]

    def close(self):
        if self.h:
            self.lib.enc_stream_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
