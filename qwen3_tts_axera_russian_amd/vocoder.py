"""Host side of the vocoder (include/qwen3tts_voc.h): codec ids [frames][16] -> 24 kHz waveform.  voc_set_exact_fp32 and
voc_set_max_workgroups act on the whole process, not on one handle: they stay plain library calls.  They may be made from any
thread and take effect from the next call on: a decode in flight finishes under the settings it started with."""
from __future__ import annotations

import numpy as np

from . import hiplib


def _cat(codes_list):
    """utterances' frames -> contiguous int64 [sum n][16]"""
    return np.ascontiguousarray(np.concatenate([np.asarray(c, np.int64).reshape(-1, 16) for c in codes_list]
                                               + [np.zeros((0, 16), np.int64)]))


def _packed(fn, args, n, cap, int16):
    """fn(*args, out, cap, offsets), an entry point with packed output -> its n arrays out[offsets[i]:offsets[i + 1]]"""
    out = np.empty(max(cap, 1), np.int16 if int16 else np.float32)
    off = np.zeros(n + 1, np.int64)
    if fn(*args, out.ctypes.data_as(hiplib.i16p if int16 else hiplib.f32p), cap, off.ctypes.data_as(hiplib.i64p)) != 0:
        raise RuntimeError(f"{fn.__name__} failed")
    return [out[off[i]:off[i + 1]] for i in range(n)]


class Vocoder:
    def __init__(self, weights, chunk_tokens=64, max_batch=1):
        self.lib = hiplib.load()
        self.h = self.lib.voc_load(str(weights).encode(), int(chunk_tokens), int(max_batch))
        if not self.h:
            raise RuntimeError(f"voc_load({weights}) failed (no HIP device, or no vocoder program; see the log)")
        self.chunk_tokens = self.lib.voc_chunk_tokens(self.h)
        self.chunk_samples = self.lib.voc_chunk_samples(self.h)     # one decode's output (<= chunk_tokens * samples_per_token)
        self.samples_per_token = self.lib.voc_samples_per_token(self.h)
        self._streams = []
        self._incr1 = {}                 # synthesize_incremental's one-stream object per arithmetic

    def decode(self, codes):
        """codes [B][chunk_tokens][16] -> f32 [B][chunk_samples] (the reference's ONNX call, vocoder_server.py:67-71)"""
        c = np.ascontiguousarray(codes, np.int64)
        out = np.empty((c.shape[0], self.chunk_samples), np.float32)
        if self.lib.voc_decode(self.h, c.ctypes.data_as(hiplib.i64p), c.shape[0], hiplib.fptr(out)) != 0:
            raise RuntimeError("voc_decode failed")
        return out

    def synthesize(self, codes, int16=False):
        """codes [n][16] -> VocoderServer.synthesize (vocoder_server.py:73-121): f32, or int16 by the reference's rule"""
        c = _cat([codes])
        out = np.empty(self.lib.voc_synthesize_max_samples(self.h, len(c)), np.int16 if int16 else np.float32)
        ns = np.zeros(1, np.int32)
        fn, p = (self.lib.voc_synthesize, hiplib.i16p) if int16 else (self.lib.voc_synthesize_f32, hiplib.f32p)
        if fn(self.h, c.ctypes.data_as(hiplib.i64p), len(c), out.ctypes.data_as(p), hiplib.iptr(ns)) != 0:
            raise RuntimeError(f"{fn.__name__} failed")
        return out[:ns[0]]

    def synthesize_batch(self, codes_list, int16=True):
        """Many utterances in one call (their chunks decoded together) -> per utterance what synthesize returns for it; an
        utterance of 0 frames gives an empty array."""
        live = [u for u, c in enumerate(codes_list) if len(c)]
        res = [np.zeros(0, np.int16 if int16 else np.float32) for _ in codes_list]
        n = np.array([len(codes_list[u]) for u in live], np.int32)
        if live:
            cap = int(self.lib.voc_synthesize_batch_max_samples(self.h, hiplib.iptr(n), len(n)))
            args = (self.h, _cat([codes_list[u] for u in live]).ctypes.data_as(hiplib.i64p), hiplib.iptr(n), len(n))
            fn = self.lib.voc_synthesize_batch if int16 else self.lib.voc_synthesize_batch_f32
            for u, pcm in zip(live, _packed(fn, args, len(n), cap, int16)):
                res[u] = pcm.copy()
        return res

    def last_batch(self):
        """-> (chunks decoded, GPU milliseconds) of the last synthesize* call"""
        return int(self.lib.voc_last_batch_chunks(self.h)), float(self.lib.voc_last_batch_ms(self.h))

    def stream(self, max_streams):
        """-> a VocoderStream of max_streams utterances on this handle (freed by its close() or by this handle's)"""
        self._streams.append(VocoderStream(self.lib, self.h, max_streams))
        return self._streams[-1]

    def incremental(self, max_streams, arithmetic="exact"):
        """-> an IncrementalStream of max_streams utterances on this handle (freed by its close() or by this handle's);
        arithmetic: "exact" (the default) or "split" (voc_incr_set_arithmetic)"""
        self._streams.append(IncrementalStream(self.lib, self.h, max_streams, arithmetic))
        return self._streams[-1]

    def incremental_samples(self, n_frames):
        """S(n): the samples of a whole carry-state decode of n_frames frames (voc_incr_samples)"""
        return int(self.lib.voc_incr_samples(self.h, int(n_frames)))

    def snapshots(self, n_slots):
        """Reserve n_slots snapshot slots of one stream's carried state on this handle (0: release them); every snapshot
        held so far is dropped (voc_incr_snapshots)."""
        if self.lib.voc_incr_snapshots(self.h, int(n_slots)) < 0:
            raise RuntimeError("voc_incr_snapshots failed (a negative count, or no device memory; see the log)")

    def snapshot_frames(self, slot):
        """the frames the stream saved in `slot` had taken; -1: an empty slot (voc_incr_snapshot_frames)"""
        return int(self.lib.voc_incr_snapshot_frames(self.h, int(slot)))

    def incremental_one(self, arithmetic="exact"):
        """-> synthesize_incremental's one-stream object for `arithmetic` (created on first use)"""
        if arithmetic not in self._incr1:
            self._incr1[arithmetic] = self.incremental(1, arithmetic)
        return self._incr1[arithmetic]

    def synthesize_incremental(self, codes, int16=False, arithmetic="exact", start_slot=None):
        """codes [n][16] -> the carry-state decode of the whole utterance (voc_incr_*): one stream, pushed in chunk_tokens
        pieces.  One seamless decode of all n frames -- not synthesize()'s cross-faded chunk walk -- and bit for bit what
        any other split of the frames across pushes gives (arithmetic="split": as long as no push is redone exactly).
        start_slot: the stream starts from that snapshot (IncrementalStream.save) instead of from silence, and the result
        holds the samples of `codes` alone: what a decode of [the snapshot's frames ; codes] yields behind the snapshot's."""
        c = _cat([codes])
        st = self.incremental_one(arithmetic)
        if start_slot is None:
            st.reset(0)
        else:
            st.restore([0], [start_slot])
        parts = [st.push([0], [c[f:f + self.chunk_tokens]], [f + self.chunk_tokens >= len(c)], int16)[0].copy()
                 for f in range(0, len(c), self.chunk_tokens)]
        return np.concatenate(parts + [np.zeros(0, np.int16 if int16 else np.float32)])

    def close(self):
        self._incr1 = {}
        for s in self._streams:          # every stream before the handle it runs on
            s.close()
        if self.h:
            self.lib.voc_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ARITHMETICS = ("exact", "split")     # voc_incr_set_arithmetic's 0 / 1


class VocoderStream:
    """The chunk walk fed frame by frame, for up to max_streams utterances at once (voc_stream_*)."""

    def __init__(self, lib, voc, max_streams):
        self.lib, self.h = lib, lib.voc_stream_create(voc, int(max_streams))
        if not self.h:
            raise RuntimeError("voc_stream_create failed")
        self.last_decodes, self.last_chunks, self.last_ms = 0, 0, 0.0    # of the last push

    def reset(self, k):
        """stream k starts a new utterance"""
        if self.lib.voc_stream_reset(self.h, int(k)) != 0:
            raise RuntimeError("voc_stream_reset failed")

    def push(self, streams, new_codes, finish, int16=True):
        """streams[i] takes the frames new_codes[i] [k][16] (k >= 0), and its utterance ends if finish[i] -> per entry the
        samples that became final."""
        st = np.array(streams, np.int32)
        n_new = np.array([len(c) for c in new_codes], np.int32)
        fin = np.array([int(f) for f in finish], np.int32)
        cap = int(self.lib.voc_stream_push_max_samples(self.h, len(st), hiplib.iptr(st), hiplib.iptr(n_new), hiplib.iptr(fin)))
        if cap < 0:
            raise RuntimeError("voc_stream_push: invalid push")
        args = (self.h, len(st), hiplib.iptr(st), _cat(new_codes).ctypes.data_as(hiplib.i64p), hiplib.iptr(n_new), hiplib.iptr(fin))
        fn = self.lib.voc_stream_push if int16 else self.lib.voc_stream_push_f32
        pcm = _packed(fn, args, len(st), cap, int16)
        self.last_decodes = int(self.lib.voc_stream_last_decodes(self.h))
        self.last_chunks = int(self.lib.voc_stream_last_chunks(self.h))
        self.last_ms = float(self.lib.voc_stream_last_ms(self.h))
        return pcm

    def close(self):
        if self.h:
            self.lib.voc_stream_free(self.h)
            self.h = None


class IncrementalStream:
    """The carry-state incremental decode, for up to max_streams utterances at once (voc_incr_*): every push hands out the
    samples of its new frames; joined, a stream's samples are one whole-utterance decode whatever the split."""

    def __init__(self, lib, voc, max_streams, arithmetic="exact"):
        self.lib, self.h = lib, lib.voc_incr_create(voc, int(max_streams))
        if not self.h:
            raise RuntimeError("voc_incr_create failed (see the log)")
        self.last_launches, self.last_ms = 0, 0.0    # of the last push
        self.last_restore_ms = 0.0                   # GPU milliseconds of the last restore
        self.last_split_launches, self.last_redone = 0, 0    # conv launches on the fp16 MFMA path, entries redone exactly
        self.state_bytes = int(lib.voc_incr_state_bytes(self.h))     # per stream, constant
        if arithmetic != "exact":
            self.set_arithmetic(arithmetic)

    @property
    def arithmetic(self):
        return ARITHMETICS[int(self.lib.voc_incr_arithmetic(self.h))]

    def set_arithmetic(self, arithmetic):
        """"exact" or "split" (voc_incr_set_arithmetic): accepted only while every stream is idle"""
        if arithmetic not in ARITHMETICS:
            raise ValueError(f"arithmetic must be one of {ARITHMETICS}, got {arithmetic!r}")
        if self.lib.voc_incr_set_arithmetic(self.h, ARITHMETICS.index(arithmetic)) < 0:
            raise RuntimeError("voc_incr_set_arithmetic refused (a stream is running, or no device memory; see the log)")

    def device_bytes(self):
        """device memory the object holds (fixed at creation; grows once with the first switch to "split")"""
        return int(self.lib.voc_incr_device_bytes(self.h))

    def reset(self, k):
        """stream k starts a new utterance"""
        if self.lib.voc_incr_reset(self.h, int(k)) != 0:
            raise RuntimeError("voc_incr_reset failed")

    def push(self, streams, new_codes, finish, int16=True):
        """streams[i] takes the frames new_codes[i] [k][16] (0 <= k <= chunk_tokens), and its utterance ends if finish[i] ->
        per entry the samples of its new frames."""
        st = np.array(streams, np.int32)
        n_new = np.array([len(c) for c in new_codes], np.int32)
        fin = np.array([int(f) for f in finish], np.int32)
        cap = int(self.lib.voc_incr_push_max_samples(self.h, len(st), hiplib.iptr(st), hiplib.iptr(n_new), hiplib.iptr(fin)))
        if cap < 0:
            raise RuntimeError("voc_incr_push: invalid push")
        args = (self.h, len(st), hiplib.iptr(st), _cat(new_codes).ctypes.data_as(hiplib.i64p), hiplib.iptr(n_new), hiplib.iptr(fin))
        fn = self.lib.voc_incr_push if int16 else self.lib.voc_incr_push_f32
        pcm = _packed(fn, args, len(st), cap, int16)
        self.last_launches = int(self.lib.voc_incr_last_launches(self.h))
        self.last_split_launches = int(self.lib.voc_incr_last_split_launches(self.h))
        self.last_redone = int(self.lib.voc_incr_last_redone(self.h))
        self.last_ms = float(self.lib.voc_incr_last_ms(self.h))
        return pcm

    def save(self, k, slot):
        """the carried state of the unfinished stream k -> snapshot slot `slot` of the handle (voc_incr_save)"""
        if self.lib.voc_incr_save(self.h, int(k), int(slot)) != 0:
            raise RuntimeError("voc_incr_save failed (a bad or finished stream, a bad slot, or no pool: Vocoder.snapshots)")

    def restore(self, streams, slots):
        """streams[i] continues the stream saved in slots[i], all in one launch (voc_incr_restore); a slot may repeat, a
        stream may not.  Nothing changes when any entry is refused."""
        st, sl = np.array(streams, np.int32), np.array(slots, np.int32)
        if len(st) != len(sl) or self.lib.voc_incr_restore(self.h, len(st), hiplib.iptr(st), hiplib.iptr(sl)) != 0:
            raise RuntimeError("voc_incr_restore refused (a bad or repeated stream, an empty slot, or one saved under the "
                               "other arithmetic; see the log)")
        self.last_restore_ms = float(self.lib.voc_incr_last_restore_ms(self.h))

    def close(self):
        if self.h:
            self.lib.voc_incr_free(self.h)
            self.h = None
