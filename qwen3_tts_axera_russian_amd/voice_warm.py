"""The batch server's cache of vocoder warm-ups per voice (`--voice_warm N`): a host-side LRU over the N snapshot slots of the
server's vocoder handle (include/qwen3tts_voc.h, voc_incr_snapshots).  An utterance that continues a codec prompt in
"vocoder": "incremental" needs its stream's carried state to hold the prompt; that state is a function of the prompt's frames
and the arithmetic alone, so it is decoded once (a miss: the warm-up pushes, then a save) and copied afterwards (a hit: one
restore launch for all hits of a call).  This module knows the stream object only by its reset / push / save / restore
methods (vocoder.IncrementalStream's) and imports nothing of HIP.  One thread -- the server's vocoder worker -- uses it."""
from __future__ import annotations

import collections
import hashlib

import numpy as np


def voice_key(prompt, arithmetic):
    """(digest of the prompt's [T][16] ids and T, arithmetic): a named voice and the same codes sent inline share an entry"""
    ids = np.ascontiguousarray(np.asarray(prompt, np.int64).reshape(-1, 16))
    h = hashlib.blake2b(digest_size=16)
    h.update(len(ids).to_bytes(8, "little"))
    h.update(ids.tobytes())
    return h.hexdigest(), str(arithmetic)


def warm_up(stream, k, prompt, chunk_tokens, samples):
    """Stream k (just reset) takes the prompt's frames, in pieces of at most chunk_tokens; none of their samples goes out.
    -> the samples of the prompt that the stream has still to hand out (and its caller to drop): samples(T) less what the
    pushes returned."""
    drop = samples(len(prompt))
    for f in range(0, len(prompt), chunk_tokens):
        drop -= len(stream.push([k], [prompt[f:f + chunk_tokens]], [False])[0])
    return drop


class VoiceWarmCache:
    """n_slots snapshot slots, least recently used first out.  n_slots == 0: nothing is cached, every call is the plain reset
    and warm-up."""

    def __init__(self, n_slots):
        self.n_slots = int(n_slots)
        if self.n_slots < 0:
            raise ValueError("--voice_warm takes a number of slots >= 0")
        self._slot = collections.OrderedDict()      # key -> slot, least recently used first
        self.hits = self.misses = self.evictions = 0

    def _take_slot(self, key, pinned):
        """-> a slot for a new entry: a free one, else the least recently used that no pending restore of this call reads
        (None: every slot is pinned -- the entry is not kept)"""
        used = set(self._slot.values())
        free = [z for z in range(self.n_slots) if z not in used]
        if free:
            z = free[0]
        else:
            old = next((k for k, z in self._slot.items() if z not in pinned), None)
            if old is None:
                return None
            z = self._slot.pop(old)
            self.evictions += 1
        self._slot[key] = z
        return z

    def _save(self, stream, k, key, z):
        try:
            stream.save(k, z)
        except Exception:
            del self._slot[key]         # the slot holds nothing usable: no later request may hit it
            raise

    def start(self, stream, arithmetic, resets, prompts, chunk_tokens, samples):
        """The streams `resets` start new utterances; prompts: {stream index: [T][16] ids} for those that continue a prompt.
        A stream without a prompt is reset.  With one: a hit takes no push at all -- all hits of the call go into ONE
        stream.restore, after the misses -- and a miss is reset, warmed up exactly as without the cache and saved, so that a
        later stream of the same call already hits.  -> {stream index: prompt samples it has still to hand out}: 0 after a
        hit (a restored stream never hands the prompt's samples out), warm_up's count after a miss."""
        drop, hit_streams, hit_slots = {}, [], []
        for k in resets:
            pr = prompts.get(k)
            if pr is None or not len(pr):
                stream.reset(k)
                continue
            key = voice_key(pr, arithmetic) if self.n_slots else None
            if key is not None and key in self._slot:
                self._slot.move_to_end(key)
                self.hits += 1
                hit_streams.append(k)
                hit_slots.append(self._slot[key])
                drop[k] = 0
                continue
            stream.reset(k)
            drop[k] = warm_up(stream, k, pr, chunk_tokens, samples)
            if key is not None:
                self.misses += 1
                z = self._take_slot(key, set(hit_slots))
                if z is not None:
                    self._save(stream, k, key, z)
        if hit_streams:
            stream.restore(hit_streams, hit_slots)
        return drop

    def slot_of(self, stream, arithmetic, prompt, chunk_tokens, samples):
        """For a one-stream object (an unstreamed reply): -> the slot that holds the prompt's state under `arithmetic`, warming
        stream 0 up with the prompt alone and saving it on a miss."""
        key = voice_key(prompt, arithmetic)
        if key in self._slot:
            self._slot.move_to_end(key)
            self.hits += 1
            return self._slot[key]
        self.misses += 1
        stream.reset(0)
        warm_up(stream, 0, prompt, chunk_tokens, samples)
        z = self._take_slot(key, ())
        self._save(stream, 0, key, z)
        return z

    def note(self):
        """for the per-request log line"""
        return f" (voice warm-ups: {self.hits} hits, {self.misses} misses so far)" if self.n_slots else ""
