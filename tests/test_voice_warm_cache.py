"""The batch server's voice warm-up cache (voice_warm.VoiceWarmCache) alone, on the CPU: a fake stream object records the reset /
push / save / restore calls the cache makes.  The fake hands no sample out, so what a warm-up leaves to drop is all of S(T)."""
import sys

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd.voice_warm import VoiceWarmCache, voice_key

CH = 64                                   # chunk_tokens
S = lambda n: 1920 * n - 555 if n else 0  # any S(n) will do


class FakeStream:
    def __init__(self):
        self.calls = []

    def reset(self, k):
        self.calls.append(("reset", k))

    def push(self, streams, new_codes, finish, int16=True):
        self.calls.append(("push", list(streams), [len(c) for c in new_codes], list(finish)))
        return [np.zeros(0, np.int16) for _ in streams]

    def save(self, k, slot):
        self.calls.append(("save", k, slot))

    def restore(self, streams, slots):
        self.calls.append(("restore", list(streams), list(slots)))


def voice(seed, T):
    return np.random.default_rng(seed).integers(0, 2048, size=(T, 16)).astype(np.int32)


def present_behaviour(resets, prompts):
    """the calls the server made before the cache existed: reset, then the prompt in chunk_tokens pieces"""
    calls = []
    for k in resets:
        calls.append(("reset", k))
        pr = prompts.get(k)
        if pr is not None and len(pr):
            calls += [("push", [k], [min(CH, len(pr) - f)], [False]) for f in range(0, len(pr), CH)]
    return calls


def test_the_module_does_not_import_hip():
    assert "qwen3_tts_axera_russian_amd.voice_warm" in sys.modules
    import qwen3_tts_axera_russian_amd.voice_warm as vw
    assert not any(name in vars(vw) for name in ("hiplib", "ctypes", "Vocoder"))


def test_a_miss_pushes_the_prompt_in_chunk_pieces_then_saves():
    c, st, a = VoiceWarmCache(2), FakeStream(), voice(1, 150)
    drop = c.start(st, "exact", [3], {3: a}, CH, S)
    assert st.calls == [("reset", 3), ("push", [3], [64], [False]), ("push", [3], [64], [False]), ("push", [3], [22], [False]),
                        ("save", 3, 0)]
    assert drop == {3: S(150)} and (c.hits, c.misses, c.evictions) == (0, 1, 0)


def test_a_hit_pushes_nothing_and_one_call_restores_once():
    c, st, a, b = VoiceWarmCache(2), FakeStream(), voice(1, 75), voice(2, 30)
    c.start(st, "exact", [0, 1], {0: a, 1: b}, CH, S)
    st.calls.clear()
    drop = c.start(st, "exact", [4, 2, 5, 0], {4: a, 2: b, 0: a}, CH, S)          # 5: no prompt
    assert st.calls == [("reset", 5), ("restore", [4, 2, 0], [0, 1, 0])]
    assert drop == {4: 0, 2: 0, 0: 0} and (c.hits, c.misses) == (3, 2)
    # several streams of one call with the same new voice: the first is the miss, the rest hit
    c, st = VoiceWarmCache(2), FakeStream()
    drop = c.start(st, "split", [1, 0, 2], {1: a, 0: a, 2: a}, CH, S)
    assert st.calls == [("reset", 1), ("push", [1], [64], [False]), ("push", [1], [11], [False]), ("save", 1, 0),
                        ("restore", [0, 2], [0, 0])]
    assert drop == {1: S(75), 0: 0, 2: 0} and (c.hits, c.misses) == (2, 1)


def test_the_key_separates_arithmetics_prompts_and_lengths():
    a = voice(1, 40)
    one_id = a.copy()
    one_id[17, 5] ^= 1
    keys = {voice_key(a, "exact"), voice_key(a, "split"), voice_key(one_id, "exact"), voice_key(a[:39], "exact"),
            voice_key(np.concatenate([a, np.zeros((1, 16), np.int32)]), "exact")}
    assert len(keys) == 5
    # the same ids in another container or integer type are the same voice (a named voice and inline prompt_codes)
    assert voice_key(a.astype(np.int64).tolist(), "exact") == voice_key(a, "exact")
    c, st = VoiceWarmCache(4), FakeStream()
    for pr, arith in ((a, "exact"), (a, "split"), (one_id, "exact"), (a[:39], "exact")):
        c.start(st, arith, [0], {0: pr}, CH, S)
    assert (c.hits, c.misses) == (0, 4)
    c.start(st, "split", [0], {0: a}, CH, S)
    assert (c.hits, c.misses) == (1, 4)


def test_lru_order_and_the_eviction_count():
    c, st = VoiceWarmCache(2), FakeStream()
    a, b, d = voice(1, 10), voice(2, 10), voice(3, 10)
    start = lambda pr: c.start(st, "exact", [0], {0: pr}, CH, S)
    saves = lambda: [x for x in st.calls if x[0] == "save"]
    start(a), start(b)
    assert saves() == [("save", 0, 0), ("save", 0, 1)] and c.evictions == 0
    start(a)                               # a is the most recently used now
    start(d)                               # evicts b
    assert saves()[-1] == ("save", 0, 1) and (c.hits, c.misses, c.evictions) == (1, 3, 1)
    start(a)
    assert (c.hits, c.misses, c.evictions) == (2, 3, 1)
    start(b)                               # a miss again: evicts d, the least recently used
    assert saves()[-1] == ("save", 0, 1) and (c.hits, c.misses, c.evictions) == (2, 4, 2)
    start(d)                               # evicts a
    assert saves()[-1] == ("save", 0, 0) and (c.hits, c.misses, c.evictions) == (2, 5, 3)
    # a slot that a hit of the same call is still to be restored from is not given away
    c, st = VoiceWarmCache(1), FakeStream()
    c.start(st, "exact", [0], {0: a}, CH, S)
    st.calls.clear()
    drop = c.start(st, "exact", [0, 1], {0: a, 1: b}, CH, S)
    assert st.calls == [("reset", 1), ("push", [1], [10], [False]), ("restore", [0], [0])]
    assert drop == {0: 0, 1: S(10)} and (c.hits, c.misses, c.evictions) == (1, 2, 0)


def test_the_one_stream_path():
    c, st, a = VoiceWarmCache(2), FakeStream(), voice(1, 70)
    assert c.slot_of(st, "exact", a, CH, S) == 0
    assert st.calls == [("reset", 0), ("push", [0], [64], [False]), ("push", [0], [6], [False]), ("save", 0, 0)]
    st.calls.clear()
    assert c.slot_of(st, "exact", a, CH, S) == 0 and st.calls == [] and (c.hits, c.misses) == (1, 1)
    # the streamed path finds the voice the unstreamed one warmed
    assert c.start(st, "exact", [2], {2: a}, CH, S) == {2: 0} and st.calls == [("restore", [2], [0])]


def test_a_failed_save_leaves_no_entry():
    class Failing(FakeStream):
        def save(self, k, slot):
            raise RuntimeError("no")
    c, a = VoiceWarmCache(1), voice(1, 5)
    with pytest.raises(RuntimeError):
        c.start(Failing(), "exact", [0], {0: a}, CH, S)
    st = FakeStream()
    c.start(st, "exact", [0], {0: a}, CH, S)
    assert ("save", 0, 0) in st.calls and c.hits == 0


def test_the_server_refuses_the_flag_without_concurrent():
    from qwen3_tts_axera_russian_amd import batch_server as bs
    for kw in (dict(concurrent=False, voice_warm=2), dict(concurrent=True, voice_warm=-1)):
        with pytest.raises(ValueError, match="voice_warm"):      # (before any file is opened)
            bs.BatchSynthesisServer("no.q3w", "no.q3w", install_signal_handlers=False, **kw)


def test_without_slots_it_is_the_present_behaviour_call_for_call():
    c, st = VoiceWarmCache(0), FakeStream()
    a, b = voice(1, 130), voice(2, 64)
    for resets, prompts in (([2, 0, 1], {2: a, 1: b}), ([0], {0: a}), ([1, 2], {}), ([], {}), ([3], {3: a[:0]})):
        st.calls.clear()
        drop = c.start(st, "exact", resets, dict(prompts), CH, S)
        assert st.calls == present_behaviour(resets, prompts)
        assert drop == {k: S(len(p)) for k, p in prompts.items() if len(p)}
    assert (c.hits, c.misses, c.evictions) == (0, 0, 0) and c.note() == ""
    with pytest.raises(ValueError):
        VoiceWarmCache(-1)
