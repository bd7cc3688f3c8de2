"""The vocoder's host wrapper (qwen3_tts_axera_russian_amd/vocoder.py) against the C ABI it wraps: the same bits from every
method, and a close() that frees every stream before the vocoder handle."""
import os

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.vocoder import Vocoder
from tests.util import CACHE

pytestmark = pytest.mark.gpu


def _ptr(a):
    return a.ctypes.data_as({np.int16: hiplib.i16p, np.float32: hiplib.f32p, np.int32: hiplib.i32p, np.int64: hiplib.i64p}[a.dtype.type])


class _Spy:
    """the library, with voc_stream_free / voc_free calls recorded"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in ("voc_stream_free", "voc_free"):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def test_wrapper_is_the_abi_and_closes_streams_first(gpu_lib):
    lib = gpu_lib
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, "voc_tiny_s7b.q3w")
    if not os.path.exists(path):
        W.write_pack(path, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    voc = Vocoder(path, 64, 4)
    assert (voc.chunk_tokens, voc.samples_per_token, voc.chunk_samples) == (64, 1920, lib.voc_chunk_samples(voc.h))
    rng = np.random.default_rng(23)
    utts = [rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in (1, 70, 150)]
    chunk = rng.integers(0, 2048, size=(2, 64, 16)).astype(np.int64)
    want = np.empty((2, voc.chunk_samples), np.float32)
    assert lib.voc_decode(voc.h, _ptr(chunk), 2, _ptr(want)) == 0
    np.testing.assert_array_equal(voc.decode(chunk), want)
    for dt, fn, fn_batch in ((np.float32, lib.voc_synthesize_f32, lib.voc_synthesize_batch_f32),
                             (np.int16, lib.voc_synthesize, lib.voc_synthesize_batch)):
        int16 = dt is np.int16
        for c in utts:
            out, ns = np.empty(lib.voc_synthesize_max_samples(voc.h, len(c)), dt), np.zeros(1, np.int32)
            assert fn(voc.h, _ptr(c), len(c), _ptr(out), _ptr(ns)) == 0
            got = voc.synthesize(c, int16=int16)
            assert got.dtype == dt
            np.testing.assert_array_equal(got, out[:ns[0]])
        # a batch with an utterance of 0 frames: an empty array for it, the others as one ABI call without it
        got = voc.synthesize_batch([utts[0], np.zeros((0, 16), np.int64), utts[2]], int16=int16)
        n = np.array([1, 150], np.int32)
        cap = int(lib.voc_synthesize_batch_max_samples(voc.h, _ptr(n), 2))
        out, off = np.empty(cap, dt), np.zeros(3, np.int64)
        assert fn_batch(voc.h, _ptr(np.concatenate([utts[0], utts[2]])), _ptr(n), 2, _ptr(out), cap, _ptr(off)) == 0
        assert len(got) == 3 and got[1].size == 0 and all(g.dtype == dt for g in got)
        np.testing.assert_array_equal(got[0], out[off[0]:off[1]])
        np.testing.assert_array_equal(got[2], out[off[1]:off[2]])
        assert voc.last_batch()[0] == lib.voc_last_batch_chunks(voc.h) == 1 + 4
    # the streaming walk: the same pushes through the wrapper and through the ABI on a stream object of its own
    ws, raw = voc.stream(2), lib.voc_stream_create(voc.h, 2)
    assert raw
    pushes = [([0, 1], [utts[1][:64], utts[2][:30]], [0, 0]), ([1], [utts[2][30:100]], [0]),
              ([0, 1], [utts[1][64:], utts[2][100:]], [1, 1])]
    for int16 in (True, False):
        dt = np.int16 if int16 else np.float32
        fn = lib.voc_stream_push if int16 else lib.voc_stream_push_f32
        for k in (0, 1):
            ws.reset(k)
            assert lib.voc_stream_reset(raw, k) == 0
        for streams, new, fin in pushes:
            got = ws.push(streams, new, fin, int16=int16)
            st, nn, ff = (np.array(x, np.int32) for x in (streams, [len(c) for c in new], fin))
            cap = int(lib.voc_stream_push_max_samples(raw, len(st), _ptr(st), _ptr(nn), _ptr(ff)))
            out, off = np.empty(max(cap, 1), dt), np.zeros(len(st) + 1, np.int64)
            assert fn(raw, len(st), _ptr(st), _ptr(np.concatenate(new)), _ptr(nn), _ptr(ff), _ptr(out), cap, _ptr(off)) == 0
            assert len(got) == len(streams)
            for i, g in enumerate(got):
                assert g.dtype == dt
                np.testing.assert_array_equal(g, out[off[i]:off[i + 1]])
            assert (ws.last_decodes, ws.last_chunks) == (lib.voc_stream_last_decodes(raw), lib.voc_stream_last_chunks(raw))
    lib.voc_stream_free(raw)
    # close(): every stream the handle made is freed before the handle; a second close() does nothing
    spy = _Spy(lib)
    for obj in (voc, ws, voc.stream(1)):
        obj.lib = spy
    voc.close()
    assert spy.calls == ["voc_stream_free", "voc_stream_free", "voc_free"]
    voc.close()
    ws.close()
    assert spy.calls == ["voc_stream_free", "voc_stream_free", "voc_free"] and voc.h is None and ws.h is None
