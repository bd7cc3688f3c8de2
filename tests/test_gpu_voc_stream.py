"""Streaming chunk walk (voc_stream_*): frames pushed as they are generated, many utterances per call.  Per stream, the samples
of all pushes joined are the whole-utterance walk (voc_synthesize_f32 / voc_synthesize, and the restatement pinned to the
reference's VocoderServer.synthesize around voc_decode) bit for bit, however the frames were split; after every push that does
not finish a stream, exactly the samples no later chunk can change have gone out."""
import os

import numpy as np
import pytest

from oracle import frontend as fe
from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from tests.util import CACHE

pytestmark = pytest.mark.gpu

LENS = [1, 10, 16, 63, 64, 65, 97, 112, 113, 150, 200]


class Voc:
    def __init__(self, lib, path, max_batch=5):
        self.lib = lib
        self.h = lib.voc_load(path.encode(), 64, max_batch)
        assert self.h
        self.spt, self.cs = lib.voc_samples_per_token(self.h), lib.voc_chunk_samples(self.h)

    def decode(self, codes):
        codes = np.ascontiguousarray(codes, np.int64)
        out = np.empty((codes.shape[0], self.cs), np.float32)
        assert self.lib.voc_decode(self.h, codes.ctypes.data_as(hiplib.i64p), codes.shape[0], hiplib.fptr(out)) == 0
        return out

    def synth(self, codes, i16):
        codes = np.ascontiguousarray(codes, np.int64)
        n = codes.shape[0]
        out = np.empty(self.lib.voc_synthesize_max_samples(self.h, n), np.int16 if i16 else np.float32)
        ns = np.zeros(1, np.int32)
        fn = self.lib.voc_synthesize if i16 else self.lib.voc_synthesize_f32
        ptr = out.ctypes.data_as(hiplib.i16p) if i16 else hiplib.fptr(out)
        assert fn(self.h, codes.ctypes.data_as(hiplib.i64p), n, ptr, hiplib.iptr(ns)) == 0
        return out[:ns[0]]

    def close(self):
        self.lib.voc_free(self.h)


class Stream:
    def __init__(self, voc, max_streams):
        self.lib = voc.lib
        self.s = self.lib.voc_stream_create(voc.h, max_streams)
        assert self.s

    def _args(self, entries):
        streams = np.array([e[0] for e in entries], np.int32)
        n_new = np.array([len(e[1]) for e in entries], np.int32)
        fin = np.array([int(e[2]) for e in entries], np.int32)
        cat = np.ascontiguousarray(np.concatenate([np.asarray(e[1], np.int64).reshape(-1, 16) for e in entries]
                                                  + [np.zeros((0, 16), np.int64)]))
        return streams, n_new, fin, cat

    def max_samples(self, entries):
        streams, n_new, fin, _ = self._args(entries)
        return int(self.lib.voc_stream_push_max_samples(self.s, len(entries), hiplib.iptr(streams), hiplib.iptr(n_new),
                                                        hiplib.iptr(fin)))

    def push_raw(self, entries, i16, out):
        """-> (return code, offsets); `out` is the caller's buffer, all of it is the capacity"""
        streams, n_new, fin, cat = self._args(entries)
        off = np.zeros(len(entries) + 1, np.int64)
        fn = self.lib.voc_stream_push if i16 else self.lib.voc_stream_push_f32
        ptr = out.ctypes.data_as(hiplib.i16p) if i16 else hiplib.fptr(out)
        rc = fn(self.s, len(entries), hiplib.iptr(streams), cat.ctypes.data_as(hiplib.i64p), hiplib.iptr(n_new), hiplib.iptr(fin),
                ptr, len(out), off.ctypes.data_as(hiplib.i64p))
        return rc, off

    def push(self, entries, i16=False):
        """entries: (stream, new frames [n][16], finish) -> the samples each entry handed out"""
        cap = self.max_samples(entries)
        assert cap >= 0
        out = np.empty(cap, np.int16 if i16 else np.float32)
        rc, off = self.push_raw(entries, i16, out)
        assert rc == 0 and off[-1] == cap
        return [out[off[i]:off[i + 1]].copy() for i in range(len(entries))]

    def reset(self, k):
        assert self.lib.voc_stream_reset(self.s, k) == 0

    def close(self):
        self.lib.voc_stream_free(self.s)


def final_after(f, cs, ov):
    """samples a stream has handed out after pushes of f frames in all, none finishing: the full 64-frame chunks decoded so far
    assembled (the first whole, each next one cross-faded over the last OV), minus the OV the next chunk may still change"""
    k = 0 if f < 64 else (f - 64) // 48 + 1
    return 0 if k == 0 else cs + (k - 1) * (cs - ov) - ov


def run_pattern(st, utts, step, i16, cs, ov):
    """All streams through the same calls, `step` frames per push each (None: everything in the finish push)."""
    got = [[] for _ in utts]
    fed = [0] * len(utts)
    done = [False] * len(utts)
    for k in range(len(utts)):
        st.reset(k)
    while not all(done):
        entries = []
        for k, c in enumerate(utts):
            if done[k]:
                continue
            n = len(c) - fed[k] if step is None else min(step, len(c) - fed[k])
            entries.append((k, c[fed[k]:fed[k] + n], fed[k] + n == len(c)))
        outs = st.push(entries, i16)
        for (k, new, fin), o in zip(entries, outs):
            fed[k] += len(new)
            got[k].append(o)
            done[k] = fin
            if not fin:   # latency contract: exactly the samples no later chunk can change
                assert sum(len(x) for x in got[k]) == final_after(fed[k], cs, ov), (k, fed[k])
    return [np.concatenate(g) for g in got]


@pytest.mark.parametrize("trim", ["both", "right"])
def test_streamed_walk_is_the_whole_utterance_walk(gpu_lib, tmp_path, trim):
    vc = W.tiny_voc_config()
    vc.convt_trim = trim
    path = str(tmp_path / f"voc_{trim}.q3w")
    W.write_pack(path, {"voc_chunk": 64.0}, W.make_synthetic_voc(vc, seed=7))
    rng = np.random.default_rng(5)
    utts = [rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in LENS]
    try:
        for exact in (1, 0):
            gpu_lib.voc_set_exact_fp32(exact)
            v = Voc(gpu_lib, path, max_batch=5)
            ov = 16 * v.spt
            want = [v.synth(c, False) for c in utts]
            want16 = [v.synth(c, True) for c in utts]
            for c, w in zip(utts, want):
                np.testing.assert_array_equal(w, fe.voc_synthesize(c, lambda padded: v.decode(padded)[0], 64))
            st = Stream(v, len(utts))
            for step in (1, 7, 48, 64, None):
                for i16 in (False, True):
                    got = run_pattern(st, utts, step, i16, v.cs, ov)
                    for k in range(len(utts)):
                        np.testing.assert_array_equal(got[k], (want16 if i16 else want)[k], err_msg=f"len {LENS[k]} step {step}")
            st.close()
            v.close()
    finally:
        gpu_lib.voc_set_exact_fp32(0)


def test_push_batches_chunks_across_streams(gpu_lib, tmp_path):
    """The chunks one push completes are decoded together, max_batch per call; a push that completes none decodes nothing."""
    path = str(tmp_path / "voc.q3w")
    W.write_pack(path, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    v = Voc(gpu_lib, path, max_batch=5)
    st = Stream(v, 8)
    rng = np.random.default_rng(6)
    utts = [rng.integers(0, 2048, size=(150, 16)).astype(np.int64) for _ in range(8)]
    st.push([(k, utts[k][:63], False) for k in range(8)])
    assert gpu_lib.voc_stream_last_chunks(st.s) == 0 and gpu_lib.voc_stream_last_decodes(st.s) == 0
    st.push([(k, utts[k][63:112], False) for k in range(8)])              # 112 frames: chunks 0 and 1 of each stream
    assert gpu_lib.voc_stream_last_chunks(st.s) == 16 and gpu_lib.voc_stream_last_decodes(st.s) == 4
    outs = st.push([(k, utts[k][112:], True) for k in range(8)])           # finish: chunk 2 (54 frames) and the 6-frame tail
    assert gpu_lib.voc_stream_last_chunks(st.s) == 16
    assert all(len(o) > 0 for o in outs)
    st.close()
    v.close()


def test_reset_mid_utterance_and_errors(gpu_lib, tmp_path):
    path = str(tmp_path / "voc.q3w")
    W.write_pack(path, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    gpu_lib.voc_set_exact_fp32(1)
    try:
        v = Voc(gpu_lib, path, max_batch=5)
        st = Stream(v, 3)
        rng = np.random.default_rng(8)
        a, b, c = (rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in (100, 150, 130))
        # stream 0 drops utterance a after 100 frames and takes b; stream 1 carries c through it all
        got_c = st.push([(0, a, False), (1, c[:70], False)])[1:]
        st.reset(0)
        got_b = []
        for f0 in range(0, 150, 48):
            fin = f0 + 48 >= 150
            o = st.push([(0, b[f0:f0 + 48], fin)] + ([(1, c[70:], True)] if fin else []))
            got_b.append(o[0])
            got_c += o[1:]
        np.testing.assert_array_equal(np.concatenate(got_b), v.synth(b, False))
        np.testing.assert_array_equal(np.concatenate(got_c), v.synth(c, False))
        # a stream that ends with no frame hands out nothing
        st.reset(2)
        assert [len(o) for o in st.push([(2, np.zeros((0, 16), np.int64), True)])] == [0]

        # errors: < 0, nothing written, nothing changed -- the same push then succeeds
        for k in range(3):
            st.reset(k)
        head = st.push([(0, a[:60], False)])
        assert len(head[0]) == 0
        bad = np.full(10, 7.0, np.float32)
        for entries in ([(3, a[60:80], False)], [(-1, a[60:80], False)], [(0, a[60:80], False), (0, a[80:90], False)]):
            assert st.max_samples(entries) < 0
            assert st.push_raw(entries, False, bad)[0] < 0
        streams, n_new, fin = np.array([0], np.int32), np.array([-1], np.int32), np.array([0], np.int32)
        off = np.zeros(2, np.int64)
        assert gpu_lib.voc_stream_push_f32(st.s, 1, hiplib.iptr(streams), a.ctypes.data_as(hiplib.i64p), hiplib.iptr(n_new),
                                           hiplib.iptr(fin), hiplib.fptr(bad), len(bad), off.ctypes.data_as(hiplib.i64p)) < 0
        entries = [(0, a[60:100], False)]                  # completes chunk 0: CS - OV samples go out
        need = st.max_samples(entries)
        assert need == final_after(100, v.cs, 16 * v.spt) > 0
        small = np.full(need - 1 + 5, 7.0, np.float32)
        assert st.push_raw(entries, False, small[:need - 1])[0] < 0
        assert (small == 7.0).all()
        rest = st.push(entries) + st.push([(0, np.zeros((0, 16), np.int64), True)])
        np.testing.assert_array_equal(np.concatenate(head + rest), v.synth(a, False))
        # a finished stream refuses frames until it is reset
        assert st.push_raw([(0, a[:5], False)], False, bad)[0] < 0
        st.reset(0)
        assert len(st.push([(0, a[:5], True)])[0]) == 5 * v.spt
        st.close()
        v.close()
    finally:
        gpu_lib.voc_set_exact_fp32(0)


def test_full_size_table_streamed_in_48_frame_pushes(gpu_lib):
    """The benchmark's vocoder, exact fp32: about 200 frames pushed 48 at a time == voc_synthesize_f32."""
    path = os.path.join(CACHE, "voc_whole_s1234.q3w")
    os.makedirs(CACHE, exist_ok=True)
    if not os.path.exists(path):
        W.write_pack(path, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.VocConfig(), seed=1234))
    gpu_lib.voc_set_exact_fp32(1)
    try:
        v = Voc(gpu_lib, path, max_batch=4)
        st = Stream(v, 2)
        rng = np.random.default_rng(11)
        utts = [rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in (197, 130)]
        got = run_pattern(st, utts, 48, False, v.cs, 16 * v.spt)
        for g, c in zip(got, utts):
            np.testing.assert_array_equal(g, v.synth(c, False))
        st.close()
        v.close()
    finally:
        gpu_lib.voc_set_exact_fp32(0)
