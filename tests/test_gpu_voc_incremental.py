"""Carry-state incremental decode (voc_incr_*): the decoder run as a stateful stream.  Per stream the samples of all pushes,
joined, are ONE whole-utterance decode of its frames -- the same bits however the frames were split across pushes, whatever
other streams shared the calls and whichever stream index it ran in -- and after pushes totalling n frames exactly S(n)
samples have gone out (S: the table's convt_out chain).  Against the model (oracle/voc_ref.py's whole decode, the code2wav
golden waveforms) and against voc_decode the tolerance is the project's existing 2e-4 of full scale
(test_code2wav_golden_on_the_gpu), every sample compared."""
import os

import numpy as np
import pytest

from oracle.voc_ref import voc_reference
from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from tests.util import CACHE

pytestmark = pytest.mark.gpu

TOL = 2e-4      # of full scale: test_code2wav_golden_on_the_gpu's bound
LENS = [1, 2, 3, 7, 8, 9, 23, 24, 25, 47, 63, 64, 65, 97, 113, 150, 199, 200]
PATTERNS = (1, 7, 8, 48, 64, None)       # frames per push; None: everything at once, in chunk_tokens pieces


def samples_of(prog, n):
    """S(n): the convt_out chain of the table applied to n frames (0 where it is not positive)"""
    L = int(n)
    for row in np.asarray(prog):
        if int(row[0]) == W.VOP_CONVT:
            L = max(0, (L - 1) * int(row[4]) + int(row[3]) - int(row[6]) - int(row[7]))
    return L


class Voc:
    def __init__(self, lib, path, chunk=64, max_batch=5):
        self.lib = lib
        self.h = lib.voc_load(path.encode(), chunk, max_batch)
        assert self.h
        self.chunk, self.cs = lib.voc_chunk_tokens(self.h), lib.voc_chunk_samples(self.h)

    def decode(self, codes):
        codes = np.ascontiguousarray(codes, np.int64)
        out = np.empty((codes.shape[0], self.cs), np.float32)
        assert self.lib.voc_decode(self.h, codes.ctypes.data_as(hiplib.i64p), codes.shape[0], hiplib.fptr(out)) == 0
        return out

    def close(self):
        self.lib.voc_free(self.h)


class Incr:
    def __init__(self, voc, max_streams):
        self.lib, self.voc = voc.lib, voc
        self.s = self.lib.voc_incr_create(voc.h, max_streams)
        assert self.s

    @staticmethod
    def _args(entries):
        streams = np.array([e[0] for e in entries], np.int32)
        n_new = np.array([len(e[1]) for e in entries], np.int32)
        fin = np.array([int(e[2]) for e in entries], np.int32)
        cat = np.ascontiguousarray(np.concatenate([np.asarray(e[1], np.int64).reshape(-1, 16) for e in entries]
                                                  + [np.zeros((0, 16), np.int64)]))
        return streams, n_new, fin, cat

    def max_samples(self, entries):
        streams, n_new, fin, _ = self._args(entries)
        return int(self.lib.voc_incr_push_max_samples(self.s, len(entries), hiplib.iptr(streams), hiplib.iptr(n_new), hiplib.iptr(fin)))

    def push_raw(self, entries, i16, out):
        """-> (return code, offsets); `out` is the caller's buffer, all of it is the capacity"""
        streams, n_new, fin, cat = self._args(entries)
        off = np.zeros(len(entries) + 1, np.int64)
        fn = self.lib.voc_incr_push if i16 else self.lib.voc_incr_push_f32
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
        assert self.lib.voc_incr_reset(self.s, k) == 0

    def close(self):
        self.lib.voc_incr_free(self.s)


def run_pattern(st, prog, utts, step, i16=False, slots=None):
    """All streams through the same calls, `step` frames per push each (None: chunk_tokens pieces); utterance u runs in stream
    slots[u].  After every push the running sample count of each stream is S(frames so far).  -> the joined samples."""
    slots = list(range(len(utts))) if slots is None else slots
    piece = st.voc.chunk if step is None else step
    got, fed, done = [[] for _ in utts], [0] * len(utts), [False] * len(utts)
    for k in slots:
        st.reset(k)
    while not all(done):
        entries, who = [], []
        for u, c in enumerate(utts):
            if done[u]:
                continue
            n = min(piece, len(c) - fed[u])
            entries.append((slots[u], c[fed[u]:fed[u] + n], fed[u] + n == len(c)))
            who.append(u)
        outs = st.push(entries, i16)
        for u, (k, new, fin), o in zip(who, entries, outs):
            fed[u] += len(new)
            got[u].append(o)
            done[u] = fin
            assert sum(len(x) for x in got[u]) == samples_of(prog, fed[u]) == st.lib.voc_incr_samples(st.voc.h, fed[u]), (u, fed[u])
    return [np.concatenate(g) for g in got]


def to_int16(x):
    """the project's int16 rule (vocoder_server.py:175): float32 product, clip, truncation toward zero"""
    return np.clip(x.astype(np.float32) * np.float32(32767), -32768, 32767).astype(np.int16)


def write_tiny(tmp_path, trim):
    vc = W.tiny_full_voc_config()       # every op kind: transformer with a 24-frame window, ConvNeXt blocks
    vc.convt_trim = trim
    tens = W.make_synthetic_voc(vc, seed=7)
    path = str(tmp_path / f"voc_tiny_{trim}.q3w")
    W.write_pack(path, {"voc_chunk": 64.0}, tens)
    return path, tens


def full_table(trim):
    vc = W.VocConfig()
    vc.convt_trim = trim
    name = "voc_whole_s1234.q3w" if trim == "both" else f"voc_whole_s1234_{trim}.q3w"
    path = os.path.join(CACHE, name)
    os.makedirs(CACHE, exist_ok=True)
    tens = W.make_synthetic_voc(vc, seed=1234)
    if not os.path.exists(path):
        W.write_pack(path, {"voc_chunk": 64.0}, tens)
    return path, tens


@pytest.mark.parametrize("trim", ["both", "right"])
def test_tiny_table_invariance_counts_and_the_oracle(gpu_lib, tmp_path, trim):
    """Lengths 1-200 in 18 streams over a handle of max_batch 5: every push pattern, another stream placement and the split
    arithmetic selected process-wide give the same bits; the joined samples are the oracle's whole decode of the N frames."""
    path, tens = write_tiny(tmp_path, trim)
    prog = tens["voc.program"]
    assert samples_of(prog, 8) == (14805 if trim == "both" else 8 * 1920) and samples_of(prog, 0) == 0
    rng = np.random.default_rng(5)
    utts = [rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in LENS]
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, len(utts) + 3)
    try:
        base = run_pattern(st, prog, utts, None)
        for u, c in enumerate(utts):
            ref = voc_reference(tens, c[None])[0]
            assert base[u].shape == ref.shape, (LENS[u], base[u].shape, ref.shape)
            if len(ref):
                err = float(np.abs(base[u] - ref).max())
                print(f"tiny {trim} N={LENS[u]}: max abs err vs the oracle's whole decode {err:.2e} (signal {np.abs(ref).max():.2f})")
                assert err < TOL, (LENS[u], err)
        for step in PATTERNS:
            got = run_pattern(st, prog, utts, step)
            for u in range(len(utts)):
                np.testing.assert_array_equal(got[u], base[u], err_msg=f"len {LENS[u]} step {step}")
        # other stream indices, other neighbours in the calls
        slots = [(5 * u + 2) % (len(utts) + 3) for u in range(len(utts))]
        assert len(set(slots)) == len(slots)
        got = run_pattern(st, prog, utts[::-1], 7, slots=slots)
        for u in range(len(utts)):
            np.testing.assert_array_equal(got[len(utts) - 1 - u], base[u])
        # alone in its calls
        np.testing.assert_array_equal(run_pattern(st, prog, [utts[-1]], 8, slots=[4])[0], base[-1])
        # the int16 push is the int16 rule applied to the f32 push
        got16 = run_pattern(st, prog, utts, 48, i16=True)
        for u in range(len(utts)):
            np.testing.assert_array_equal(got16[u], to_int16(base[u]))
        # the incremental mode is exact-fp32 whatever the process-wide arithmetic is
        for exact in (1, 0):
            gpu_lib.voc_set_exact_fp32(exact)
            np.testing.assert_array_equal(run_pattern(st, prog, utts[-3:], 8)[2], base[-1])
    finally:
        gpu_lib.voc_set_exact_fp32(0)
        st.close()
        v.close()


@pytest.mark.parametrize("trim,fused", [("both", 1), ("both", 0), ("right", 1)])
def test_full_size_table(gpu_lib, trim, fused):
    """The benchmark's vocoder: invariance over push patterns and stream placement, the oracle's whole decode of N = 80 frames
    (beyond chunk_tokens and the 72-frame window), voc_decode's first S(N) samples for N <= chunk_tokens."""
    path, tens = full_table(trim)
    prog = tens["voc.program"]
    assert samples_of(prog, 64) == (122325 if trim == "both" else 122880)
    rng = np.random.default_rng(21)
    lens = [80, 1, 8, 65, 30, 64, 73]
    utts = [rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in lens]
    gpu_lib.voc_set_fused_units(fused)
    gpu_lib.voc_set_exact_fp32(1)
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 8)
    try:
        base = run_pattern(st, prog, utts, None)
        for step in (1, 7, 8, 48, 64):
            got = run_pattern(st, prog, utts, step, slots=[7, 0, 3, 1, 6, 2, 5] if step == 8 else None)
            for u in range(len(utts)):
                np.testing.assert_array_equal(got[u], base[u], err_msg=f"len {lens[u]} step {step}")
        ref = voc_reference(tens, utts[0][None])[0]
        assert ref.shape == base[0].shape and np.abs(ref).max() > 0.05
        err = float(np.abs(base[0] - ref).max())
        print(f"full {trim} fused={fused} N=80: max abs err vs the oracle's whole decode {err:.2e} (signal {np.abs(ref).max():.2f})")
        assert err < TOL
        # the existing entry point on the same handle (exact fp32): its first S(N) samples, N <= chunk_tokens
        for u in (4, 5):
            padded = np.zeros((1, 64, 16), np.int64)
            padded[0, :lens[u]] = utts[u]
            dec = v.decode(padded)[0][:len(base[u])]
            err = float(np.abs(dec - base[u]).max())
            print(f"full {trim} fused={fused} N={lens[u]}: max abs diff to voc_decode {err:.2e}, bit-equal: {np.array_equal(dec, base[u])}")
            assert err < TOL
        got16 = run_pattern(st, prog, utts[:2], 48, i16=True)
        np.testing.assert_array_equal(got16[0], to_int16(base[0]))
    finally:
        gpu_lib.voc_set_fused_units(1)
        gpu_lib.voc_set_exact_fp32(0)
        st.close()
        v.close()


@pytest.mark.parametrize("name", ["omni", "omni_b", "tts"])
def test_code2wav_golden_waveforms_frame_by_frame(gpu_lib, tmp_path, name):
    """The waveforms of the importable implementation of the decoder family (tests/golden/code2wav_golden.npz), decoded one
    frame per push and all at once: the same bits, within 2e-4 of the golden, every sample."""
    from tests.test_code2wav_golden import load_case
    case, vc, tens, codes, gold, _ = load_case(name)
    path = str(tmp_path / f"c2w_{name}.q3w")
    W.write_pack(path, {"voc_chunk": float(case["T"])}, tens)
    v = Voc(gpu_lib, path, chunk=case["T"], max_batch=2)
    st = Incr(v, 2)
    try:
        one = run_pattern(st, tens["voc.program"], [codes[0]], 1)[0]
        whole = run_pattern(st, tens["voc.program"], [codes[0]], None, slots=[1])[0]
        np.testing.assert_array_equal(one, whole)
        assert whole.shape == gold["wav"].shape
        err = float(np.abs(whole - gold["wav"]).max())
        print(f"{name}: incremental max abs err vs the golden {err:.2e} (signal max {np.abs(gold['wav']).max():.2f})")
        assert err < TOL
    finally:
        st.close()
        v.close()


def test_error_paths_leave_the_streams_untouched(gpu_lib, tmp_path):
    path, tens = write_tiny(tmp_path, "both")
    prog = tens["voc.program"]
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 3)
    try:
        rng = np.random.default_rng(8)
        a = rng.integers(0, 2048, size=(130, 16)).astype(np.int64)
        want = run_pattern(st, prog, [a], None)[0]
        st.reset(0)
        head = st.push([(0, a[:60], False)])
        bad = np.full(10, 7.0, np.float32)
        for entries in ([(3, a[60:80], False)], [(-1, a[60:80], False)], [(0, a[60:80], False), (0, a[80:90], False)],
                        [(0, a[60:125], False)]):                       # bad index, named twice, n_new beyond chunk_tokens
            assert st.max_samples(entries) < 0
            assert st.push_raw(entries, False, bad)[0] < 0
            assert (bad == 7.0).all()
        entries = [(0, a[60:100], False)]
        need = st.max_samples(entries)
        assert need == samples_of(prog, 100) - samples_of(prog, 60) > 0
        small = np.full(need - 1 + 5, 7.0, np.float32)
        assert st.push_raw(entries, False, small[:need - 1])[0] < 0      # too small a capacity
        assert (small == 7.0).all()
        rest = st.push(entries) + st.push([(0, a[100:], True)])
        np.testing.assert_array_equal(np.concatenate(head + rest), want)  # every refused push left the state as it was
        # a finished stream refuses frames until it is reset; the same push then succeeds
        entries = [(0, a[:5], False)]
        assert st.max_samples(entries) < 0 and st.push_raw(entries, False, bad)[0] < 0
        st.reset(0)
        np.testing.assert_array_equal(st.push(entries)[0], want[:samples_of(prog, 5)])
        # the finish push adds no sample; a stream that ends with no frame hands out nothing
        assert [len(o) for o in st.push([(0, np.zeros((0, 16), np.int64), True)])] == [0]
        st.reset(2)
        assert [len(o) for o in st.push([(2, np.zeros((0, 16), np.int64), True)])] == [0]
        # a reset drops an unfinished utterance: the next one starts from silence
        st.reset(1)
        st.push([(1, a[:33], False)])
        st.reset(1)
        np.testing.assert_array_equal(np.concatenate(st.push([(1, a[:64], False)]) + st.push([(1, a[64:128], False)])
                                                     + st.push([(1, a[128:], True)])), want)
    finally:
        st.close()
        v.close()


def test_long_stream_keeps_constant_memory_and_stays_on_the_model(gpu_lib, tmp_path):
    """3000 frames through one stream: the object's device allocation does not move, and the last 100 frames' samples agree
    with the oracle's decode of those frames behind 100 frames of left context (the receptive field: two attention layers of
    23 frames each + the convs' few frames)."""
    path, tens = write_tiny(tmp_path, "both")
    prog = tens["voc.program"]
    v = Voc(gpu_lib, path, 64, max_batch=2)
    st = Incr(v, 2)
    try:
        N, TAIL, CTX = 3000, 100, 100
        rng = np.random.default_rng(13)
        c = rng.integers(0, 2048, size=(N, 16)).astype(np.int64)
        st.reset(1)
        bytes0, state = gpu_lib.voc_incr_device_bytes(st.s), gpu_lib.voc_incr_state_bytes(st.s)
        assert bytes0 > 2 * state > 0
        got = []
        for f in range(0, N, 50):
            got += st.push([(1, c[f:f + 50], f + 50 >= N)])
            assert gpu_lib.voc_incr_device_bytes(st.s) == bytes0
        got = np.concatenate(got)
        assert len(got) == samples_of(prog, N)
        ref = voc_reference(tens, c[None, N - TAIL - CTX:])[0]
        n_tail = samples_of(prog, N) - samples_of(prog, N - TAIL)
        err = float(np.abs(got[-n_tail:] - ref[-n_tail:]).max())
        print(f"long stream: tail of {TAIL} frames after {N}: max abs err vs the oracle on the window {err:.2e}")
        assert np.abs(ref[-n_tail:]).max() > 0.05 and err < TOL
    finally:
        st.close()
        v.close()
