"""Snapshots of an incremental stream's carried state (voc_incr_snapshots / save / restore): a stream restored from the state
saved after frames P and fed U hands out, bit for bit, samples [S(T), S(T + |U|)) of ONE uninterrupted stream fed [P ; U] --
whatever the pushes on either side, the stream index, the neighbours, the object (of the same handle and arithmetic) -- and
after m frames it has handed out exactly S(T + m) - S(T) samples.  Array equality throughout; against the model the project's
existing 2e-4 of full scale (TOL of test_gpu_voc_incremental.py)."""
import math

import numpy as np
import pytest

from oracle.voc_ref import voc_reference
from qwen3_tts_axera_russian_amd import hiplib
from tests.test_gpu_voc_incremental import TOL, Incr, Voc, full_table, run_pattern, samples_of, write_tiny

pytestmark = pytest.mark.gpu

PROMPTS = [0, 1, 23, 24, 25, 33, 64, 65, 75, 97]     # either side of window - 1 = 23 and of chunk_tokens = 64; 0: a fresh stream
CONTS = [1, 9, 40, 70]
STEPS = [1, 8, 64]


def set_arith(st, split):
    return st.lib.voc_incr_set_arithmetic(st.s, split)


def snapshots(v, n):
    return v.lib.voc_incr_snapshots(v.h, n)


def frames_of(v, slot):
    return int(v.lib.voc_incr_snapshot_frames(v.h, slot))


def save(st, stream, slot):
    return st.lib.voc_incr_save(st.s, stream, slot)


def restore(st, streams, slots):
    a, b = np.array(streams, np.int32), np.array(slots, np.int32)
    return st.lib.voc_incr_restore(st.s, len(a), hiplib.iptr(a), hiplib.iptr(b))


def feed(st, k, codes, piece, finish=False, no_redo=False):
    """stream k takes `codes` in pushes of `piece` frames -> the joined samples"""
    got = [np.zeros(0, np.float32)]
    for f in range(0, len(codes), piece):
        got += st.push([(k, codes[f:f + piece], finish and f + piece >= len(codes))])
        if no_redo:
            assert st.lib.voc_incr_last_redone(st.s) == 0
    return np.concatenate(got)


def warm(st, k, prompt, slot, piece=64, no_redo=False):
    """stream k is reset, takes the prompt and is saved to `slot`"""
    st.reset(k)
    feed(st, k, prompt, piece, no_redo=no_redo)
    assert save(st, k, slot) == 0
    assert frames_of(st.voc, slot) == len(prompt)


def continue_together(st, prog, T, streams, conts, step, no_redo=False):
    """Restored streams take their continuations `step` frames per push, in the same calls; after every push each has handed
    out S(T + fed) - S(T) samples.  -> the joined samples per stream."""
    got, fed = [[np.zeros(0, np.float32)] for _ in conts], [0] * len(conts)
    while any(fed[i] < len(c) for i, c in enumerate(conts)):
        who = [i for i, c in enumerate(conts) if fed[i] < len(c)]
        outs = st.push([(streams[i], conts[i][fed[i]:fed[i] + step], False) for i in who])
        if no_redo:
            assert st.lib.voc_incr_last_redone(st.s) == 0
        for i, o in zip(who, outs):
            fed[i] = min(fed[i] + step, len(conts[i]))
            got[i].append(o)
            assert sum(len(x) for x in got[i]) == samples_of(prog, T + fed[i]) - samples_of(prog, T), (T, i, fed[i])
    return [np.concatenate(g) for g in got]


@pytest.mark.parametrize("arith", ["exact", "split"])
@pytest.mark.parametrize("trim", ["both", "right"])
def test_continuation_is_the_uninterrupted_stream(gpu_lib, tmp_path, trim, arith):
    """One code sequence; P = its first T frames, U the |U| frames behind them, so that the uninterrupted stream over [P ; U]
    is, for every T and |U|, a prefix of ONE uninterrupted stream over the whole sequence (a stream's samples are final when
    they are handed out).  The four continuations of a (T, step) pair run in four streams restored by one call."""
    path, tens = write_tiny(tmp_path, trim)
    prog = tens["voc.program"]
    S = lambda n: samples_of(prog, n)
    split = arith == "split"
    seq = np.random.default_rng(41).integers(0, 2048, size=(max(PROMPTS) + max(CONTS), 16)).astype(np.int64)
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 6)
    try:
        assert set_arith(st, int(split)) == int(split)
        assert snapshots(v, 2) == 2
        st.reset(5)
        base = feed(st, 5, seq, 64, finish=True, no_redo=split)
        assert len(base) == S(len(seq))
        for T in PROMPTS:
            warm(st, 0, seq[:T], 1, no_redo=split)
            for step in STEPS:
                streams = [1, 2, 3, 4]
                assert restore(st, streams, [1] * 4) == 0
                got = continue_together(st, prog, T, streams, [seq[T:T + u] for u in CONTS], step, no_redo=split)
                for u, g in zip(CONTS, got):
                    np.testing.assert_array_equal(g, base[S(T):S(T + u)], err_msg=f"T {T} |U| {u} step {step}")
        # the prompt in pieces of 7: the same state
        for T in (33, 75):
            warm(st, 0, seq[:T], 0, piece=7, no_redo=split)
            assert restore(st, [3], [0]) == 0
            got = continue_together(st, prog, T, [3], [seq[T:T + 40]], 8, no_redo=split)[0]
            np.testing.assert_array_equal(got, base[S(T):S(T + 40)])
        # a 0-frame snapshot is a reset: the stream starts from silence
        warm(st, 0, seq[:0], 0)
        feed(st, 2, seq[:50], 64)                      # (stream 2 holds something else)
        assert restore(st, [2], [0]) == 0
        np.testing.assert_array_equal(feed(st, 2, seq[:30], 8), base[:S(30)])
    finally:
        st.close()
        v.close()


def test_one_snapshot_into_many_streams_beside_neighbours(gpu_lib, tmp_path):
    path, tens = write_tiny(tmp_path, "both")
    prog = tens["voc.program"]
    S = lambda n: samples_of(prog, n)
    rng = np.random.default_rng(43)
    T = 33
    P = rng.integers(0, 2048, size=(T, 16)).astype(np.int64)
    U = [rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in (9, 40, 70)]
    N = [rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in (90, 110)]      # the neighbours' utterances
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 6)
    try:
        assert snapshots(v, 1) == 1
        ref = run_pattern(st, prog, [np.concatenate([P, u]) for u in U], None)
        ref_n = run_pattern(st, prog, N, 8, slots=[1, 4])                             # no restore anywhere
        warm(st, 5, P, 0)
        for k in (1, 4):
            st.reset(k)
        got_n = [[feed(st, 1, N[0][:30], 8)], [feed(st, 4, N[1][:50], 8)]]
        fed_n = [30, 50]
        assert restore(st, [0, 2, 3], [0, 0, 0]) == 0                                  # one call, one slot, three streams
        got, fed = [[] for _ in U], [0] * 3
        while any(f < len(u) for f, u in zip(fed, U)) or any(f < len(n) for f, n in zip(fed_n, N)):
            entries, who = [], []
            for i, k in enumerate((0, 2, 3)):
                if fed[i] < len(U[i]):
                    entries.append((k, U[i][fed[i]:fed[i] + 8], False))
                    who.append(("u", i))
            for i, k in enumerate((1, 4)):
                if fed_n[i] < len(N[i]):
                    entries.append((k, N[i][fed_n[i]:fed_n[i] + 8], fed_n[i] + 8 >= len(N[i])))
                    who.append(("n", i))
            for (kind, i), o in zip(who, st.push(entries)):
                if kind == "u":
                    fed[i] = min(fed[i] + 8, len(U[i]))
                    got[i].append(o)
                    assert sum(map(len, got[i])) == S(T + fed[i]) - S(T)
                else:
                    fed_n[i] = min(fed_n[i] + 8, len(N[i]))
                    got_n[i].append(o)
        for i in range(3):
            np.testing.assert_array_equal(np.concatenate(got[i]), ref[i][S(T):], err_msg=f"restored stream {i}")
        for i in range(2):
            np.testing.assert_array_equal(np.concatenate(got_n[i]), ref_n[i], err_msg=f"neighbour {i}")
    finally:
        st.close()
        v.close()


def test_across_objects_and_lifetimes(gpu_lib, tmp_path):
    path, tens = write_tiny(tmp_path, "both")
    prog = tens["voc.program"]
    S = lambda n: samples_of(prog, n)
    rng = np.random.default_rng(44)
    T = 40
    seq = rng.integers(0, 2048, size=(T + 40, 16)).astype(np.int64)
    X = rng.integers(0, 2048, size=(40, 16)).astype(np.int64)
    v = Voc(gpu_lib, path, 64, max_batch=5)
    a, b = Incr(v, 6), Incr(v, 1)
    a_open = True
    try:
        assert snapshots(v, 2) == 2
        base = run_pattern(a, prog, [seq], None)[0]
        warm(a, 4, seq[:T], 1)
        # a 6-stream object's snapshot continues in a 1-stream object of the same handle
        assert restore(b, [0], [1]) == 0
        np.testing.assert_array_equal(feed(b, 0, seq[T:], 8), base[S(T):])
        # ... after the saving object is gone
        a.close()
        a_open = False
        assert frames_of(v, 1) == T and restore(b, [0], [1]) == 0
        np.testing.assert_array_equal(feed(b, 0, seq[T:], 64), base[S(T):])
        # ... and after the arithmetic went there and back (accepted between utterances only: the restored stream is running)
        assert set_arith(b, 1) < 0
        b.reset(0)
        assert set_arith(b, 1) == 1 and set_arith(b, 0) == 0 and frames_of(v, 1) == T
        assert restore(b, [0], [1]) == 0
        np.testing.assert_array_equal(feed(b, 0, seq[T:], 7), base[S(T):])
        # a slot saved under "exact" is refused by an object in "split"; the stream goes on as if nothing had been asked
        b.reset(0)
        assert set_arith(b, 1) == 1
        split_x = feed(b, 0, X, 8, no_redo=True)
        split_seq = run_pattern(b, prog, [seq], None)[0]
        b.reset(0)
        head = feed(b, 0, X[:16], 8)
        assert restore(b, [0], [1]) < 0
        np.testing.assert_array_equal(np.concatenate([head, feed(b, 0, X[16:], 8)]), split_x)
        # the reverse: saved under "split", refused in "exact", accepted in "split" again
        warm(b, 0, seq[:T], 0)
        b.reset(0)
        assert set_arith(b, 0) == 0
        exact_x = run_pattern(b, prog, [X], 8)[0]
        b.reset(0)
        head = feed(b, 0, X[:16], 8)
        assert restore(b, [0], [0]) < 0
        np.testing.assert_array_equal(np.concatenate([head, feed(b, 0, X[16:], 8)]), exact_x)
        b.reset(0)
        assert set_arith(b, 1) == 1 and restore(b, [0], [0]) == 0
        np.testing.assert_array_equal(feed(b, 0, seq[T:], 8, no_redo=True), split_seq[S(T):])
    finally:
        if a_open:
            a.close()
        b.close()
        v.close()


def test_error_paths_change_nothing(gpu_lib, tmp_path):
    path, tens = write_tiny(tmp_path, "both")
    prog = tens["voc.program"]
    S = lambda n: samples_of(prog, n)
    rng = np.random.default_rng(45)
    T = 33
    seq = rng.integers(0, 2048, size=(T + 24, 16)).astype(np.int64)
    X = rng.integers(0, 2048, size=(40, 16)).astype(np.int64)
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 6)
    try:
        base, base_x = run_pattern(st, prog, [seq, X], None)
        for k in range(6):
            st.reset(k)
        got_x = [feed(st, 1, X[:16], 8)]
        # no pool
        assert frames_of(v, 0) == -1 and save(st, 1, 0) < 0 and restore(st, [2], [0]) < 0
        assert snapshots(v, -1) < 0 and frames_of(v, 0) == -1
        assert snapshots(v, 2) == 2 and frames_of(v, 0) == frames_of(v, 1) == -1 and frames_of(v, 2) == frames_of(v, -1) == -1
        warm(st, 0, seq[:T], 0)
        # a bad slot or stream
        for stream, slot in ((1, 2), (1, -1), (6, 1), (-1, 1)):
            assert save(st, stream, slot) < 0
        assert frames_of(v, 0) == T and frames_of(v, 1) == -1
        # a finished stream is not saved
        st.reset(5)
        st.push([(5, X[:8], True)])
        assert save(st, 5, 1) < 0 and frames_of(v, 1) == -1
        # restores that are refused as a whole: stream 1 (mid-utterance) and stream 2 (fresh) stay as they were
        for streams, slots in (([1, 6], [0, 0]), ([1, -1], [0, 0]), ([1, 2], [0, 2]), ([1, 2], [0, -1]),
                               ([1, 2, 1], [0, 0, 0]), ([1, 2], [0, 1])):             # bad stream, bad slot, named twice, empty slot
            assert restore(st, streams, slots) < 0
        got_x.append(feed(st, 1, X[16:], 8))
        np.testing.assert_array_equal(np.concatenate(got_x), base_x)
        np.testing.assert_array_equal(feed(st, 2, X, 64), base_x)
        # snapshots(-1) drops nothing; the slot still continues the prompt
        assert snapshots(v, -1) < 0 and frames_of(v, 0) == T
        assert restore(st, [3], [0]) == 0
        np.testing.assert_array_equal(feed(st, 3, seq[T:], 8), base[S(T):])
        # the slot is overwritten by the next save
        assert save(st, 3, 0) == 0 and frames_of(v, 0) == len(seq)
        # snapshots(0) empties every slot and releases the pool
        assert snapshots(v, 0) == 0
        assert frames_of(v, 0) == frames_of(v, 1) == -1
        assert restore(st, [4], [0]) < 0 and save(st, 4, 0) < 0
        np.testing.assert_array_equal(feed(st, 4, X, 8), base_x)
    finally:
        st.close()
        v.close()


def test_against_the_model(gpu_lib, tmp_path):
    path, tens = write_tiny(tmp_path, "both")
    prog = tens["voc.program"]
    T, n = 33, 40
    seq = np.random.default_rng(46).integers(0, 2048, size=(T + n, 16)).astype(np.int64)
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 2)
    try:
        assert snapshots(v, 1) == 1
        warm(st, 0, seq[:T], 0)
        assert restore(st, [1], [0]) == 0
        got = feed(st, 1, seq[T:], 8)
        ref = voc_reference(tens, seq[None])[0][samples_of(prog, T):]
        assert got.shape == ref.shape and np.abs(ref).max() > 0.05
        err = float(np.abs(got - ref).max())
        print(f"restored continuation T={T} |U|={n}: max abs err vs the oracle's whole decode {err:.2e}")
        assert err < TOL
    finally:
        st.close()
        v.close()


def test_full_size_table(gpu_lib):
    path, tens = full_table("both")
    prog = tens["voc.program"]
    T, n = 75, 24
    seq = np.random.default_rng(47).integers(0, 2048, size=(T + n, 16)).astype(np.int64)
    v = Voc(gpu_lib, path, 64, max_batch=2)
    st = Incr(v, 2)
    try:
        assert gpu_lib.voc_incr_state_bytes(st.s) == 5193984
        assert snapshots(v, 1) == 1
        base = run_pattern(st, prog, [seq], None)[0]
        warm(st, 0, seq[:T], 0)
        assert restore(st, [1], [0]) == 0
        ms = float(gpu_lib.voc_incr_last_restore_ms(st.s))
        print(f"full-size table: restore of one stream ({gpu_lib.voc_incr_state_bytes(st.s)} B) {ms:.4f} ms")
        assert ms > 0 and math.isfinite(ms)
        got = continue_together(st, prog, T, [1], [seq[T:]], 8)[0]
        np.testing.assert_array_equal(got, base[samples_of(prog, T):])
    finally:
        st.close()
        v.close()
