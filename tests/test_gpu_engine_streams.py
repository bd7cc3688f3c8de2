"""The engine runs on ONE stream and the vocoder on one ("hardware queues the process opens"): the frame graph
replays on the engine's own stream, the parallel-chain streams exist only once more than one chain is asked for, and every
read-back goes through pinned staging on the handle's stream.  None of that may change a bit of a result, so every
comparison here is exact: single chain against parallel chains, a re-capture in mid-utterance, a second engine after the
first was freed, engine and vocoder driven from two threads against their sequential runs, and the vocoder's staged
read-back against the un-staged one of voc_debug_run."""
import ctypes
import os
import threading

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.engine import FrameEngine
from tests.util import CACHE, synthetic_pack

pytestmark = pytest.mark.gpu

FRAMES = 4


@pytest.fixture(scope="module")
def pack():
    return synthetic_pack(2, 2)[0]


@pytest.fixture(scope="module")
def tiny_voc():
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, "voc_tiny_s7b.q3w")
    if not os.path.exists(path):
        W.write_pack(path, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    return path


def _inputs(B, seed=5):
    rng = np.random.default_rng(seed)
    lens = [9 + (7 * b) % 13 for b in range(B)]
    prefixes = [(0.05 * rng.standard_normal((n, 1024))).astype(np.float32) for n in lens]
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    return prefixes, [40] * B, pad


def _engine(pack, B, chains=None):
    eng = FrameEngine(pack, max_batch=B, n_ctx=64, max_frames=FRAMES)
    if chains is not None:
        eng.set_chains(chains)
    return eng


def _run(eng, B, split=None, chains_after_split=None):
    """FRAMES frames of the B-row batch -> codes[FRAMES][B][16]; `split`: run that many frames first, then (optionally
    after set_chains) the rest."""
    prefixes, n_text, pad = _inputs(B)
    eng.set_pad_embed(pad)
    eng.start(prefixes, n_text, ignore_eos=True, max_frames=FRAMES)
    if split is None:
        assert eng.run(FRAMES) == FRAMES
    else:
        assert eng.run(split) == split
        if chains_after_split is not None:
            eng.set_chains(chains_after_split)
        assert eng.run(FRAMES - split) == FRAMES - split
    codes, per = eng.codes()
    assert codes.shape == (FRAMES, B, 16) and (per == FRAMES).all()
    assert ((codes >= 0) & (codes < 2048)).all()
    return codes.copy()


@pytest.fixture(scope="module")
def single_chain(gpu_lib, pack):
    """The default engine's codes at 3 and 32 rows: computed once, compared against by every test below."""
    out = {}
    for B in (3, 32):
        eng = _engine(pack, B)
        out[B] = _run(eng, B)
        eng.destroy()
        out[B].setflags(write=False)
    return out


def test_two_chains_give_the_single_chain_codes_at_32_rows(gpu_lib, pack, single_chain):
    """32 rows split into two 16-row chains on their own (lazily created) streams against the single chain, bit for bit: a
    chain of a split batch launches the talker's attention shaped for the whole batch's rows and runs the code predictor's
    positions 0 and 1 through the kernels of the single chain's one-pass form (before that: 52 of these 2048 codes
    differed).  The existing test_engine_parallel_chains_match_single_chain never splits: 5 rows are one chain."""
    eng = _engine(pack, 32, chains=2)
    got = _run(eng, 32)
    eng.destroy()
    np.testing.assert_array_equal(got, single_chain[32])


@pytest.mark.parametrize("B", [3, 32])
def test_set_chains_in_mid_utterance_recaptures_and_continues(gpu_lib, pack, single_chain, B):
    """Two frames on the single chain (captured on the engine's stream), then set_chains(2): the chain streams are created
    now, the frame is captured again (at 3 rows two chains fall back to one: the batch is no multiple of 32) and the
    utterances go on exactly where they were.  Both forms keep the next frame's code-predictor input in the same rows (cp_seed_row0), so
    the hand-over needs nothing (before that: 985 of 2048 codes differed at 32 rows)."""
    eng = _engine(pack, B)
    got = _run(eng, B, split=2, chains_after_split=2)
    np.testing.assert_array_equal(got, single_chain[B])
    # ... and back to one chain on the same engine: a fresh batch, the streams of the two chains now idle
    eng.set_chains(1)
    np.testing.assert_array_equal(_run(eng, B), single_chain[B])
    eng.destroy()


@pytest.mark.parametrize("B", [3, 32])
def test_create_run_codes_destroy_create_again(gpu_lib, pack, single_chain, B):
    """Lazy creation and the free path: an engine that never made chain streams, one that did, and both again.  Engines of
    the same chain count agree with each other bit for bit (and the single-chain ones with the module's reference)."""
    got = []
    for chains in (None, 2, None, 2):
        eng = _engine(pack, B, chains)
        got.append(_run(eng, B))
        eng.destroy()
    np.testing.assert_array_equal(got[0], single_chain[B])
    np.testing.assert_array_equal(got[2], single_chain[B])
    np.testing.assert_array_equal(got[3], got[1])


def _voc_decode(lib, h, codes, out):
    return lib.voc_decode(h, codes.ctypes.data_as(hiplib.i64p), codes.shape[0], hiplib.fptr(out))


def test_vocoder_decode_beside_the_frame_loop_from_a_second_thread(gpu_lib, pack, tiny_voc):
    """One handle, one stream each: a vocoder decode submitted from a worker thread while q3e_run runs on the main thread
    returns the bits of its sequential run, and so does the frame loop."""
    lib = gpu_lib
    B = 2
    h = lib.voc_load(tiny_voc.encode(), 64, B)
    assert h
    rng = np.random.default_rng(11)
    vc = rng.integers(0, 2048, size=(B, 64, 16)).astype(np.int64)
    cs = lib.voc_chunk_samples(h)
    wave_seq = np.empty((B, cs), np.float32)
    assert _voc_decode(lib, h, vc, wave_seq) == 0
    eng = _engine(pack, B)
    codes_seq = _run(eng, B)
    # together
    prefixes, n_text, pad = _inputs(B)
    eng.start(prefixes, n_text, ignore_eos=True, max_frames=FRAMES)
    wave_par = np.full((B, cs), np.nan, np.float32)
    rc = []
    t = threading.Thread(target=lambda: rc.append(_voc_decode(lib, h, vc, wave_par)))
    t.start()
    ran = eng.run(FRAMES)
    t.join()
    codes_par = eng.codes()[0].copy()
    eng.destroy()
    lib.voc_free(h)
    assert ran == FRAMES and rc == [0]
    np.testing.assert_array_equal(codes_par, codes_seq)
    np.testing.assert_array_equal(wave_par, wave_seq)


def test_voc_decode_into_a_pageable_buffer_keeps_its_bits(gpu_lib, tiny_voc):
    """voc_decode reads back through the handle's pinned staging.  The same decode read back WITHOUT it (voc_debug_run over the
    whole op table copies straight into the caller's buffer, as voc_decode used to) must give the same bits; a destination
    that starts in the middle of a page takes them too, nothing is written past the last row, and a smaller batch after a
    larger one does not see the larger one's rows."""
    lib = gpu_lib
    lib.voc_debug_run.restype = ctypes.c_int
    lib.voc_debug_run.argtypes = [ctypes.c_void_p, hiplib.i64p, ctypes.c_int, ctypes.c_int, hiplib.f32p, hiplib.i32p, hiplib.i32p]
    B = 3
    h = lib.voc_load(tiny_voc.encode(), 64, B)
    assert h
    cs = lib.voc_chunk_samples(h)
    rng = np.random.default_rng(12)
    vc = rng.integers(0, 2048, size=(B, 64, 16)).astype(np.int64)
    for exact in (1, 0):
        lib.voc_set_exact_fp32(exact)
        direct = np.empty(B * cs + 64, np.float32)
        C, L = np.zeros(1, np.int32), np.zeros(1, np.int32)
        assert lib.voc_debug_run(h, vc.ctypes.data_as(hiplib.i64p), B, -1, hiplib.fptr(direct), hiplib.iptr(C), hiplib.iptr(L)) == 0
        assert (int(C[0]), int(L[0])) == (1, cs)
        want = direct[:B * cs].reshape(B, cs)
        raw = np.full(B * cs + 7 + 5, -7.0, np.float32)     # 28 bytes into its allocation, 5 sentinels behind the last row
        out = raw[7:7 + B * cs].reshape(B, cs)
        assert _voc_decode(lib, h, vc, out) == 0
        np.testing.assert_array_equal(out, want)
        assert (raw[:7] == -7.0).all() and (raw[7 + B * cs:] == -7.0).all()
        assert np.isfinite(out).all() and float(np.abs(out).max()) > 0
        one = np.full((2, cs), -7.0, np.float32)
        assert _voc_decode(lib, h, vc[1:2], one[:1]) == 0
        np.testing.assert_array_equal(one[0], want[1])
        assert (one[1] == -7.0).all()
    lib.voc_set_exact_fp32(0)      # (the library's default, as the other vocoder tests leave it)
    lib.voc_free(h)
