"""A vocoder call runs under ONE snapshot of the process-wide settings (csrc/q3_voc_settings.h): voc_set_* calls made from
another thread while a synthesize call is in flight change the NEXT call, never the one running.  Every result of a call made
under a setter storm is, bit for bit, the output of one of the four (exact_fp32, fused_units) settings -- never a decode whose
convs ran partly split and partly exact, whose tail chunk was planned under one arithmetic and decoded under the other, or
whose overflow flag was not looked at."""
import os
import threading

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from tests import voc_gpu_common as vg
from tests.util import CACHE

pytestmark = pytest.mark.gpu

SEED = 11
FRAMES = 45      # chunk 40: one full chunk and a 21-frame tail, decoded at 24 frames (exact) or 40 (split)


def synth(lib, h, codes):
    n = codes.shape[0]
    out = np.empty(lib.voc_synthesize_max_samples(h, n), np.float32)
    ns = np.zeros(1, np.int32)
    assert lib.voc_synthesize_f32(h, codes.ctypes.data_as(hiplib.i64p), n, hiplib.fptr(out), hiplib.iptr(ns)) == 0
    return out[:ns[0]].copy()


def test_a_call_in_flight_keeps_the_settings_it_started_with(gpu_lib):
    lib = vg.hooks(gpu_lib)
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, "voc_tiny_s7b.q3w")
    if not os.path.exists(path):
        W.write_pack(path, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    codes = np.ascontiguousarray(np.random.default_rng(SEED).integers(0, 2048, size=(FRAMES, 16)), np.int64)
    stop = threading.Event()

    def flip():   # (the cap between 0 and 8, never -1: this thread makes no HIP call)
        i = 0
        while not stop.is_set():
            lib.voc_set_exact_fp32(i & 1)
            lib.voc_set_fused_units((i >> 1) & 1)
            lib.voc_set_max_workgroups(8 if (i >> 2) & 1 else 0)
            i += 1

    flipper = threading.Thread(target=flip, daemon=True)
    vg.reset(lib)
    h = lib.voc_load(path.encode(), 40, 2)
    assert h
    try:
        refs = {}
        for exact in (0, 1):
            for fused in (0, 1):
                vg.reset(lib)
                lib.voc_set_exact_fp32(exact)
                lib.voc_set_fused_units(fused)
                refs[exact, fused] = synth(lib, h, codes)
                np.testing.assert_array_equal(synth(lib, h, codes), refs[exact, fused])   # deterministic
        vg.reset(lib)
        assert all(len(r) == len(refs[0, 0]) for r in refs.values())
        # the test's condition: the two arithmetics give different bits, so a mixture could be told from either
        for fused in (0, 1):
            assert np.any(refs[0, fused].view(np.uint32) != refs[1, fused].view(np.uint32))

        def mode_of(y):   # -> the arithmetic of the reference y equals bit for bit, None for a mixture
            for (exact, fused), r in refs.items():
                if np.array_equal(y.view(np.uint32), r.view(np.uint32)):
                    return exact
            return None

        flipper.start()
        seen = {0: 0, 1: 0}
        calls = 0
        while calls < 1000 and (calls < 100 or not (seen[0] and seen[1])):
            m = mode_of(synth(lib, h, codes))
            calls += 1
            assert m is not None, f"call {calls}: the output is none of the four settings' outputs (a mixture)"
            seen[m] += 1
        print(f"{calls} calls under the setter storm: {seen[1]} exact, {seen[0]} split")
        assert seen[0] and seen[1], f"after {calls} calls only one arithmetic was seen: {seen}"
    finally:
        stop.set()
        if flipper.is_alive():
            flipper.join()
        vg.reset(lib)
        lib.voc_free(h)
