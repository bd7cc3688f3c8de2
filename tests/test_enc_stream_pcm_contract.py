"""The streaming encode's PCM front-end (enc_stream_push_pcm, include/qwen3tts_enc_stream_pcm.h) without a GPU.

1. The host arithmetic (csrc/q3_enc_stream_pcm_host.h) through tests/pcm_stream_host_driver.cpp, a stand-alone program built
   from the two host headers alone, plain (every reduced (up, down) a rate of 8000..192000 Hz gives) and with
   -fsanitize=address,undefined (a comb of them and the listed rates); nothing is preloaded into it.  It requires the hand-out
   rule after every push, the joined output bit-equal to the whole-clip sum, max_frames_in sufficient at every phase and
   above its floor.
2. tests/pcm_stream_ref.py, the numpy restatement of the rule, against tests/pcm_ref.resample of the whole clip on the same
   kinds of splits: the same float64 bits (both add the same products in the same order).
3. The ABI: the header declares exactly its five names, qwen3tts_enc.h includes it, the library exports them and the hook
   enc_stream_debug_push_pcm, hiplib declares them, the new kernels are held to no spills, the host header names no device
   header.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import pcm_ref as P
from tests import pcm_stream_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen3_tts_axera_russian_amd", "csrc")
NAMES = ["enc_stream_pcm_device_bytes", "enc_stream_pcm_max_frames_in", "enc_stream_pcm_samples", "enc_stream_push_pcm",
         "enc_stream_push_pcm_max_frames"]
RATES = (8000, 8120, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 184000, 192000)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver(build, tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / f"pcm_stream_host_driver_{build}")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if build == "sanitized" else ["-O2"]
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "pcm_stream_host_driver.cpp"), "-o", exe])
    r = subprocess.run([exe] + (["9"] if build == "sanitized" else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    word, pairs, pushes = r.stdout.split()
    print(f"{build}: {pairs} (up, down) pairs, {pushes} pushes")
    assert word == "ok" and int(pairs) >= (5000 if build == "plain" else 500) and int(pushes) > 10 * int(pairs)


@pytest.mark.parametrize("rate", RATES)
def test_numpy_restatement_against_the_whole_clip(rate):
    up, down, half, J = S.geometry(rate)
    assert J - 1 <= 160 and (rate != 24000 or (J == 1 and S.ready(7, rate) == 7))
    r = np.random.default_rng(rate)
    for n in (0, 1, J, 5 * J + 3 + int(r.integers(0, 2 * down))):
        x = r.standard_normal(n)
        want = P.resample(x, rate) if n else np.zeros(0)
        for kind in ("one", "frames", "short", "finish_alone"):
            st, got, at = S.Stream(rate), [], 0
            for size, fin in S.splits(n, J, kind, seed=n):
                y = st.push(x[at:at + size], fin)
                at += size
                got.append(y)
                have = sum(g.size for g in got)
                assert have == S.total(at, rate, fin) == (P.out_len(at, up, down) if fin else S.ready(at, rate)), (rate, n, kind, at)
                if not fin:      # exactly the outputs whose newest frame has arrived
                    assert have == sum(1 for m in range(P.out_len(at, up, down) + 1) if (m * down + half) // up <= at - 1)
            assert at == n
            got = np.concatenate(got) if got else np.zeros(0)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (rate, n, kind)
        tail = P.out_len(n, up, down) - S.ready(n, rate)
        assert 0 <= tail <= 31
    for max_push in (32, 1920, 24000):
        k = S.max_frames_in(max_push, rate)
        assert k >= (max_push - 32) * down // up
        for n0 in range(0, 2 * down + half // up + 3):
            assert S.total(n0 + k, rate, True) - S.ready(n0, rate) <= max_push, (rate, max_push, n0)


def test_header_exports_and_declarations():
    from qwen3_tts_axera_russian_amd import build, hiplib
    src = open(os.path.join(ROOT, "include", "qwen3tts_enc_stream_pcm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(enc_[a-z0-9_]+)\s*\(", code))) == NAMES
    assert "bit" in src and "enc_stream_pcm_device_bytes: 0 before" in src       # the contract and the memory rule are stated
    assert '#include "qwen3tts_enc_stream_pcm.h"' in open(os.path.join(ROOT, "include", "qwen3tts_enc.h")).read()
    lib = ctypes.CDLL(build.build())
    for name in NAMES + ["enc_stream_debug_push_pcm"]:
        assert hasattr(lib, name), name
    assert "q3_enc_stream_pcm.hip" in build.SOURCES
    assert {"enc_stream_pcm_kernel", "enc_stream_pcm_carry_kernel"} <= set(build.NO_SPILL)
    res = build.kernel_resources(build.build())
    mine = {k: v for k, v in res.items() if "enc_stream_pcm" in k}
    assert len(mine) == 2 and all(v[2] == 0 and v[3] == 0 for v in mine.values()), mine      # no spills, no scratch
    h = hiplib.load()
    assert h.enc_stream_pcm_samples.restype is ctypes.c_int64 and len(h.enc_stream_pcm_samples.argtypes) == 4
    assert len(h.enc_stream_pcm_max_frames_in.argtypes) == 2 and len(h.enc_stream_push_pcm_max_frames.argtypes) == 8
    assert h.enc_stream_push_pcm.restype is ctypes.c_int and len(h.enc_stream_push_pcm.argtypes) == 12
    assert len(h.enc_stream_pcm_device_bytes.argtypes) == 1 and len(h.enc_stream_debug_push_pcm.argtypes) == 14
    # no object: refused, no device touched
    assert h.enc_stream_pcm_samples(None, 16000, 100, 0) < 0 and h.enc_stream_pcm_max_frames_in(None, 16000) < 0
    assert h.enc_stream_pcm_device_bytes(None) < 0


def test_the_host_header_stands_alone():
    src = open(os.path.join(CSRC, "q3_enc_stream_pcm_host.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["q3_enc_pcm_host.h"]
    assert "hip" not in re.sub(r"//.*", "", src).lower()
    drv = open(os.path.join(ROOT, "tests", "pcm_stream_host_driver.cpp")).read()
    inc = re.findall(r'#include\s+[<"]([^>"]+)[>"]', drv)
    assert [i for i in inc if i.endswith(".h")] == ["../qwen3_tts_axera_russian_amd/csrc/q3_enc_stream_pcm_host.h"]
