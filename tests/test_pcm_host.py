"""csrc/q3_enc_pcm_host.h, the host arithmetic of the encoder's PCM front-end, through tests/pcm_host_driver.cpp: the reduced
factors, n_out, the tap design against scipy, the device's phase layout, and every refusal.  The driver is built twice from
the header alone (it is plain C++: no HIP, no library) -- plain, and with -fsanitize=address,undefined
-fno-sanitize-recover=undefined -- and every case runs through both builds; the sanitized one is a stand-alone program run
on the CPU, nothing is preloaded into it.

Taps: the largest |h - up * firwin(20 mr + 1, 1 / mr, window=("kaiser", 5.0))| over mr in {2, 3, 147, 160, 320, 640} was
measured at 8.9e-16 (printed below; the taps reach up / mr <= 1, so a few ulps); that is below 1e-15, so the bound is 1e-13.  The I0 series and libm's sin / sqrt are the
only freedom.  CPU only."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pcm_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAP_BOUND = 1e-13
# (up, down) with max(up, down) = 2, 3, 147, 160, 320, 640, by factors: no rate of 8000..192000 Hz reduces to exactly 640
# (640 does not divide 24000, and down = 640 needs up in {1, 3}: megahertz); 600/203 is 8120 Hz, the largest table a rate gives
TAP_FACTORS = [(1, 2), (3, 1), (80, 147), (160, 147), (320, 147), (3, 640), (639, 640), (600, 203)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pcm_host") / f"pcm_host_driver_{request.param}")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror"] + flags +
                          [os.path.join(ROOT, "tests", "pcm_host_driver.cpp"), "-o", exe])
    return exe


def run(driver, *args):
    r = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (args, r.returncode, r.stderr[-2000:])
    out = r.stdout.strip()
    if out == "refused":
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[qwen3tts] ")]
        assert len(lines) == 1, f"{args}: a refusal logs one line, got {r.stderr!r}"
        return None
    assert not r.stderr, r.stderr
    return out.split()


@pytest.mark.parametrize("rate", [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000, 9225, 8120])
def test_plan(driver, rate):
    got = run(driver, "plan", 0, 1, rate)
    g = math.gcd(rate, 24000)
    up, down = 24000 // g, rate // g
    mr = max(up, down)
    half = 0 if mr == 1 else 10 * mr
    n = 2 * half + 1
    J = -(-n // up)
    assert got == ["plan"] + [str(v) for v in (up, down, half, n, J, 255 * down // up + 1 + J)]
    assert (up, down) == P.factors(rate) and n <= 12801


def test_clip_lengths(driver):
    for rate in (8000, 16000, 22050, 24000, 44100, 48000, 192000):
        up, down = P.factors(rate)
        for n in (1, 2, 7, down, down + 1, 3 * down - 1, 100000):
            want = -(-n * up // down)
            assert run(driver, "clip", rate, n, 1 << 30) == ["n_out", str(want)], (rate, n)
            assert want == P.out_len(n, up, down)
    # the limits of n_out: exactly max_samples passes, one more does not
    assert run(driver, "clip", 48000, 2000, 1000) == ["n_out", "1000"]
    assert run(driver, "clip", 48000, 2001, 1000) is None
    assert run(driver, "clip", 8000, 333, 1000) == ["n_out", "999"]
    assert run(driver, "clip", 8000, 334, 1000) is None


def test_refusals(driver):
    assert run(driver, "plan", 0, 1, 16000) and run(driver, "plan", 1, 8, 16000)
    for fmt in (-1, 2):
        assert run(driver, "plan", fmt, 1, 16000) is None
    for ch in (0, -1, 9):
        assert run(driver, "plan", 0, ch, 16000) is None
    for rate in (0, -16000, 7999, 192001, 1 << 30):
        assert run(driver, "plan", 0, 1, rate) is None
    # inside the range, but max(up, down) > 640: 8001 (8000 / 2667), 44101, 9226 (up 12000), 191999
    for rate in (8001, 44101, 9226, 191999, 23999):
        g = math.gcd(rate, 24000)
        assert max(24000 // g, rate // g) > 640
        assert run(driver, "plan", 0, 1, rate) is None
    assert run(driver, "plan", 0, 1, 8120)[1:3] == ["600", "203"]      # the largest factor a rate in the range reduces to
    assert run(driver, "taps", 641, 640, "/dev/null") is None and run(driver, "taps", 0, 1, "/dev/null") is None
    # n_out of 0 (no frames), negative lengths, above max_samples
    for n in (0, -1, -(1 << 31)):
        assert run(driver, "clip", 16000, n, 1000) is None
    assert run(driver, "clip", 16000, 1000, 1499) is None and run(driver, "clip", 16000, 1000, 1500) == ["n_out", "1500"]
    # lengths whose n * up leaves 32 bits (and, read as 64-bit text, 31 bits): refused, never wrapped into a small n_out
    for n in ((1 << 31) - 1, (1 << 31) // 3 + 1, 1 << 31, 1 << 32, (1 << 32) + 5, (1 << 62)):
        assert run(driver, "clip", 8000, n, (1 << 31) - 1) is None, n
        if n >= (1 << 31) - 1:
            assert run(driver, "clip", 8120, n, (1 << 31) - 1) is None, n
    assert run(driver, "clip", 8000, 715827882, (1 << 31) - 1) == ["n_out", str(715827882 * 3)]   # the largest that fits


def test_taps_against_scipy(driver, tmp_path):
    from scipy.signal import firwin
    worst = 0.0
    for up, down in TAP_FACTORS:
        mr = max(up, down)
        path = str(tmp_path / f"taps_{up}_{down}.bin")
        assert run(driver, "taps", up, down, path) == ["taps", str(20 * mr + 1)]
        h = np.fromfile(path, np.float64)
        want = up * firwin(20 * mr + 1, 1.0 / mr, window=("kaiser", 5.0))
        d = float(np.abs(h - want).max())
        worst = max(worst, d)
        print(f"mr {mr} ({up}/{down}): largest |taps - up * firwin| {d:.2e}, against pcm_ref "
              f"{float(np.abs(h - P.taps(up, down)[0]).max()):.2e}")
        assert d <= TAP_BOUND
        # the device's layout: [j][phase] = h[phase + j * up], zero past the last tap
        assert run(driver, "poly", up, down, path) == ["poly", str(-(-h.size // up)), str(up)]
        t = np.fromfile(path, np.float64)
        padded = np.concatenate([h, np.zeros(t.size - h.size)])
        assert np.array_equal(t, padded)       # (row-major [j][up] of h[j * up + phase] is h itself, zero padded)
    print(f"largest tap difference over all: {worst:.2e} (bound {TAP_BOUND:.0e})")


def test_no_filter(driver, tmp_path):
    path = str(tmp_path / "t.bin")
    assert run(driver, "plan", 0, 1, 24000) == ["plan", "1", "1", "0", "1", "1", "257"]
    assert run(driver, "taps", 1, 1, path) == ["taps", "1"] and np.fromfile(path, np.float64).tolist() == [1.0]
