"""tests/pcm_ref.py, the float64 restatement the device front-end is graded against (tests/test_gpu_enc_pcm.py), held
against scipy: resample_poly in float64 at the common rates, the tap formula against firwin, and the s16 decode / downmix
against the CLI's load_wav.  CPU only."""
import wave

import numpy as np
import pytest

from tests import pcm_ref as P

RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000)


def lengths(up, down):
    """1, 2, 7, lengths whose n * up is a multiple of down and ones where it is not, one past the filter's reach"""
    ns = {1, 2, 7, down, 3 * down, down + 1, 5 * down - 1, 1000, 20 * max(up, down) // up + 300}
    assert any(n * up % down == 0 for n in ns) and (down == 1 or any(n * up % down for n in ns))
    return sorted(ns)


@pytest.mark.parametrize("rate", RATES)
def test_against_resample_poly(rate):
    from scipy.signal import resample_poly
    up, down = P.factors(rate)
    r = np.random.default_rng(rate)
    worst, bits = 0.0, 0
    for n in lengths(up, down):
        x = (0.5 * r.standard_normal(n)).astype(np.float32)
        want = resample_poly(x.astype(np.float64), up, down)
        got = P.resample(x.astype(np.float64), rate)
        assert got.shape == want.shape == (P.out_len(n, up, down),)
        worst = max(worst, float(np.abs(got - want).max()))
        bits += int((got.astype(np.float32).view(np.uint32) != want.astype(np.float32).view(np.uint32)).sum())
    print(f"rate {rate}: up/down {up}/{down}, largest |pcm_ref - resample_poly| {worst:.2e}, {bits} float32 roundings differ")
    assert worst <= 1e-12


@pytest.mark.parametrize("mr_pair", [(3, 1), (3, 2), (2, 1), (1, 2), (80, 147), (160, 147), (320, 147), (1, 4), (600, 203)])
def test_taps_against_firwin(mr_pair):
    from scipy.signal import firwin
    up, down = mr_pair
    mr = max(up, down)
    h, half = P.taps(up, down)
    want = up * firwin(2 * 10 * mr + 1, 1.0 / mr, window=("kaiser", 5.0))
    assert half == 10 * mr and h.shape == want.shape
    d = float(np.abs(h - want).max())
    print(f"up/down {up}/{down}: largest |taps - up * firwin| {d:.2e}")
    assert d <= 1e-14     # (taps are at most up / mr <= 1 in size: some tens of ulps, the freedom of the sum's order)


def test_no_filter_at_24k():
    h, half = P.taps(*P.factors(24000))
    assert h.tolist() == [1.0] and half == 0
    x = np.random.default_rng(1).standard_normal(50)
    assert np.array_equal(P.resample(x, 24000), x)


@pytest.mark.parametrize("channels", [1, 2])
def test_s16_downmix_is_load_wav(channels, tmp_path):
    from qwen3_tts_axera_russian_amd.encode_reference_audio import load_wav
    r = np.random.default_rng(channels)
    x = r.integers(-32768, 32768, size=(500, channels)).astype(np.int16)
    x[:4] = [[-32768] * channels, [32767] * channels, [-32768, 32767][:channels], [1, -2][:channels]]
    path = str(tmp_path / "c.wav")
    with wave.open(path, "w") as wf:
        wf.setnchannels(channels)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(x.tobytes())
    want, sr = load_wav(path)
    got = P.decode(x if channels > 1 else x[:, 0], channels).astype(np.float32)
    assert sr == 16000 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
