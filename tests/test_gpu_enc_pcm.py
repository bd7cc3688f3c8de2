"""The encoder's PCM front-end on the GPU (csrc/q3_enc_pcm.hip: enc_encode_pcm, enc_pcm_frames, the hook enc_debug_pcm).

Prepared rows (the 24 kHz mono f32 the encoder then reads, through the hook, so the quantiser does not blur the grade)
against tests/pcm_ref.py, the float64 restatement that tests/test_pcm_reference.py holds against scipy.  Per sample

    |y - y_ref| <= 2^-24 |y_ref| + 1e-12 sum |x_i| + 2^-149

derived, not measured: the one rounding of the float64 sum to float32 (half an ulp: 2^-24 relative, 2^-149 where the result
is subnormal), and for the sum itself -- at most 162 terms of float64 products against taps that differ from scipy's by
below 1e-15 -- 1e-12 of the magnitudes x_i (the downmixed samples in the output's support), a few thousand times what
float64 loses.  How many samples differ from float32(y_ref) in their bits is printed (0 expected, not asserted).

Then the ids: enc_encode_pcm against enc_encode of the same samples, a clip alone against the clip in a batch,
enc_pcm_frames, and every error path with the handle still good afterwards.  One handle serves the whole module, so its
tap tables (four kept) are evicted and rebuilt along the way."""
import json
import os

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.encoder import Encoder
from tests import enc_common as C
from tests import pcm_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mimi_encode_golden.npz")
MAX_SAMPLES, MAX_BATCH = 6000, 3
RATES = (8000, 16000, 22050, 44100, 48000, 24000)
# beyond the issue's list: the longest windows (192 kHz: 8 input frames per output), 8 channels, and 8120 Hz = 600/203, the
# largest tap table a rate in the range gives (101 KB of LDS)
EXTRA = ((11025, 1), (32000, 2), (88200, 1), (192000, 8), (8120, 1))


@pytest.fixture(scope="module")
def enc(gpu_lib, tmp_path_factory):
    gold = np.load(GOLDEN)
    keys = json.loads(bytes(gold["mimi.keys"]).decode())
    state = C.seeded_state(C.CASES["mimi"]["seed"], [(k, tuple(s)) for k, s in keys])
    _, t, _ = W.state_to_enc(state, json.loads(bytes(gold["mimi.config"]).decode()), 16)
    path = str(tmp_path_factory.mktemp("enc_pcm") / "enc_mimi.q3w")
    W.write_pack(path, {"enc_sample_rate": 24000.0}, t)
    e = Encoder(path, max_batch=MAX_BATCH, max_samples=MAX_SAMPLES)
    yield e
    e.close()


def clip(r, fmt, n, ch):
    shape = (n, ch) if ch > 1 else (n,)
    if fmt == "s16":
        x = r.integers(-32768, 32768, size=shape).astype(np.int16)
        x.reshape(-1)[:2] = [-32768, 32767][:x.size]
        return x
    x = (0.3 * r.standard_normal(shape)).astype(np.float32)
    if x.size > 4:
        x.reshape(-1)[1:4] = [1e-30, -3.5, 0.0]
    return x


def prepared(enc, clips, rate, ch, rc=0):
    """the hook -> (rows [B][ld] as the handle holds them, n_out [B])"""
    fmt, n, flat = Encoder._pcm_payload(clips, ch)
    up, down = P.factors(rate)
    ld = (max(P.out_len(x, up, down) for x in n) + 31) // 32 * 32
    out = np.full((len(clips), ld), np.nan, np.float32)
    n_out, got_ld = np.zeros(len(clips), np.int32), np.zeros(1, np.int32)
    got = enc.lib.enc_debug_pcm(enc.h, flat.ctypes.data, fmt, ch, rate, hiplib.iptr(n), len(clips), hiplib.fptr(out), hiplib.iptr(n_out),
                                hiplib.iptr(got_ld))
    assert got == rc, f"enc_debug_pcm -> {got}"
    if rc == 0:
        assert int(got_ld[0]) == ld
    return out, n_out


def lengths(rate):
    """1, 2, up - 1, one shorter than the filter's half-width in input frames (both edges clip every output), ~700 outputs
    (three workgroups, the last one ragged), and a ragged batch of 3"""
    up, down = P.factors(rate)
    half_in = max(10 * max(up, down) // up - 1, 1)
    long_ = -(-700 * down // up)
    singles = sorted({1, 2, max(up - 1, 1), half_in, long_})
    return singles, (long_ - 3, 7, half_in)


def grade(enc, clips, rate, ch, what):
    rows, n_out = prepared(enc, clips, rate, ch)
    differ = total = 0
    worst = 0.0
    for b, x in enumerate(clips):
        want, mag = P.prepare(x, rate, ch, want_mag=True)
        assert int(n_out[b]) == want.size, f"{what} clip {b}: n_out {n_out[b]}, expected {want.size}"
        got = rows[b, :want.size]
        assert np.isfinite(got).all(), what
        bound = 2.0 ** -24 * np.abs(want) + 1e-12 * mag + 2.0 ** -149
        err = np.abs(got.astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"{what} clip {b}: {float((err / bound).max()):.3f} of the bound at sample {int((err / bound).argmax())}"
        assert not rows[b, want.size:].view(np.uint32).any(), f"{what} clip {b}: the row is not zero past n_out"
        differ += int((got.view(np.uint32) != want.astype(np.float32).view(np.uint32)).sum())
        total += want.size
    return differ, total, worst


@pytest.mark.parametrize("fmt", ["s16", "f32"])
@pytest.mark.parametrize("rate", RATES)
def test_prepared_rows(enc, rate, fmt):
    r = np.random.default_rng(rate + (fmt == "f32"))
    singles, batch = lengths(rate)
    differ = total = 0
    worst = 0.0
    for ch in (1, 2, 3):
        for n in singles:
            d, t, w = grade(enc, [clip(r, fmt, n, ch)], rate, ch, f"{rate} Hz {fmt} x{ch} n={n}")
            differ, total, worst = differ + d, total + t, max(worst, w)
        d, t, w = grade(enc, [clip(r, fmt, n, ch) for n in batch], rate, ch, f"{rate} Hz {fmt} x{ch} batch {batch}")
        differ, total, worst = differ + d, total + t, max(worst, w)
    print(f"{rate} Hz {fmt}: {differ} of {total} samples differ from float32(y_ref) in their bits; worst error {worst:.3f} of the bound")


@pytest.mark.parametrize("rate,ch", EXTRA)
def test_prepared_rows_other_rates(enc, rate, ch):
    r = np.random.default_rng(rate)
    singles, batch = lengths(rate)
    differ = total = 0
    for fmt in ("s16", "f32"):
        for n in singles:
            d, t, _ = grade(enc, [clip(r, fmt, n, ch)], rate, ch, f"{rate} Hz {fmt} x{ch} n={n}")
            differ, total = differ + d, total + t
        d, t, _ = grade(enc, [clip(r, fmt, n, ch) for n in batch], rate, ch, f"{rate} Hz {fmt} x{ch} batch {batch}")
        differ, total = differ + d, total + t
    print(f"{rate} Hz x{ch}: {differ} of {total} samples differ from float32(y_ref) in their bits")


def test_24k_mono_is_the_plain_conversion(enc):
    r = np.random.default_rng(24)
    for n in (1, 255, 256, 257, 1000):
        x = clip(r, "f32", n, 1)
        rows, n_out = prepared(enc, [x], 24000, 1)
        assert n_out[0] == n and np.array_equal(rows[0, :n].view(np.uint32), x.view(np.uint32))
        s = clip(r, "s16", n, 1)
        rows, n_out = prepared(enc, [s], 24000, 1)
        assert n_out[0] == n and np.array_equal(rows[0, :n].view(np.uint32), (s.astype(np.float32) / np.float32(32768.0)).view(np.uint32))
        assert not rows[0, n:].any()


def test_a_longer_call_leaves_no_trace(enc):
    """rows are zero past n_out also right after a longer call wrote the same buffer"""
    r = np.random.default_rng(5)
    prepared(enc, [clip(r, "f32", 3000, 2)] * 3, 16000, 2)
    rows, n_out = prepared(enc, [clip(r, "s16", 40, 1), clip(r, "s16", 3, 1)], 16000, 1)
    assert n_out.tolist() == [60, 5] and not rows[0, 60:].any() and not rows[1, 5:].any()


def test_ids(enc):
    r = np.random.default_rng(77)
    # 24 kHz mono: enc_encode of the same samples
    x = C.seeded_clip(7, 5000)
    assert np.array_equal(enc.encode_pcm([x], 24000)[0], enc.encode([x])[0])
    s = (x * 20000).astype(np.int16)
    assert np.array_equal(enc.encode_pcm([s], 24000)[0], enc.encode([s.astype(np.float32) / 32768.0])[0])
    # 16 kHz stereo s16: enc_encode of the rows the hook returned
    st = np.stack([(C.seeded_clip(8, 3300) * 20000), (C.seeded_clip(9, 3300) * 9000)], 1).astype(np.int16)
    rows, n_out = prepared(enc, [st], 16000, 2)
    assert n_out[0] == 4950
    ids = enc.encode_pcm([st], 16000, channels=2)[0]
    assert enc.last_ms() > 0
    assert ids.shape == (enc.frames(4950), 16) and np.array_equal(ids, enc.encode([rows[0, :4950]])[0])
    assert len({tuple(f) for f in ids.tolist()}) > 1          # (not one constant frame)
    # a clip alone and in a batch, in every position
    others = [clip(r, "s16", n, 2) for n in (1, 2000)]
    for order in ([st] + others, others + [st], [others[0], st, others[1]]):
        got = enc.encode_pcm(order, 16000, channels=2)
        at = [i for i, c in enumerate(order) if c is st][0]
        assert np.array_equal(got[at], ids)
        for i, c in enumerate(order):
            if c is not st:
                assert np.array_equal(got[i], enc.encode_pcm([c], 16000, channels=2)[0])
    # more clips than max_batch: several library calls
    many = enc.encode_pcm([st, others[0], others[1], st], 16000, channels=2)
    assert np.array_equal(many[0], ids) and np.array_equal(many[3], ids)


def test_pcm_frames(enc):
    for rate in RATES + (192000, 8120):
        up, down = P.factors(rate)
        for n in (1, 2, down, 1920 * down // up, 1920 * down // up + 1, 1921 * down // up + 1, MAX_SAMPLES * down // up):
            n_out = P.out_len(n, up, down)
            assert 1 <= n_out <= MAX_SAMPLES
            assert enc.pcm_frames(n, rate) == enc.frames(n_out) == -(-n_out // 1920), (rate, n)
    assert enc.pcm_frames(0, 16000) < 0 and enc.pcm_frames(-5, 16000) < 0
    assert enc.pcm_frames(MAX_SAMPLES * 2 // 3 + 1, 16000) < 0 and enc.pcm_frames(MAX_SAMPLES * 2 // 3, 16000) == enc.frames(MAX_SAMPLES)
    assert enc.pcm_frames(100, 7999) < 0 and enc.pcm_frames(100, 44101) < 0 and enc.pcm_frames(100, 192001) < 0
    assert enc.lib.enc_pcm_frames(None, 100, 16000) < 0


def test_every_error_leaves_the_handle_good(enc):
    st = np.stack([(C.seeded_clip(8, 3300) * 20000), (C.seeded_clip(9, 3300) * 9000)], 1).astype(np.int16)
    want = enc.encode_pcm([st], 16000, channels=2)[0]
    lib, h = enc.lib, enc.h
    codes = np.empty((MAX_BATCH + 1, 8, 16), np.int64)
    nf = np.zeros(MAX_BATCH + 1, np.int32)
    f32 = (0.1 * np.ones(400, np.float32))

    def call(pcm=st, fmt=0, ch=2, rate=16000, n=(3300,), B=None, max_frames=8, handle=h, out=codes, nfp=nf):
        n = np.asarray(n, np.int32)
        return lib.enc_encode_pcm(handle, None if pcm is None else np.ascontiguousarray(pcm).ctypes.data, fmt, ch, rate, hiplib.iptr(n),
                                  len(n) if B is None else B, None if out is None else out.ctypes.data_as(hiplib.i64p), max_frames,
                                  None if nfp is None else hiplib.iptr(nfp))

    def good():
        codes[:] = -7
        assert call() == 0 and nf[0] == want.shape[0] and np.array_equal(codes[0, :nf[0]], want) and (codes[0, nf[0]:] == -1).all()

    good()
    bad_nan, bad_inf = f32.copy(), f32.copy()
    bad_nan[399], bad_inf[0] = np.nan, -np.inf
    cases = {
        "NULL handle": dict(handle=None), "NULL pcm": dict(pcm=None), "NULL codes": dict(out=None), "NULL n_frames": dict(nfp=None),
        "format -1": dict(fmt=-1), "format 2": dict(fmt=2), "0 channels": dict(ch=0), "9 channels": dict(ch=9),
        "rate 7999": dict(rate=7999), "rate 192001": dict(rate=192001), "rate 44101 (factor > 640)": dict(rate=44101), "rate 0": dict(rate=0),
        "B = 0": dict(B=0), "B > max_batch": dict(n=(10,) * (MAX_BATCH + 1)), "0 frames": dict(n=(0,)), "negative frames": dict(n=(-3,)),
        "second clip empty": dict(n=(100, 0)), "n_out above max_samples": dict(n=(4001,)),
        "n * up beyond 32 bits": dict(n=(2 ** 31 - 1,)), "max_frames too small": dict(max_frames=2),
        "NaN sample": dict(pcm=bad_nan, fmt=1, ch=1, n=(400,)), "inf sample": dict(pcm=bad_inf, fmt=1, ch=2, n=(200,)),
    }
    for what, kw in cases.items():
        assert call(**kw) < 0, what
        good()
    big = np.zeros((4000, 2), np.int16)      # exactly max_samples at 24 kHz: taken
    codes[:] = -7
    assert call(pcm=big, n=(4000,)) == 0 and nf[0] == enc.frames(MAX_SAMPLES)
    good()
