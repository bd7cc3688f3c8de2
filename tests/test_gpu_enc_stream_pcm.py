"""The streaming encode's PCM front-end on the GPU (csrc/q3_enc_stream_pcm.hip: enc_stream_push_pcm and the hook
enc_stream_debug_push_pcm), held to include/qwen3tts_enc_stream_pcm.h.  No tolerance anywhere but the last line of 1:

1. samples: joined over any split, the 24 kHz float32 samples a stream hands to the op table (through the hook) are equal as
   uint32 to the row enc_debug_pcm prepares for the whole clip, every push hands out what enc_stream_pcm_samples says, and the
   samples pass tests/test_gpu_enc_pcm.py's grade against tests/pcm_ref.py with that file's derived bound, unchanged;
2. ids: push_pcm's joined ids are those of enc_stream_push fed enc_debug_pcm's samples, whatever the split; frame counts are
   enc_pcm_frames';
3. independence: streams at different phases in one call, five streams at five rates round-robin (the handle keeps four tap
   tables: evictions), a stream reused after reset at another rate and format, a clip longer than the handle's max_samples;
4. every refusal leaves the interrupted clip as it was (samples and ids still bit-equal) and the memory figures still;
5. a single-entry push costs at most two launches more than the plain push of its samples;
6. the CLI's --resample device --push_seconds writes the ids of push_pcm driven by hand."""
import json
import os

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.encoder import Encoder
from tests import enc_common as C
from tests import pcm_ref as P
from tests import pcm_stream_ref as S
from tests.test_gpu_enc_pcm import EXTRA, RATES, clip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mimi_encode_golden.npz")
MAX_SAMPLES, MAX_BATCH, MAX_STREAMS, MAX_PUSH = 6000, 3, 5, 2500
HOP = 1920
CASES = [(r, c) for r in RATES for c in (1, 2, 3)] + [(r, c) for r, c in EXTRA]


@pytest.fixture(scope="module")
def rig(gpu_lib, tmp_path_factory):
    """(encoder, its container's path, one stream object for the module)"""
    gold = np.load(GOLDEN)
    keys = json.loads(bytes(gold["mimi.keys"]).decode())
    state = C.seeded_state(C.CASES["mimi"]["seed"], [(k, tuple(s)) for k, s in keys])
    _, t, _ = W.state_to_enc(state, json.loads(bytes(gold["mimi.config"]).decode()), 16)
    path = str(tmp_path_factory.mktemp("enc_stream_pcm") / "enc_mimi.q3w")
    W.write_pack(path, {"enc_sample_rate": 24000.0}, t)
    e = Encoder(path, max_batch=MAX_BATCH, max_samples=MAX_SAMPLES)
    st = e.stream(MAX_STREAMS, MAX_PUSH)
    assert e.samples_per_frame == HOP
    yield e, path, st
    st.close()
    e.close()


def whole_row(enc, x, rate, ch):
    """enc_debug_pcm's row of the whole clip: float32 [n_out]"""
    fmt, n, flat = Encoder._pcm_payload([x], ch)
    up, down = P.factors(rate)
    n_out = P.out_len(n[0], up, down)
    out = np.full((1, (n_out + 31) // 32 * 32), np.nan, np.float32)
    got_n, ld = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert enc.lib.enc_debug_pcm(enc.h, flat.ctypes.data, fmt, ch, rate, hiplib.iptr(n), 1, hiplib.fptr(out), hiplib.iptr(got_n),
                                 hiplib.iptr(ld)) == 0
    assert int(got_n[0]) == n_out
    return out[0, :n_out].copy()


def raw_push(st, entries, rate, ch, fmt=None, cap=None, hook=True):
    """one enc_stream_debug_push_pcm (hook=False: enc_stream_push_pcm) -> (rc, per entry (ids, samples)); on a refusal nothing
    may have been written"""
    sidx = np.array([e[0] for e in entries], np.int32)
    fin = np.array([int(bool(e[2])) for e in entries], np.int32)
    f, n_in, flat = Encoder._pcm_payload([e[1] for e in entries], ch)
    fmt = f if fmt is None else fmt
    codes = np.full((64, st.n_q), -7, np.int64)
    off = np.full(len(sidx) + 1, -7, np.int64)
    soff = np.full(len(sidx) + 1, -7, np.int64)
    samples = np.full(len(sidx) * MAX_PUSH + 1, np.float32(-7.0), np.float32)
    args = (st.h, len(sidx), hiplib.iptr(sidx), flat.ctypes.data, fmt, ch, rate, hiplib.iptr(n_in), hiplib.iptr(fin),
            codes.ctypes.data_as(hiplib.i64p), 64 if cap is None else cap, off.ctypes.data_as(hiplib.i64p))
    if hook:
        rc = st.lib.enc_stream_debug_push_pcm(*args, hiplib.fptr(samples), soff.ctypes.data_as(hiplib.i64p))
    else:
        rc = st.lib.enc_stream_push_pcm(*args)
    if rc != 0:
        assert rc < 0 and (codes == -7).all() and (off == -7).all() and (soff == -7).all() and (samples == -7).all()
        return rc, None
    return 0, [(codes[off[i]:off[i + 1]].copy(), samples[soff[i]:soff[i + 1]].copy() if hook else None) for i in range(len(sidx))]


def run_streams(st, jobs, ch=1):
    """jobs: {stream: (clip, rate, [(frames, finish)])}.  Call by call, the streams whose next push has the same rate go together
    (one rate per call), lowest stream first -> {stream: (ids, samples)}; checks both hand-out rules after every push."""
    for k in jobs:
        st.reset(k)
    at, step = {k: 0 for k in jobs}, {k: 0 for k in jobs}
    got = {k: ([], []) for k in jobs}
    while any(step[k] < len(jobs[k][2]) for k in jobs):
        live = [k for k in jobs if step[k] < len(jobs[k][2])]
        rate = jobs[live[0]][1]
        live = [k for k in live if jobs[k][1] == rate]
        entries = []
        for k in live:
            size, fin = jobs[k][2][step[k]]
            entries.append((k, jobs[k][0][at[k]:at[k] + size], fin))
            at[k] += size
        rc, outs = raw_push(st, entries, rate, ch)
        assert rc == 0, f"push refused: {[(k, e[1].shape, e[2]) for k, e in zip(live, entries)]} at {rate} Hz"
        for k, (ids, smp) in zip(live, outs):
            fin = jobs[k][2][step[k]][1]
            got[k][0].append(ids)
            got[k][1].append(smp)
            have = sum(x.size for x in got[k][1])
            want = st.pcm_samples(rate, at[k], fin)
            assert have == want == S.total(at[k], rate, fin), f"stream {k}: {have} samples after {at[k]} frames (finish={fin}), the rule says {want}"
            frames = sum(len(x) for x in got[k][0])
            assert frames == (-(-have // HOP) if fin else have // HOP), f"stream {k}: {frames} frames from {have} samples (finish={fin})"
            step[k] += 1
    for k in jobs:
        assert at[k] == jobs[k][0].shape[0]
    return {k: (np.concatenate(got[k][0]), np.concatenate(got[k][1])) for k in jobs}


def same_bits(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and a[1].shape == b[1].shape and \
        np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def plain_ids(st, k, y, push=MAX_PUSH):
    """enc_stream_push of 24 kHz float32 samples on stream k -> ids"""
    st.reset(k)
    parts = [st.push([(k, y[a:a + push], a + push >= y.size)])[0] for a in range(0, max(y.size, 1), push)]
    return np.concatenate(parts)


@pytest.mark.parametrize("fmt", ["s16", "f32"])
@pytest.mark.parametrize("rate,ch", CASES)
def test_samples_any_split(rig, rate, ch, fmt):
    enc, _, st = rig
    up, down, half, J = S.geometry(rate)
    r = np.random.default_rng(rate * 16 + ch * 2 + (fmt == "f32"))
    n = -(-700 * down // up) + int(r.integers(0, 5))
    x = clip(r, fmt, n, ch)
    row = whole_row(enc, x, rate, ch)
    want, mag = P.prepare(x, rate, ch, want_mag=True)
    assert row.size == want.size and 690 <= row.size <= 720
    for kind in ("one", "frames", "short", "finish_alone"):
        sp = S.splits(n, J, kind, seed=rate + ch)
        assert all(s <= st.pcm_max_frames_in(rate) for s, _ in sp)
        if kind == "short":
            assert all(s < max(J - 1, 2) for s, _ in sp) and any(s == 0 for s, _ in sp)
        if kind == "frames":
            assert all(s == 1 for s, _ in sp[:min(2 * J, n - 1)])
        ids, got = run_streams(st, {1: (x, rate, sp)}, ch)[1]
        assert got.size == row.size and np.array_equal(got.view(np.uint32), row.view(np.uint32)), \
            f"{rate} Hz {fmt} x{ch} split '{kind}': {int((got.view(np.uint32) != row.view(np.uint32)).sum())} samples are not the whole clip's bits"
        assert ids.shape == (enc.pcm_frames(n, rate), 16)
    # tests/test_gpu_enc_pcm.py's grade of the samples, its bound unchanged
    bound = 2.0 ** -24 * np.abs(want) + 1e-12 * mag + 2.0 ** -149
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), f"{rate} Hz {fmt} x{ch}: {float((err / bound).max()):.3f} of the bound"


@pytest.mark.parametrize("rate,ch,fmt", [(16000, 2, "s16"), (44100, 1, "f32"), (24000, 1, "f32"), (8120, 1, "s16")])
def test_ids_are_the_plain_streams(rig, rate, ch, fmt):
    enc, _, st = rig
    up, down, half, J = S.geometry(rate)
    n = -(-(3 * HOP + 200) * down // up)
    if fmt == "s16":
        x = np.stack([(C.seeded_clip(8 + c, n) * (20000 - 5000 * c)) for c in range(ch)], 1).astype(np.int16).reshape((n, ch) if ch > 1 else (n,))
    else:
        x = np.stack([C.seeded_clip(18 + c, n) for c in range(ch)], 1).astype(np.float32).reshape((n, ch) if ch > 1 else (n,))
    row = whole_row(enc, x, rate, ch)
    want = plain_ids(st, 0, row)
    assert want.shape == (enc.pcm_frames(n, rate), 16) == (4, 16) and len({tuple(f) for f in want.tolist()}) > 1
    most = st.pcm_max_frames_in(rate)
    assert most >= (MAX_PUSH - 32) * down // up
    for kind in ("big", "frames", "finish_alone"):
        sp = [(min(most, n - a), a + most >= n) for a in range(0, n, most)] if kind == "big" else S.splits(n, J, kind, seed=3)
        got = run_streams(st, {2: (x, rate, sp)}, ch)[2]
        assert np.array_equal(got[0], want), f"{rate} Hz split '{kind}': ids differ from enc_stream_push of the same samples"
        assert np.array_equal(got[1].view(np.uint32), row.view(np.uint32))
    # the product entry point and the whole-clip helper give the hook's ids
    assert np.array_equal(enc.encode_streaming_pcm(x, rate, channels=ch, push_frames=777, max_push_samples=MAX_PUSH), want)


def test_streams_do_not_see_each_other(rig):
    enc, _, st = rig
    r = np.random.default_rng(3)
    # three streams at one rate, different clips and phases, in the same calls
    rate, J = 22050, S.geometry(22050)[3]
    clips = [clip(r, "s16", n, 1) for n in (600, 1400, 2200)]
    kinds = ("frames", "finish_alone", "short")
    alone = [run_streams(st, {k: (clips[k], rate, S.splits(clips[k].shape[0], J, "one"))})[k] for k in range(3)]
    both = run_streams(st, {k: (clips[k], rate, S.splits(clips[k].shape[0], J, kinds[k], seed=k)) for k in range(3)})
    for k in range(3):
        assert same_bits(both[k], alone[k]), f"stream {k} changes beside the others"
        assert np.array_equal(alone[k][1].view(np.uint32), whole_row(enc, clips[k], rate, 1).view(np.uint32))
    # five streams at five rates, round-robin: the handle keeps four tap tables
    rates = (8000, 11025, 16000, 44100, 48000)
    xs = [clip(r, "f32", -(-900 * P.factors(q)[1] // P.factors(q)[0]), 1) for q in rates]
    solo = [run_streams(st, {0: (xs[k], rates[k], S.splits(xs[k].shape[0], S.geometry(rates[k])[3], "one"))})[0] for k in range(5)]
    jobs = {k: (xs[k], rates[k], [(s, f) for s, f in S.splits(xs[k].shape[0], S.geometry(rates[k])[3], "finish_alone", seed=k)]) for k in range(5)}
    # (run_streams sends one rate per call; interleave by hand so that every call changes the rate)
    for k in jobs:
        st.reset(k)
    at, got = [0] * 5, [([], []) for _ in range(5)]
    steps = max(len(jobs[k][2]) for k in jobs)
    for i in range(steps):
        for k in range(5):
            if i < len(jobs[k][2]):
                size, fin = jobs[k][2][i]
                rc, outs = raw_push(st, [(k, xs[k][at[k]:at[k] + size], fin)], rates[k], 1)
                assert rc == 0
                at[k] += size
                got[k][0].append(outs[0][0])
                got[k][1].append(outs[0][1])
    for k in range(5):
        assert same_bits((np.concatenate(got[k][0]), np.concatenate(got[k][1])), solo[k]), f"{rates[k]} Hz: the round-robin changes the bits"
    # a stream reused after reset at another rate, format and channel count
    y = clip(r, "s16", 1500, 2)
    a = run_streams(st, {4: (y, 32000, S.splits(1500, S.geometry(32000)[3], "frames", seed=9))}, 2)[4]
    assert np.array_equal(a[1].view(np.uint32), whole_row(enc, y, 32000, 2).view(np.uint32))


def test_a_clip_longer_than_max_samples(rig):
    enc, _, st = rig
    r = np.random.default_rng(11)
    rate = 16000
    n = (MAX_SAMPLES + 1500) * 2 // 3
    x = clip(r, "s16", n, 1)
    assert enc.pcm_frames(n, rate) < 0                          # the whole-clip call refuses it
    before = st.device_bytes(), st.pcm_device_bytes()
    most = st.pcm_max_frames_in(rate)
    ids, got = run_streams(st, {0: (x, rate, [(min(most, n - a), a + most >= n) for a in range(0, n, most)])})[0]
    assert got.size == MAX_SAMPLES + 1500 and ids.shape == (-(-got.size // HOP), 16)
    # its first max_samples-worth is a prefix no later frame reaches: the whole-clip row of the clip's head, short of the filter's tail
    head = whole_row(enc, x[:4000], rate, 1)
    settled = S.ready(4000, rate)
    assert np.array_equal(got[:settled].view(np.uint32), head[:settled].view(np.uint32))
    assert np.array_equal(plain_ids(st, 1, got), ids)
    assert (st.device_bytes(), st.pcm_device_bytes()) == before


def test_every_refusal_leaves_the_clip_alone(rig):
    enc, _, _ = rig
    st = enc.stream(3, MAX_PUSH)
    try:
        r = np.random.default_rng(21)
        rate, ch = 16000, 2
        up, down, half, J = S.geometry(rate)
        n = 3900
        x = clip(r, "f32", n, ch)
        row = whole_row(enc, x, rate, ch)
        bytes0 = st.device_bytes()
        assert st.pcm_device_bytes() == 0
        most = st.pcm_max_frames_in(rate)
        assert most == S.max_frames_in(MAX_PUSH, rate) and most < n
        ok_plain = np.zeros(100, np.float32)

        def refused():
            """every refusal, tried between two pushes of the clip on stream 0"""
            piece = x[1000:1400]
            bad = {
                "another rate": lambda: raw_push(st, [(0, piece, False)], 8000, ch),
                "another channel count": lambda: raw_push(st, [(0, piece[:, 0].copy(), False)], rate, 1),
                "another format": lambda: raw_push(st, [(0, (piece * 1000).astype(np.int16), False)], rate, ch),
                "n_in above max_frames_in": lambda: raw_push(st, [(0, np.zeros((most + 1, ch), np.float32), False)], rate, ch),
                "the same beside a good entry": lambda: raw_push(st, [(1, piece, False), (0, np.zeros((most + 1, ch), np.float32), False)], rate, ch),
                "format 2": lambda: raw_push(st, [(0, piece, False)], rate, ch, fmt=2),
                "9 channels": lambda: raw_push(st, [(0, np.zeros((10, 9), np.float32), False)], rate, 9),
                "rate 7999": lambda: raw_push(st, [(0, piece, False)], 7999, ch),
                "rate 44101 (factor > 640)": lambda: raw_push(st, [(0, piece, False)], 44101, ch),
                "bad stream index": lambda: raw_push(st, [(3, piece, False)], rate, ch),
                "negative stream index": lambda: raw_push(st, [(-1, piece, False)], rate, ch),
                "a stream named twice": lambda: raw_push(st, [(0, piece, False), (0, piece, False)], rate, ch),
                "capacity below the frames": lambda: raw_push(st, [(0, x[1000:1000 + most], True)], rate, ch, cap=0),
                "the product entry, the same": lambda: raw_push(st, [(0, x[1000:1000 + most], True)], rate, ch, cap=0, hook=False),
            }
            for v in (np.nan, np.inf, -np.inf):
                y = piece.copy()
                y[200, 1] = v
                bad[f"a sample that is {v}"] = lambda y=y: raw_push(st, [(0, y, False)], rate, ch)
                bad[f"{v} beside a good entry"] = lambda y=y: raw_push(st, [(1, piece, False), (0, y, False)], rate, ch)
            for what, call in bad.items():
                assert call()[0] < 0, what
            # enc_stream_push on a clip push_pcm has fed
            with pytest.raises(RuntimeError):
                st.push([(0, ok_plain, False)])
            # the query refuses what the push refuses
            sidx, nn, fin = np.array([0], np.int32), np.array([most + 1], np.int32), np.array([0], np.int32)
            q = lambda rt, c, f, k: st.lib.enc_stream_push_pcm_max_frames(st.h, 1, hiplib.iptr(sidx), f, c, rt, hiplib.iptr(k), hiplib.iptr(fin))
            assert q(rate, ch, 1, nn) < 0 and q(8000, ch, 1, np.array([5], np.int32)) < 0 and q(rate, ch, 1, np.array([5], np.int32)) >= 0
            assert q(rate, ch, 1, np.array([-1], np.int32)) < 0

        st.reset(0)
        got = ([], [])
        cuts = [0, 1000, 1000 + 7, 2500, n]
        for i in range(len(cuts) - 1):
            rc, outs = raw_push(st, [(0, x[cuts[i]:cuts[i + 1]], i == len(cuts) - 2)], rate, ch)
            assert rc == 0
            got[0].append(outs[0][0])
            got[1].append(outs[0][1])
            if i == 0:
                pcm_bytes = st.pcm_device_bytes()
                assert pcm_bytes >= 3 * 2 * 160 * 8
            if i < len(cuts) - 2:
                refused()
            assert st.pcm_device_bytes() == pcm_bytes and st.device_bytes() == bytes0
        assert raw_push(st, [(0, x[:10], False)], rate, ch)[0] < 0          # a finished stream without a reset
        assert raw_push(st, [(0, x[:0], True)], rate, ch)[0] < 0
        ids, smp = np.concatenate(got[0]), np.concatenate(got[1])
        assert np.array_equal(smp.view(np.uint32), row.view(np.uint32)), "a refused push has changed the clip's samples"
        # stream 1 was named in refused pushes only; it still takes a plain push from its start, and then refuses push_pcm
        want = plain_ids(st, 1, row)
        assert np.array_equal(ids, want), "a refused push has changed the clip's ids"
        st.reset(1)
        assert len(st.push([(1, row[:100], False)])) == 1
        assert raw_push(st, [(1, x[:10], False)], rate, ch)[0] < 0          # push_pcm on a clip enc_stream_push has fed
        rest = [st.push([(1, row[a:a + MAX_PUSH], a + MAX_PUSH >= row.size)])[0] for a in range(100, row.size, MAX_PUSH)]
        assert np.array_equal(np.concatenate(rest), want)
        # a stream finished with 0 frames gives 0 samples and 0 frames
        st.reset(2)
        rc, outs = raw_push(st, [(2, x[:0], True)], rate, ch)
        assert rc == 0 and outs[0][0].shape == (0, 16) and outs[0][1].size == 0
        assert st.pcm_samples(7999, 10) < 0 and st.pcm_samples(rate, -1) < 0 and st.pcm_max_frames_in(44101) < 0
        assert st.pcm_device_bytes() == pcm_bytes and st.device_bytes() == bytes0
    finally:
        st.close()


def test_launches(rig):
    enc, _, st = rig
    r = np.random.default_rng(5)
    for rate in (16000, 24000):
        up, down, half, J = S.geometry(rate)
        x = clip(r, "s16", -(-2300 * down // up), 1)
        cut = x.shape[0] // 2
        st.reset(0)
        st.reset(1)
        for piece, fin in ((x[:cut], False), (x[cut:], True)):
            rc, outs = raw_push(st, [(0, piece, fin)], rate, 1)
            assert rc == 0
            mine = int(st.lib.enc_stream_last_launches(st.h))
            st.push([(1, outs[0][1], fin)])
            plain = st.last_launches
            print(f"{rate} Hz, finish={fin}: {mine} launches from PCM, {plain} from its samples")
            assert plain > 0 and mine <= plain + 2
            assert mine == plain + (2 if J > 1 else 1)       # (one resample launch, one carry launch where anything is carried)


def test_cli_push_seconds(rig, tmp_path):
    import scipy.io.wavfile as wavfile
    from qwen3_tts_axera_russian_amd import encode_reference_audio as cli
    enc, path, st = rig
    n = 30000
    x = np.stack([(C.seeded_clip(8, n) * 20000), (C.seeded_clip(9, n) * 9000)], 1).astype(np.int16)
    wav, out = tmp_path / "x.wav", tmp_path / "ids.npy"
    wavfile.write(str(wav), 44100, x)
    assert cli.main(["--audio", str(wav), "--model", path, "--output", str(out), "--resample", "device", "--push_seconds", "0.3"]) == 0
    got = np.load(out)
    st.reset(0)
    parts = [st.push_pcm([(0, x[a:a + 1000], a + 1000 >= n)], 44100, channels=2)[0] for a in range(0, n, 1000)]
    want = np.concatenate(parts)
    assert got.dtype == np.int64 and want.shape == (-(-P.out_len(n, *P.factors(44100)) // HOP), 16)
    assert np.array_equal(got, want)
