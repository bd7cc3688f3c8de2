"""Streaming encode (enc_stream_*, include/qwen3tts_enc_stream.h) on the GPU, held to its four contracts:

1. split invariance, bits: joined per stream, ids and pre-quantiser embeddings (test hook q3t_enc_stream_embeddings) are the
   same for any split of the samples, any n_new pattern (zeros included), any other streams in the same calls, any index;
2. against enc_encode of the same clip: the frame count, embeddings within 2e-4 of the stage's scale (tests/test_gpu_encoder.py's
   stage tolerance), every id equal to enc_encode's or -- graded in float64 from the stream's own embedding, that file's rule --
   within 1e-5 of the nearest entry;
3. hand-out rule: floor(total / hop) frames after every push, enc_frames(total) after the finish;
4. constant memory: enc_stream_device_bytes never moves, and a clip longer than the handle's max_samples is encoded.

Measured on MI355X: the embeddings of a stream and of enc_encode are the same bits while the stream is shorter than the
attention window and differ by rounding after it (the carried-window attention rotates q and k by their offset inside the
window, enc_encode by the absolute column); the figures are printed by the tests."""
import dataclasses
import json
import os

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.encoder import Encoder
from tests import enc_common as C
from tests.enc_ref import rvq_encode
from tests.util import CACHE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mimi_encode_golden.npz")
STAGE_TOL = 2e-4      # of the embedding's scale (max |value|)
DIST_TOL = 1e-5       # relative: an id's float64 distance over the float64 best
GAP_TOL = 1e-4        # a float64 near-tie (the CLI test has no stream embedding to grade from)


@pytest.fixture(scope="module")
def lib(gpu_lib):
    return gpu_lib


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def full_synth():
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, "enc_full_s7.q3w")
    ec = W.EncConfig()
    if not os.path.exists(path):
        W.write_synthetic_enc(path, ec, seed=7)
    _, t = W.read_pack(path)
    return ec, {k: np.asarray(v) for k, v in t.items()}, path


@pytest.fixture(scope="module")
def tiny_synth(tmp_path_factory):
    ec = W.tiny_enc_config()
    path = str(tmp_path_factory.mktemp("encs") / "enc_tiny.q3w")
    t = W.write_synthetic_enc(path, ec, seed=3)
    return ec, t, path


def golden_table(gold, name, tmp):
    keys = json.loads(bytes(gold[f"{name}.keys"]).decode())
    state = C.seeded_state(C.CASES[name]["seed"], [(k, tuple(s)) for k, s in keys])
    assert C.digest(state) == bytes(gold[f"{name}.sha"]).decode()
    ec, t, _ = W.state_to_enc(state, json.loads(bytes(gold[f"{name}.config"]).decode()), 16)
    path = os.path.join(tmp, f"enc_stream_{name}.q3w")
    W.write_pack(path, {"enc_sample_rate": 24000.0}, t)
    return ec, t, path


def hook_push(tl, st, hidden, entries):
    """one push through the test hook -> per entry (ids [frames][n_q], embedding [frames][hidden])"""
    sidx = np.array([e[0] for e in entries], np.int32)
    new = [np.ascontiguousarray(e[1], dtype=np.float32) for e in entries]
    n_new = np.array([x.size for x in new], np.int32)
    fin = np.array([int(e[2]) for e in entries], np.int32)
    pcm = np.concatenate(new + [np.zeros(1, np.float32)])
    cap = int(st.lib.enc_stream_push_max_frames(st.h, len(sidx), hiplib.iptr(sidx), hiplib.iptr(n_new), hiplib.iptr(fin)))
    assert cap >= 0
    codes = np.full((max(cap, 1), st.n_q), -7, np.int64)
    emb = np.zeros((max(cap, 1), hidden), np.float32)
    off = np.zeros(len(sidx) + 1, np.int64)
    ch = np.zeros(1, np.int32)
    rc = tl.q3t_enc_stream_embeddings(st.h, len(sidx), hiplib.iptr(sidx), hiplib.fptr(pcm), hiplib.iptr(n_new), hiplib.iptr(fin),
                                      codes.ctypes.data_as(hiplib.i64p), cap, off.ctypes.data_as(hiplib.i64p), hiplib.fptr(emb),
                                      hiplib.iptr(ch))
    assert rc == 0 and int(ch[0]) == hidden and int(off[-1]) == cap
    return [(codes[off[i]:off[i + 1]].copy(), emb[off[i]:off[i + 1]].copy()) for i in range(len(sidx))]


def splits(n, hop, kind, seed=0):
    """-> [(samples of the push, finish)]: how a clip of n samples reaches its stream"""
    if kind == "one":
        return [(n, True)]
    if kind == "ones":
        return [(1, False)] * n + [(0, True)]
    if kind == "hop":
        sizes = [hop] * (n // hop) + ([n % hop] if n % hop else [])
    elif kind == "edges":
        sizes, left = [], n
        for s in (1, hop - 1, 1, hop, 0):
            s = min(s, left)
            sizes.append(s)
            left -= s
        sizes.append(left)
    elif kind in ("random", "finish_alone"):
        r = np.random.default_rng(seed)
        sizes, left = [], n
        while left > 0:
            s = min(int(r.integers(1, 2 * hop + 1)), left)
            sizes.append(s)
            left -= s
        if kind == "finish_alone":
            return [(s, False) for s in sizes] + [(0, True)]
    else:
        raise ValueError(kind)
    return [(s, i == len(sizes) - 1) for i, s in enumerate(sizes)]


def run_streams(tl, st, ec, jobs):
    """jobs: {stream index: (clip, [(size, finish)])}, the streams' pushes interleaved call by call -> {index: (ids, embedding)};
    checks the hand-out rule after every push."""
    hop = W.enc_hop(ec)
    for k in jobs:
        st.reset(k)
    at = {k: 0 for k in jobs}
    step = {k: 0 for k in jobs}
    got = {k: ([], []) for k in jobs}
    while any(step[k] < len(jobs[k][1]) for k in jobs):
        live = [k for k in jobs if step[k] < len(jobs[k][1])]
        entries = []
        for k in live:
            size, fin = jobs[k][1][step[k]]
            entries.append((k, jobs[k][0][at[k]:at[k] + size], fin))
            at[k] += size
        outs = hook_push(tl, st, ec.hidden, entries)
        for k, (c, e) in zip(live, outs):
            got[k][0].append(c)
            got[k][1].append(e)
            fin = jobs[k][1][step[k]][1]
            have = sum(len(x) for x in got[k][0])
            want = (W.enc_frames(ec, at[k]) if at[k] else 0) if fin else at[k] // hop
            assert have == want, f"stream {k}: {have} frames after {at[k]} samples (finish={fin}), the rule says {want}"
            step[k] += 1
    for k in jobs:
        assert at[k] == jobs[k][0].size
    return {k: (np.concatenate(got[k][0]), np.concatenate(got[k][1])) for k in jobs}


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def debug_embedding(lib, enc, ec, clip):
    n = np.array([clip.size], np.int32)
    n_ops = dict(W.enc_program(ec)[2])["embedding"]
    Cc, L = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert lib.enc_debug_shape(enc.h, hiplib.iptr(n), 1, n_ops, hiplib.iptr(Cc), hiplib.iptr(L)) == 0
    out = np.empty((1, int(Cc[0]), int(L[0])), np.float32)
    assert lib.enc_debug_run(enc.h, hiplib.fptr(np.ascontiguousarray(clip)), hiplib.iptr(n), 1, n_ops, hiplib.fptr(out), hiplib.iptr(Cc),
                             hiplib.iptr(L)) == 0
    return out[0]


def grade(t, emb, codes):
    """tests/test_gpu_encoder.py's grading: float64 distances from the given embedding [hidden][frames] -> worst ratio"""
    prog = np.asarray(t["enc.program"])
    proj = np.asarray(t[f"enc.op{len(prog) - 2}.weight"], np.float64)[:, :, 0]
    books = np.asarray(t[f"enc.op{len(prog) - 1}.codebook"], np.float64)
    _, _, ratio = rvq_encode(proj @ emb.astype(np.float64), books, int(prog[-1][6]), forced=codes)
    return float(ratio.max())


def against_one_shot(lib, enc, ec, t, clip, got, label):
    """contract 2 for one clip; -> (ids that differ, whether the embeddings are the same bits)"""
    codes, emb = got
    ref = enc.encode([clip])[0]
    assert codes.shape == ref.shape == (W.enc_frames(ec, clip.size), 16), label
    ref_emb = debug_embedding(lib, enc, ec, clip)[:, :ref.shape[0]]
    err = float(np.abs(emb.T - ref_emb).max()) / max(float(np.abs(ref_emb).max()), 1e-3)
    ratio = grade(t, emb.T, codes)
    differ = int((codes != ref).sum())
    bits = np.array_equal(emb.T.view(np.uint32), ref_emb.view(np.uint32))
    print(f"{label}: embedding {err:.2e} of its scale from enc_encode's (same bits: {bits}), {differ} of {codes.size} ids differ, "
          f"worst float64 distance ratio {ratio - 1:.2e}")
    assert err <= STAGE_TOL, f"{label}: embedding {err:.2e} of its scale"
    assert ratio <= 1 + DIST_TOL, f"{label}: an id is {ratio - 1:.2e} farther than the float64 best"
    return differ, bits


@pytest.mark.parametrize("name", list(C.CASES))
def test_golden_cases_split_invariance_and_one_shot(lib, test_lib, gold, name, tmp_path):
    case = C.CASES[name]
    ec, t, path = golden_table(gold, name, str(tmp_path))
    hop = W.enc_hop(ec)
    n_long, n_short = max(case["lengths"]), case["lengths"][-2] if name == "mimi" else 1921
    long, short = C.seeded_clip(case["seed"], n_long), C.seeded_clip(case["seed"], n_short)
    assert ec.window < W.enc_frames(ec, n_long) * ec.ds_stride      # the long clip rolls the k|v window over
    enc = Encoder(path, max_batch=2, max_samples=n_long)
    st = enc.stream(3, n_long)
    try:
        bytes0 = st.device_bytes()
        base = run_streams(test_lib, st, ec, {0: (long, splits(n_long, hop, "one"))})[0]
        against_one_shot(lib, enc, ec, t, long, base, f"{name} {n_long}")
        for kind in ("hop", "edges", "random", "finish_alone"):
            got = run_streams(test_lib, st, ec, {0: (long, splits(n_long, hop, kind, seed=5))})[0]
            assert same_bits(got, base), f"{name}: split '{kind}' changes the bits"
        # two streams, different clips and split patterns in the same calls; then the indices swapped
        alone_short = run_streams(test_lib, st, ec, {1: (short, splits(n_short, hop, "one"))})[1]
        against_one_shot(lib, enc, ec, t, short, alone_short, f"{name} {n_short}")
        both = run_streams(test_lib, st, ec, {0: (long, splits(n_long, hop, "random", seed=6)), 2: (short, splits(n_short, hop, "edges"))})
        assert same_bits(both[0], base) and same_bits(both[2], alone_short)
        swapped = run_streams(test_lib, st, ec, {2: (long, splits(n_long, hop, "edges")), 0: (short, splits(n_short, hop, "random", seed=7))})
        assert same_bits(swapped[2], base) and same_bits(swapped[0], alone_short)
        assert st.device_bytes() == bytes0 and st.state_bytes > 0
    finally:
        st.close()
        enc.close()


def test_full_config_edge_lengths(lib, test_lib, full_synth):
    """The default config on synthetic weights: clips of 1, 1919, 1920, 1921 and 5000 samples as five streams of one object whose
    encoder handle holds clips of 1920 samples at most."""
    ec, t, path = full_synth
    lengths = [1, 1919, 1920, 1921, 5000]
    clips = [C.seeded_clip(11, n) for n in lengths]
    small = Encoder(path, max_batch=len(lengths), max_samples=1920)
    ref = Encoder(path, max_batch=1, max_samples=5000)
    st = small.stream(len(lengths), 1920)
    try:
        with pytest.raises(ValueError):
            small.encode([clips[4]])                      # the whole-clip call refuses what the stream takes
        bytes0 = st.device_bytes()
        a = run_streams(test_lib, st, ec, {k: (c, splits(c.size, 1920, "hop")) for k, c in enumerate(clips)})
        assert st.device_bytes() == bytes0
        b = run_streams(test_lib, st, ec, {len(lengths) - 1 - k: (c, splits(c.size, 1920, "edges")) for k, c in enumerate(clips)})
        for k, c in enumerate(clips):
            assert same_bits(a[k], b[len(lengths) - 1 - k]), f"{c.size} samples: the split or the stream index changes the bits"
            against_one_shot(lib, ref, ec, t, c, a[k], f"full config {c.size}")
        # the product entry point gives the hook's ids
        assert np.array_equal(small.encode_streaming(clips[4], 1900), a[4][0])
        assert st.device_bytes() == bytes0
        print(f"state per stream {st.state_bytes} B, object {bytes0} B, launches of the last push {st.lib.enc_stream_last_launches(st.h)}")
    finally:
        st.close()
        small.close()
        ref.close()


@pytest.mark.parametrize("n_hops, rest", [(0, 1), (0, 5), (1, 3)], ids=["1", "5", "hop+3"])
def test_tiny_clips_a_sample_at_a_time(lib, test_lib, tiny_synth, n_hops, rest):
    """Clips of 1, 5 and hop + 3 samples (shorter than the first conv's 7 taps; one frame and a remainder) pushed a sample at a
    time and finished by an empty push: left of its one new column the first conv of every push reads only the stream's carried
    samples, zeros at the start.  Contracts 1-3: the bits of the whole clip in one push, the hand-out rule after every push
    (run_streams), enc_encode's frames, embedding and ids."""
    ec, t, path = tiny_synth
    hop = W.enc_hop(ec)
    n = n_hops * hop + rest
    clip = C.seeded_clip(31, n)
    enc = Encoder(path, max_batch=1, max_samples=hop + 3)
    st = enc.stream(1, hop + 3)
    try:
        bytes0 = st.device_bytes()
        ones = run_streams(test_lib, st, ec, {0: (clip, splits(n, hop, "ones"))})[0]
        whole = run_streams(test_lib, st, ec, {0: (clip, splits(n, hop, "one"))})[0]
        assert same_bits(ones, whole), f"{n} samples: pushing a sample at a time changes the bits"
        against_one_shot(lib, enc, ec, t, clip, ones, f"tiny config {n}, a sample at a time")
        assert st.device_bytes() == bytes0
    finally:
        st.close()
        enc.close()


def test_every_refused_push_leaves_the_streams_alone(lib, test_lib, tiny_synth):
    ec, t, path = tiny_synth
    hop = W.enc_hop(ec)
    clip = C.seeded_clip(21, 3 * hop + 100)
    enc = Encoder(path, max_batch=2, max_samples=clip.size)
    st = enc.stream(2, hop)
    try:
        want = run_streams(test_lib, st, ec, {0: (clip, splits(clip.size, hop, "hop"))})[0]

        def raw(streams, chunks, fin, cap=None):
            sidx, n_new = np.array(streams, np.int32), np.array([len(c) for c in chunks], np.int32)
            f = np.array(fin, np.int32)
            pcm = np.concatenate([np.asarray(c, np.float32) for c in chunks] + [np.zeros(1, np.float32)])
            codes = np.full((16, 16), -7, np.int64)
            off = np.full(len(streams) + 1, -7, np.int64)
            rc = lib.enc_stream_push(st.h, len(streams), hiplib.iptr(sidx), hiplib.fptr(pcm), hiplib.iptr(n_new), hiplib.iptr(f),
                                     codes.ctypes.data_as(hiplib.i64p), 16 if cap is None else cap, off.ctypes.data_as(hiplib.i64p))
            if rc < 0:
                assert (codes == -7).all() and (off == -7).all()      # nothing is written
            return rc

        def n_new_raw(streams, n_new):     # (lengths the buffer does not back: refused before anything is read)
            sidx, nn = np.array(streams, np.int32), np.array(n_new, np.int32)
            off = np.zeros(len(streams) + 1, np.int64)
            codes = np.zeros((16, 16), np.int64)
            pcm = np.zeros(4, np.float32)
            assert lib.enc_stream_push_max_frames(st.h, len(streams), hiplib.iptr(sidx), hiplib.iptr(nn), None) < 0
            return lib.enc_stream_push(st.h, len(streams), hiplib.iptr(sidx), hiplib.fptr(pcm), hiplib.iptr(nn), None,
                                       codes.ctypes.data_as(hiplib.i64p), 16, off.ctypes.data_as(hiplib.i64p))

        st.reset(0)
        st.reset(1)
        first, second, rest = clip[:hop], clip[hop:2 * hop], clip[2 * hop:]
        got = [st.push([(0, first, False)])[0]]
        assert raw([-1], [second], [0]) < 0 and raw([2], [second], [0]) < 0              # a bad stream index
        assert raw([0, 0], [second, second], [0, 0]) < 0                                # one named twice
        assert n_new_raw([0], [-1]) < 0 and n_new_raw([0], [hop + 1]) < 0               # n_new outside 0..max_push_samples
        for bad in (np.nan, np.inf, -np.inf):                                            # a non-finite sample
            y = second.copy()
            y[hop // 2] = bad
            assert raw([0], [y], [0]) < 0
            assert raw([1, 0], [first, y], [0, 0]) < 0                                   # (the good entry beside it does not run either)
        assert raw([0], [second], [0], cap=0) < 0                                        # capacity below push_max_frames
        assert lib.enc_stream_reset(st.h, 2) < 0 and lib.enc_stream_reset(st.h, -1) < 0
        got.append(st.push([(0, second, False)])[0])
        got.append(st.push([(0, rest[:hop], False)])[0])
        got.append(st.push([(0, rest[hop:], True)])[0])
        assert raw([0], [second], [0]) < 0                                               # a finished stream without a reset
        assert raw([0], [second[:0]], [1]) < 0
        assert np.array_equal(np.concatenate(got), want[0])
        # stream 1 was named in refused pushes only: it is still at its start
        again = run_streams(test_lib, st, ec, {1: (clip, splits(clip.size, hop, "hop"))})[1]
        assert same_bits(again, want)
        # a stream finished with 0 samples gives 0 frames
        st.reset(0)
        assert st.push([(0, clip[:0], True)])[0].shape == (0, 16)
    finally:
        st.close()
        enc.close()


def test_create_refuses_what_it_cannot_carry(lib, tiny_synth, tmp_path):
    ec, t, path = tiny_synth
    assert not lib.enc_stream_create(None, 1, 1920)
    h = lib.enc_load(path.encode(), 1, 1920)
    assert h
    try:
        assert not lib.enc_stream_create(h, 0, 1920) and not lib.enc_stream_create(h, 1, 0)
        s = lib.enc_stream_create(h, 1, 1920)
        assert s
        lib.enc_stream_free(s)
    finally:
        lib.enc_free(h)
    # a window of 300 columns loads, but its 299 carried columns are more than the history kernel holds
    wide = dataclasses.replace(ec, window=300)
    p2 = str(tmp_path / "wide.q3w")
    W.write_synthetic_enc(p2, wide, seed=3)
    h = lib.enc_load(p2.encode(), 1, 1920)
    assert h
    try:
        assert not lib.enc_stream_create(h, 1, 1920)
    finally:
        lib.enc_free(h)
    # a row of unknown kind behind the table: no handle, so no stream
    bad = dict(t)
    bad["enc.program"] = np.concatenate([np.asarray(t["enc.program"]), np.array([[99, 0, 0, 0, 0, 0, 0, 0]], np.int32)])
    p3 = str(tmp_path / "unknown.q3w")
    W.write_pack(p3, {}, bad)
    h = lib.enc_load(p3.encode(), 1, 1920)
    assert not h and not lib.enc_stream_create(h, 1, 1920)


def test_cli_stream_seconds(lib, tiny_synth, tmp_path):
    """--stream_seconds writes the ids of the plain call: the same shape, and a frame parts from the plain call's only at a
    float64 near-tie (tests/test_gpu_encoder.py's rule for a frame that parts from the fixture)."""
    import scipy.io.wavfile as wavfile
    from qwen3_tts_axera_russian_amd import encode_reference_audio as cli
    ec, t, path = tiny_synth
    x = C.seeded_clip(8, 50000)
    wav = tmp_path / "x.wav"
    wavfile.write(str(wav), 24000, (x * 20000).astype(np.int16))
    plain, streamed = tmp_path / "plain.npy", tmp_path / "streamed.npy"
    assert cli.main(["--audio", str(wav), "--model", path, "--output", str(plain)]) == 0
    assert cli.main(["--audio", str(wav), "--model", path, "--output", str(streamed), "--stream_seconds", "0.3"]) == 0
    a, b = np.load(plain), np.load(streamed)
    assert a.dtype == b.dtype == np.int64 and a.shape == b.shape == (W.enc_frames(ec, 50000), 16)
    pcm, _ = cli.load_wav(str(wav))
    enc = Encoder(path, max_batch=1, max_samples=50000)
    try:
        emb = debug_embedding(lib, enc, ec, pcm)[:, :a.shape[0]]
    finally:
        enc.close()
    prog = np.asarray(t["enc.program"])
    proj = np.asarray(t[f"enc.op{len(prog) - 2}.weight"], np.float64)[:, :, 0]
    _, gap, _ = rvq_encode(proj @ emb.astype(np.float64), np.asarray(t[f"enc.op{len(prog) - 1}.codebook"], np.float64), int(prog[-1][6]))
    diff = a != b
    print(f"--stream_seconds: {int(diff.sum())} of {a.size} ids differ from the plain call")
    for f in np.nonzero(diff.any(1))[0]:
        q = int(np.argmax(diff[f]))
        assert gap[f, q] < GAP_TOL, f"frame {f} group {q}: differs and is not a near-tie"
