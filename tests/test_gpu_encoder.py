"""Speech-tokenizer encoder library (enc_* ABI, include/qwen3tts_enc.h) on the GPU.

Golden cases (tests/golden/mimi_encode_golden.npz, transformers' MimiModel.encode on seeded weights): every stage within
2e-4 of the stage's scale.  Codes are graded in the spirit of NEAR_TIE (tests/test_gpu_engine.py): a GPU id must be as
near as the float64 nearest entry within a relative 1e-5 -- distances evaluated in float64 from the GPU's own embedding,
the residual formed from the GPU's own earlier ids -- and the ids that differ from the fixture are counted (0 at these
sizes).  Then: the default config on synthetic weights against tests/enc_ref.py, ragged batches bit for bit against
clips alone, every error path, the frame count, the round trip through the vocoder, the exported symbols.  Last, the
headline invariant across the quantiser's two tile widths (enc_rvq_tile): a clip alone, in a batch and streamed, id for id."""
import dataclasses
import json
import os
import re

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.encoder import Encoder
from tests import enc_common as C
from tests.enc_ref import enc_reference, rvq_encode
from tests.util import CACHE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mimi_encode_golden.npz")
STAGE_TOL = 2e-4      # of each stage's scale (max |value|)
DIST_TOL = 1e-5       # relative: a GPU id's float64 distance over the float64 best


@pytest.fixture(scope="module")
def lib(gpu_lib):
    return gpu_lib


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def golden_table(gold, name, tmp):
    keys = json.loads(bytes(gold[f"{name}.keys"]).decode())
    state = C.seeded_state(C.CASES[name]["seed"], [(k, tuple(s)) for k, s in keys])
    assert C.digest(state) == bytes(gold[f"{name}.sha"]).decode()
    ec, t, _ = W.state_to_enc(state, json.loads(bytes(gold[f"{name}.config"]).decode()), 16)
    path = os.path.join(tmp, f"enc_golden_{name}.q3w")
    W.write_pack(path, {"enc_sample_rate": 24000.0}, t)
    return ec, t, path


@pytest.fixture(scope="module")
def full_synth():
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, "enc_full_s7.q3w")
    ec = W.EncConfig()
    if not os.path.exists(path):
        W.write_synthetic_enc(path, ec, seed=7)
    _, t = W.read_pack(path)
    return ec, {k: np.asarray(v) for k, v in t.items()}, path


def debug_run(lib, h, clips, n_ops):
    """the activation after n_ops ops for a batch of clips -> [B][C][L] (L = the longest clip's columns)"""
    n = np.array([c.size for c in clips], np.int32)
    Cc, L = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert lib.enc_debug_shape(h, hiplib.iptr(n), len(clips), n_ops, hiplib.iptr(Cc), hiplib.iptr(L)) == 0
    out = np.empty((len(clips), int(Cc[0]), int(L[0])), np.float32)
    C2, L2 = np.zeros(1, np.int32), np.zeros(1, np.int32)
    pcm = np.concatenate(clips).astype(np.float32)
    assert lib.enc_debug_run(h, hiplib.fptr(pcm), hiplib.iptr(n), len(clips), n_ops, hiplib.fptr(out), hiplib.iptr(C2),
                             hiplib.iptr(L2)) == 0
    assert (C2[0], L2[0]) == (Cc[0], L[0])
    return out


def grade(t, emb, codes):
    """float64 grading of GPU ids from the GPU's own embedding [hidden][frames] -> worst distance ratio"""
    prog = np.asarray(t["enc.program"])
    proj = np.asarray(t[f"enc.op{len(prog) - 2}.weight"], np.float64)[:, :, 0]
    books = np.asarray(t[f"enc.op{len(prog) - 1}.codebook"], np.float64)
    _, _, ratio = rvq_encode(proj @ emb.astype(np.float64), books, int(prog[-1][6]), forced=codes)
    return float(ratio.max())


@pytest.mark.parametrize("name", list(C.CASES))
def test_golden_stages(lib, gold, name, tmp_path):
    case = C.CASES[name]
    ec, t, path = golden_table(gold, name, str(tmp_path))
    n = case["lengths"][case["stage_clip"]]
    enc = Encoder(path, max_batch=2, max_samples=max(case["lengths"]))
    try:
        clip = C.seeded_clip(case["seed"], n)
        for st, n_ops in W.enc_program(ec)[2]:
            a = debug_run(lib, enc.h, [clip], n_ops)[0]
            ref = gold[f"{name}.{st}"]
            got = a[:, gold[f"{name}.{st}.cols"]]
            err = float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-3)
            assert err <= STAGE_TOL, f"{name} stage {st}: {err:.2e} of its scale"
    finally:
        enc.close()


@pytest.mark.parametrize("name", list(C.CASES))
def test_golden_codes(lib, gold, name, tmp_path):
    case = C.CASES[name]
    ec, t, path = golden_table(gold, name, str(tmp_path))
    lengths = case["lengths"]
    enc = Encoder(path, max_batch=len(lengths), max_samples=max(lengths))
    try:
        clips = [C.seeded_clip(case["seed"], n) for n in lengths]
        codes = enc.encode(clips)
        emb_ops = dict(W.enc_program(ec)[2])["embedding"]
        embs = debug_run(lib, enc.h, clips, emb_ops)
        differ = total = 0
        for b, n in enumerate(lengths):
            want = gold[f"{name}.codes{n}"]
            assert codes[b].shape == want.shape
            ratio = grade(t, embs[b][:, :want.shape[0]], codes[b])
            assert ratio <= 1 + DIST_TOL, f"{name} n={n}: a GPU id is {ratio - 1:.2e} farther than the float64 best"
            diff = codes[b] != want
            differ += int(diff.sum())
            total += want.size
            for f in np.nonzero(diff.any(1))[0]:   # a frame may part from the fixture only at a float64 near-tie
                q = int(np.argmax(diff[f]))
                assert gold[f"{name}.gap{n}"][f, q] < 1e-4, f"{name} n={n} frame {f} group {q}: not a near-tie"
        print(f"{name}: {differ} of {total} ids differ from the fixture")
    finally:
        enc.close()


def test_full_config_synthetic(lib, full_synth):
    """The default config (MimiConfig() with 16 quantizers) on synthetic weights, a 4 s clip, against enc_ref."""
    ec, t, path = full_synth
    enc = Encoder(path, max_batch=1, max_samples=96000)
    try:
        clip = C.seeded_clip(9, 96000)
        codes = enc.encode([clip])[0]
        stages = dict(W.enc_program(ec)[2])
        emb = debug_run(lib, enc.h, [clip], stages["embedding"])[0]
        _, got = enc_reference(t, clip, len(W.enc_program(ec)[0]) - 1, stages={"embedding": stages["embedding"]})
        ref = got["embedding"]
        assert np.abs(emb - ref).max() <= STAGE_TOL * np.abs(ref).max()
        ref_codes, _ = enc_reference(t, clip)
        assert codes.shape == ref_codes.shape == (50, 16)
        assert grade(t, emb, codes) <= 1 + DIST_TOL
        distinct = [len(set(codes[:, g])) for g in range(16)]
        print("ids differing from enc_ref:", int((codes != ref_codes).sum()), "of", codes.size, "; distinct per group", distinct)
        assert min(distinct) >= 10, distinct     # not degenerate
        assert (codes >= 0).all() and (codes < ec.codebook_size).all()
    finally:
        enc.close()


def test_ragged_batch_same_bits(lib, full_synth):
    ec, t, path = full_synth
    lengths = [1, 1919, 1920, 1921, 2000, 240000]
    enc = Encoder(path, max_batch=len(lengths), max_samples=240000)
    try:
        clips = [C.seeded_clip(11, n) for n in lengths]
        batch = enc.encode(clips)
        again = enc.encode(clips)
        emb_ops = dict(W.enc_program(ec)[2])["embedding"]
        embs = debug_run(lib, enc.h, clips, emb_ops)
        for b, c in enumerate(clips):
            alone = enc.encode([c])[0]
            assert alone.shape == (W.enc_frames(ec, c.size), 16)
            assert np.array_equal(batch[b], alone), f"clip {b} ({c.size} samples) differs inside the batch"
            assert np.array_equal(again[b], batch[b])
            e1 = debug_run(lib, enc.h, [c], emb_ops)[0]
            assert np.array_equal(embs[b][:, :e1.shape[1]].view(np.uint32), e1.view(np.uint32))
        # batch order does not matter either
        rev = enc.encode(clips[::-1])[::-1]
        assert all(np.array_equal(a, b) for a, b in zip(rev, batch))
    finally:
        enc.close()


def test_error_paths(lib, full_synth, tmp_path):
    ec, t, path = full_synth
    h = lib.enc_load(path.encode(), 2, 48000)
    assert h
    try:
        def call(pcm, n, B, max_frames, handle=h, codes=True, nf=True):
            n = np.asarray(n, np.int32)
            out = np.zeros((max(B, 1), max(max_frames, 1), 16), np.int64)
            nfr = np.zeros(max(B, 1), np.int32)
            return lib.enc_encode(handle, hiplib.fptr(pcm) if pcm is not None else None, hiplib.iptr(n) if n.size else None, B,
                                  out.ctypes.data_as(hiplib.i64p) if codes else None, max_frames,
                                  hiplib.iptr(nfr) if nf else None)
        x = C.seeded_clip(3, 4000)
        assert call(x, [4000], 1, 3) == 0
        assert call(x, [4000], 1, 3, handle=None) < 0                    # NULL handle
        assert call(None, [4000], 1, 3) < 0                              # NULL pcm
        assert call(x, [4000], 1, 3, codes=False) < 0                    # NULL codes_out
        assert call(x, [4000], 1, 3, nf=False) < 0                       # NULL n_frames
        assert call(np.concatenate([x, x, x]), [4000] * 3, 3, 3) < 0     # B > max_batch
        assert call(x, [4000], 0, 3) < 0                                 # B = 0
        assert call(x, [0], 1, 3) < 0                                    # empty clip
        assert call(x, [-5], 1, 3) < 0
        big = np.zeros(48001, np.float32)
        assert call(big, [48001], 1, 26) < 0                             # longer than max_samples
        assert call(x, [4000], 1, 2) < 0                                 # max_frames too small (4000 -> 3 frames)
        for bad in (np.nan, np.inf, -np.inf):
            y = x.copy()
            y[1234] = bad
            assert call(y, [4000], 1, 3) < 0                             # non-finite sample
        assert call(x, [4000], 1, 3) == 0                                # the handle still works
        assert lib.enc_frames(None, 100) < 0 and lib.enc_frames(h, 0) < 0
    finally:
        lib.enc_free(h)
    assert not lib.enc_load(str(tmp_path / "missing.q3w").encode(), 1, 1000)
    assert not lib.enc_load(path.encode(), 0, 1000) and not lib.enc_load(path.encode(), 1, 0)
    # malformed tables: not an encoder container; an op whose channels do not chain; no quantiser at the end
    voc = str(tmp_path / "voc.q3w")
    W.write_pack(voc, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=1))
    assert not lib.enc_load(voc.encode(), 1, 1000)
    tt = W.make_synthetic_enc(W.tiny_enc_config(), seed=1)
    bad = dict(tt)
    prog = np.array(bad["enc.program"])
    prog[1][1] += 8
    bad["enc.program"] = prog
    W.write_pack(str(tmp_path / "bad1.q3w"), {}, bad)
    assert not lib.enc_load(str(tmp_path / "bad1.q3w").encode(), 1, 1000)
    bad = {k: v for k, v in tt.items() if not k.startswith(f"enc.op{len(tt['enc.program']) - 1}.")}
    bad["enc.program"] = np.array(tt["enc.program"])[:-1]
    W.write_pack(str(tmp_path / "bad2.q3w"), {}, bad)
    assert not lib.enc_load(str(tmp_path / "bad2.q3w").encode(), 1, 1000)


def test_frames_agree(lib, full_synth, gold, tmp_path):
    ec, t, path = full_synth
    enc = Encoder(path, max_batch=1, max_samples=24000)
    try:
        assert (enc.n_q, enc.sample_rate, enc.samples_per_frame) == (16, 24000, 1920)
        for n in list(range(1, 5000, 37)) + [1919, 1920, 1921, 3840, 3841, 240000, 240001, 10 ** 7]:
            assert enc.frames(n) == W.enc_frames(ec, n)
    finally:
        enc.close()
    ec2, _, p2 = golden_table(gold, "other", str(tmp_path))
    enc = Encoder(p2, max_batch=1, max_samples=100)
    try:
        assert enc.samples_per_frame == W.enc_hop(ec2) == 48
        for n in range(1, 500, 7):
            assert enc.frames(n) == W.enc_frames(ec2, n)
    finally:
        enc.close()


def test_round_trip_through_vocoder(lib, full_synth):
    """enc_encode -> voc_synthesize: the ids are in the vocoder's range and the waveform has the length the frames give,
    within what voc_synthesize_max_samples allows."""
    ec, t, path = full_synth
    vpath = os.path.join(CACHE, "voc_tiny_s7_enc.q3w")
    if not os.path.exists(vpath):
        W.write_pack(vpath, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    enc = Encoder(path, max_batch=2, max_samples=72000)
    vh = lib.voc_load(vpath.encode(), 64, 1)
    assert vh
    try:
        for n in (72000, 30000):
            codes = enc.encode([C.seeded_clip(5, n)])[0]
            T = codes.shape[0]
            assert T == W.enc_frames(ec, n)
            cap = lib.voc_synthesize_max_samples(vh, T)
            out = np.zeros(cap, np.int16)
            ns = np.zeros(1, np.int32)
            assert lib.voc_synthesize(vh, np.ascontiguousarray(codes).ctypes.data_as(hiplib.i64p), T,
                                      out.ctypes.data_as(hiplib.i16p), ns.ctypes.data_as(hiplib.i32p)) == 0
            spt = lib.voc_samples_per_token(vh)
            assert (T - 1) * spt < int(ns[0]) <= min(cap, T * spt)
            assert np.abs(out[:int(ns[0])].astype(np.int32)).max() > 0
    finally:
        lib.voc_free(vh)
        enc.close()


def test_header_symbols_exported(lib):
    src = open(os.path.join(ROOT, "include", "qwen3tts_enc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(enc_[a-z0-9_]+)\s*\(", src)))
    assert names == ["enc_encode", "enc_frames", "enc_free", "enc_last_ms", "enc_load", "enc_num_quantizers",
                     "enc_sample_rate", "enc_samples_per_frame"], names
    assert not [n for n in names if not hasattr(lib, n)]


def test_cli_prompt_dir_decodes(lib, full_synth, tmp_path):
    """encode_reference_audio --audio x.wav --output_dir d writes a prompt_dir whose ids voc_synthesize decodes
    (--decode_back: the reference script's decode-back step)."""
    import scipy.io.wavfile as wavfile
    from qwen3_tts_axera_russian_amd import encode_reference_audio as cli
    ec, t, path = full_synth
    vpath = os.path.join(CACHE, "voc_tiny_s7_enc.q3w")
    if not os.path.exists(vpath):
        W.write_pack(vpath, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    wav = tmp_path / "x.wav"
    wavfile.write(str(wav), 16000, (C.seeded_clip(8, 40000)[:32000] * 20000).astype(np.int16))   # 2 s at 16 kHz
    d = tmp_path / "prompt"
    out = tmp_path / "back.wav"
    assert cli.main(["--audio", str(wav), "--model", path, "--output_dir", str(d), "--ref_text", "тест",
                     "--decode_back", str(out), "--vocoder", vpath]) == 0
    codes = np.load(d / "ref_codec_tokens.npy")
    assert codes.dtype == np.int64 and codes.shape == (W.enc_frames(ec, 48000), 16)
    assert (d / "ref_text.txt").read_text() == "тест"
    sr, back = wavfile.read(str(out))
    assert sr == 24000 and back.dtype == np.int16 and (codes.shape[0] - 1) * 1920 < back.size <= codes.shape[0] * 1920


# ---- clip b gives the same ids alone, in a batch and in any split -- across the quantiser's two kernels ----
@pytest.fixture(scope="module")
def short_stride_synth(tmp_path_factory):
    """the tiny table with short strides, 8 samples per frame: thousands of frames from a few thousand samples"""
    ec = dataclasses.replace(W.tiny_enc_config(), ratios=(2, 2))
    assert W.enc_hop(ec) == 8
    path = str(tmp_path_factory.mktemp("encq") / "enc_tiny_hop8.q3w")
    W.write_synthetic_enc(path, ec, seed=5)
    return ec, path


def test_batch_and_alone_across_the_tile_widths(lib, test_lib, short_stride_synth):
    """8 ragged clips of about 300 frames: each alone is quantised by the 4-frame kernel, the batch (B * longest = 2488
    frames) by the 16-frame one.  encode(batch)[b] == encode([clip b])[0], id for id."""
    ec, path = short_stride_synth
    lengths = [2400, 2393, 2401, 2312, 2488, 2250, 2399, 2456]
    frames = [W.enc_frames(ec, n) for n in lengths]
    assert all(test_lib.q3t_enc_rvq_tile(f) == 4 for f in frames)
    assert test_lib.q3t_enc_rvq_tile(len(lengths) * max(frames)) == 16
    enc = Encoder(path, max_batch=len(lengths), max_samples=max(lengths))
    try:
        clips = [C.seeded_clip(21, n) for n in lengths]
        batch = enc.encode(clips)
        for b, c in enumerate(clips):
            alone = enc.encode([c])[0]
            assert alone.shape == (frames[b], 16)
            assert np.array_equal(batch[b], alone), f"clip {b}: {int((batch[b] != alone).sum())} ids differ inside the batch"
        assert len({tuple(r) for r in np.concatenate(batch).tolist()}) > 500      # not degenerate
    finally:
        enc.close()


def test_long_clip_and_its_stream_across_the_tile_widths(lib, test_lib, short_stride_synth):
    """One clip of 2100 frames at once (the 16-frame kernel) against the same clip through EncoderStream in pushes of 500
    frames (the 4-frame kernel), id for id."""
    ec, path = short_stride_synth
    n, push = 16795, 4000
    assert W.enc_frames(ec, n) == 2100 and test_lib.q3t_enc_rvq_tile(2100) == 16
    assert test_lib.q3t_enc_rvq_tile(W.enc_frames(ec, push)) == 4
    enc = Encoder(path, max_batch=1, max_samples=n)
    try:
        clip = C.seeded_clip(22, n)
        whole = enc.encode([clip])[0]
        streamed = enc.encode_streaming(clip, push_samples=push)
        assert whole.shape == streamed.shape == (2100, 16)
        diff = np.argwhere(whole != streamed)
        assert diff.size == 0, f"{len(diff)} ids differ between the clip at once and its stream, first (frame, group) {diff[0].tolist()}"
    finally:
        enc.close()
