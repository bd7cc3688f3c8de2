"""Speaker encoder library (spk_* ABI, include/qwen3tts_spk.h) on the GPU, against tests/golden/spk_golden.npz
(float64 torch.stft + the slaney bank; transformers' ECAPA_TimeDelayNet in float64, seeded weights).

Log-mel: |gpu - ref| <= 4e-6 absolute, both cases, every clip length.  Derived: a float64 reordering error of at most
n_fft * 2^-53 * sum |w x| * sqrt(2) / sqrt(mag_eps) ~ 2.6e-6 for |x| <= 1 (the seeded clips stay inside [-1, 1]), plus the one
float32 rounding of values up to 11.6 (9.5e-7).

Every stage and the embedding: 2e-4 of each stage's scale, end to end from the GPU's own log-mel -- the project's bound for
the same exact-f32 kernels (tests/test_gpu_encoder.py).  Then: a ragged batch bit for bit against its clips alone (the 5-
and the 6-frame clip among them), every refusal with the handle still good, and enc_resample_pcm against tests/pcm_ref.py's
pinned samples, against the rows enc_encode_pcm encodes and through enc_encode."""
import json
import os

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.encoder import Encoder
from qwen3_tts_axera_russian_amd.speaker import SpeakerEncoder
from tests import enc_common as EC
from tests import pcm_ref as P
from tests import spk_common as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "spk_golden.npz")
MEL_TOL = 4e-6        # absolute
STAGE_TOL = 2e-4      # of each stage's scale (max |value|)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def handles(gpu_lib, gold, tmp_path_factory):
    """one handle per case for the whole module, sized for all of the case's clips in one call"""
    out, tmp = {}, tmp_path_factory.mktemp("spk")
    for name, case in C.CASES.items():
        assert C.digest(C.state(name)) == bytes(gold[f"{name}.sha"]).decode()
        path = str(tmp / f"spk_{name}.q3w")
        sc = C.write_container(name, path)
        out[name] = (SpeakerEncoder(path, max_batch=len(case["lengths"]), max_samples=max(case["lengths"])), sc)
    yield out
    for spk, _ in out.values():
        spk.close()


@pytest.fixture(scope="module")
def clips():
    return {name: [C.seeded_clip(case["seed"], n) for n in case["lengths"]] for name, case in C.CASES.items()}


def hook(tl, spk, sc, cl, stage):
    """stage None: the log-mel [B][n_mels][L]; else the activation after the stage, [B][C][L] or [B][C] (pooled)"""
    n = np.array([c.size for c in cl], np.int32)
    L = max(W.spk_frames(sc, int(x)) for x in n)
    cm = sc.channels[-1]
    chans = sc.n_mels if stage is None else ([sc.channels[0]] * (len(sc.channels) - 1) + [cm, 2 * cm, sc.dim])[stage]
    pooled = stage is not None and stage >= len(sc.channels)
    out = np.full((len(cl), chans, 1 if pooled else L), np.nan, np.float32)
    Cc, Lc = np.zeros(1, np.int32), np.zeros(1, np.int32)
    pcm = np.concatenate(cl).astype(np.float32)
    if stage is None:
        rc = tl.q3t_spk_mel(spk.h, hiplib.fptr(pcm), hiplib.iptr(n), len(cl), hiplib.fptr(out), hiplib.iptr(Cc), hiplib.iptr(Lc))
    else:
        rc = tl.q3t_spk_stage(spk.h, hiplib.fptr(pcm), hiplib.iptr(n), len(cl), stage, hiplib.fptr(out), hiplib.iptr(Cc), hiplib.iptr(Lc))
    assert rc == 0 and (int(Cc[0]), int(Lc[0])) == out.shape[1:]
    return out[:, :, 0] if pooled else out


@pytest.mark.parametrize("name", list(C.CASES))
def test_log_mel(test_lib, handles, clips, gold, name):
    spk, sc = handles[name]
    for cl in ([c] for c in clips[name]), (clips[name],):           # every clip alone, then all of them as one ragged batch
        for group in cl:
            mel = hook(test_lib, spk, sc, group, None)
            for b, c in enumerate(group):
                assert np.abs(c).max() <= 1.0
                F = W.spk_frames(sc, c.size)
                ref = gold[f"{name}.mel{c.size}"]
                got = mel[b][np.ix_(C.row_subset(sc.n_mels), C.column_subset(F))]
                err = float(np.abs(got.astype(np.float64) - ref).max())
                print(f"{name} mel n={c.size} B={len(group)}: max |gpu - ref| = {err:.2e}, max |ref| = {np.abs(ref).max():.2f}")
                assert err <= MEL_TOL, f"{name} mel {c.size}: {err:.2e}"


@pytest.mark.parametrize("name", list(C.CASES))
def test_stages_and_embedding(test_lib, handles, clips, gold, name):
    spk, sc = handles[name]
    assert len(C.STAGES) == len(sc.channels) + 2
    for si, st in enumerate(C.STAGES):
        a = hook(test_lib, spk, sc, clips[name], si)
        for b, c in enumerate(clips[name]):
            ref, scale = gold[f"{name}.{st}{c.size}"], float(gold[f"{name}.{st}{c.size}.scale"])
            got = a[b][np.ix_(C.row_subset(a.shape[1]), C.column_subset(W.spk_frames(sc, c.size)))] if a.ndim == 3 else a[b]
            err = float(np.abs(got.astype(np.float64) - ref).max()) / max(scale, 1e-3)
            print(f"{name} {st} n={c.size}: {err:.2e} of its scale ({scale:.3g})")
            assert err <= STAGE_TOL, f"{name} stage {st} clip {c.size}: {err:.2e} of its scale"
    emb = spk.embed(clips[name])
    assert emb.shape == (len(clips[name]), sc.dim) == (len(clips[name]), spk.dim)
    assert np.array_equal(emb, hook(test_lib, spk, sc, clips[name], len(C.STAGES) - 1))   # spk_embed is the walk the hooks run


@pytest.mark.parametrize("name", list(C.CASES))
def test_clip_gives_the_same_bits_alone_and_in_any_batch(handles, clips, name):
    spk, sc = handles[name]
    three = clips[name][:3]
    assert [W.spk_frames(sc, c.size) for c in three[:2]] == [5, 6]
    alone = [spk.embed([c])[0] for c in three]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2)):
        got = spk.embed([three[i] for i in order])
        for row, i in zip(got, order):
            assert np.array_equal(row.view(np.uint32), alone[i].view(np.uint32)), (name, order, i)
    assert spk.last_launches() > 0 and spk.last_ms() > 0.0
    assert len({a.tobytes() for a in alone}) == 3


def test_refusals_leave_the_handle_usable(handles, clips, capfd):
    spk, sc = handles["tiny"]
    good = clips["tiny"][2]
    want = spk.embed([good])[0]
    out = np.zeros((4, spk.dim), np.float32)

    def call(cl, B=None):
        n = np.array([c.size for c in cl], np.int32)
        pcm = np.concatenate(cl).astype(np.float32)
        capfd.readouterr()
        rc = spk.lib.spk_embed(spk.h, hiplib.fptr(pcm), hiplib.iptr(n), len(cl) if B is None else B, hiplib.fptr(out))
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[qwen3tts] ")]
        return rc, lines
    nan = good.copy()
    nan[37] = np.nan
    assert spk.min_samples == W.spk_min_samples(sc) == 80 and spk.sample_rate == 24000
    assert spk.frames(sc.pad) < 0 and spk.frames(79) < 0 and spk.frames(80) == 5
    for what, cl, B in (("n <= pad", [good, good[:sc.pad]], None), ("fewer than 5 frames", [good[:79]], None),
                        ("a NaN sample", [good, nan], None), ("B > max_batch", [good] * 4, 4), ("B = 0", [good], 0),
                        ("longer than max_samples", [np.zeros(spk.max_samples + 1, np.float32)], None)):
        rc, lines = call(cl, B)
        assert rc < 0 and len(lines) == 1, (what, rc, lines)
        rc, lines = call([good])
        assert rc == 0 and not lines and np.array_equal(out[0], want), what
    assert spk.lib.spk_embed(spk.h, None, None, 1, hiplib.fptr(out)) < 0
    assert spk.lib.spk_embed(None, None, None, 1, hiplib.fptr(out)) < 0
    assert np.array_equal(spk.embed([good])[0], want)
    with pytest.raises(ValueError):
        spk.embed([good[:10]])


def test_load_refusals(gpu_lib, tmp_path, capfd):
    sc = W.tiny_spk_config()
    st = {"speaker_encoder." + k: v for k, v in W.synthetic_spk_state(sc, 5).items()}
    _, meta, t = W.convert_speaker_encoder(st, sc=sc, verbose=False)
    p = str(tmp_path / "a.q3w")
    for what, m2, t2 in (("no geometry", meta, {k: v for k, v in t.items() if k != "spk.geometry"}),
                         ("a missing weight", meta, {k: v for k, v in t.items() if k != "spk.block2.res1.w"}),
                         ("a misshapen bank", meta, {**t, "spk.mel_fb": t["spk.mel_fb"][:-1]}),
                         ("a non-finite weight", meta, {**t, "spk.fc.b": np.full_like(t["spk.fc.b"], np.inf)}),
                         ("win != n_fft", {**meta, "spk_win": 32}, t)):
        W.write_pack(p, m2, t2)
        assert not gpu_lib.spk_load(p.encode(), 1, 2000), what
        assert "[qwen3tts]" in capfd.readouterr().err, what
    W.write_pack(p, meta, t)
    assert not gpu_lib.spk_load(p.encode(), 1, 79)      # max_samples below the shortest clip
    h = gpu_lib.spk_load(p.encode(), 1, 2000)
    assert h and gpu_lib.spk_dim(h) == 32
    gpu_lib.spk_free(h)


@pytest.fixture(scope="module")
def enc(gpu_lib, tmp_path_factory):
    g = np.load(os.path.join(ROOT, "tests", "golden", "mimi_encode_golden.npz"))
    keys = json.loads(bytes(g["mimi.keys"]).decode())
    state = EC.seeded_state(EC.CASES["mimi"]["seed"], [(k, tuple(s)) for k, s in keys])
    _, t, _ = W.state_to_enc(state, json.loads(bytes(g["mimi.config"]).decode()), 16)
    path = str(tmp_path_factory.mktemp("spk_enc") / "enc_mimi.q3w")
    W.write_pack(path, {"enc_sample_rate": 24000.0}, t)
    e = Encoder(path, max_batch=3, max_samples=6000)
    yield e
    e.close()


@pytest.mark.parametrize("rate,ch,fmt", [(16000, 2, "s16"), (44100, 1, "f32")])
def test_resample_pcm_is_the_front_end_of_encode_pcm(enc, rate, ch, fmt):
    r = np.random.default_rng(rate)
    shape = lambda n: (n, ch) if ch > 1 else (n,)
    mk = (lambda n: r.integers(-32768, 32768, size=shape(n)).astype(np.int16)) if fmt == "s16" else \
         (lambda n: (0.3 * r.standard_normal(shape(n))).astype(np.float32))
    up, down = P.factors(rate)
    cl = [mk(n) for n in (-(-700 * down // up), 7, 1234)]
    got = enc.resample_pcm(cl, rate, ch)
    # the rows the handle encodes (the hook of q3_enc_pcm.hip), bit for bit
    f, n, flat = Encoder._pcm_payload(cl, ch)
    ld = (max(P.out_len(int(x), up, down) for x in n) + 31) // 32 * 32
    rows = np.zeros((len(cl), ld), np.float32)
    n_out, got_ld = np.zeros(len(cl), np.int32), np.zeros(1, np.int32)
    assert enc.lib.enc_debug_pcm(enc.h, flat.ctypes.data, f, ch, rate, hiplib.iptr(n), len(cl), hiplib.fptr(rows), hiplib.iptr(n_out),
                                 hiplib.iptr(got_ld)) == 0
    for b, x in enumerate(cl):
        want = P.prepare(x, rate, ch).astype(np.float32)
        assert got[b].dtype == np.float32 and got[b].size == want.size == int(n_out[b])
        assert np.array_equal(got[b].view(np.uint32), rows[b, :want.size].view(np.uint32)), b
        differ = int((got[b].view(np.uint32) != want.view(np.uint32)).sum())
        print(f"{rate} Hz {fmt} x{ch} clip {b}: {differ} of {want.size} samples differ from pcm_ref's in their bits")
        assert differ == 0
    # enc_encode_pcm is unchanged: its ids are enc_encode's of these samples, and of a clip alone
    ids = enc.encode_pcm(cl, rate, ch)
    for a, b in zip(ids, enc.encode(got)):
        assert np.array_equal(a, b)
    assert np.array_equal(enc.resample_pcm([cl[2]], rate, ch)[0].view(np.uint32), got[2].view(np.uint32))
    # refusals: a clip longer than out holds, a rate outside the front-end's; the handle stays good
    n1 = np.array([cl[0].shape[0]], np.int32)
    small, no = np.zeros((1, 16), np.float32), np.zeros(1, np.int32)
    x0 = np.ascontiguousarray(cl[0]).reshape(-1)
    assert enc.lib.enc_resample_pcm(enc.h, x0.ctypes.data, f, ch, rate, hiplib.iptr(n1), 1, hiplib.fptr(small), 16, hiplib.iptr(no)) < 0
    assert enc.lib.enc_resample_pcm(enc.h, x0.ctypes.data, f, ch, 7999, hiplib.iptr(n1), 1, hiplib.fptr(rows), ld, hiplib.iptr(no)) < 0
    assert np.array_equal(enc.resample_pcm([cl[0]], rate, ch)[0].view(np.uint32), got[0].view(np.uint32))
