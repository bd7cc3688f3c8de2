"""The speaker encoder without a GPU.

1. csrc/q3_spk.h's host arithmetic through tests/spk_host_driver.cpp (built plain and with -fsanitize=address,undefined: a
   stand-alone program, nothing is preloaded): spk_frames = 1 + (n + 2 pad - n_fft) // hop, refused when n <= pad or below
   5 frames; the shortest clip; the reflection index against numpy's reflect padding.
2. The numpy float64 restatement tests/spk_ref.py (log-mel + network) against the committed fixture
   (tests/golden/spk_golden.npz: torch.stft and transformers' ECAPA_TimeDelayNet in float64) within 1e-9 of each stage's scale.
3. The fixture's own float32-forward error (err32) is at most 5e-5 of every stage's scale: a quarter of the GPU bound, so the
   inputs leave the reference itself well inside it.
4. The converter: round trip of a seeded state dict, the packed layout, an unknown key refused.
5. The ABI: the header's names are exported, hiplib declares them.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import weights as W
from tests import spk_common as C
from tests import spk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "spk_golden.npz")
REF_TOL = 1e-9       # numpy float64 vs torch float64, of each stage's scale
ERR32_BOUND = 5e-5   # a quarter of the GPU tests' STAGE_TOL


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("spk_host") / f"spk_host_driver_{request.param}")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "spk_host_driver.cpp"), "-o", exe])
    return exe


def run(driver, *args):
    r = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (args, r.returncode, r.stderr[-2000:])
    out = r.stdout.strip().split()
    return None if out == ["refused"] else out


@pytest.mark.parametrize("name", list(C.CASES))
def test_frames_arithmetic(driver, name):
    sc = C.CASES[name]["sc"]
    g = (sc.n_fft, sc.hop, sc.pad, W.spk_min_frames(sc))
    assert W.spk_min_frames(sc) == 5
    lo = W.spk_min_samples(sc)
    assert run(driver, "min", *g) == ["min", str(lo)]
    for n in (lo, lo + 1, lo + sc.hop - 1, lo + sc.hop, 7 * sc.hop + 3, 24017, 240000) + tuple(C.CASES[name]["lengths"]):
        want = 1 + (n + 2 * sc.pad - sc.n_fft) // sc.hop
        assert run(driver, "frames", *g, n) == ["frames", str(want)], n
        assert W.spk_frames(sc, n) == want
        assert want == 1 + (np.pad(np.zeros(n), sc.pad, mode="reflect").size - sc.n_fft) // sc.hop
    assert run(driver, "frames", *g, lo) == ["frames", "5"]
    for n in (lo - 1, sc.pad + 1, sc.pad, 1, 0, -5):   # fewer than 5 frames, then n <= pad
        assert run(driver, "frames", *g, n) is None, n
        assert W.spk_frames(sc, n) == -1
    assert run(driver, "frames", sc.n_fft, sc.hop, sc.pad, 5, (1 << 40)) is None   # a frame count past 2^31 - 1


def test_reflection_index(driver):
    for L, p in ((5, 4), (6, 4), (9, 2), (100, 3)):
        want = np.pad(np.arange(L), p, mode="reflect")
        assert run(driver, "reflect", L, -p, L - 1 + p) == ["reflect"] + [str(v) for v in want]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(C.CASES))
def test_numpy_reference_matches_the_fixture(gold, name):
    case = C.CASES[name]
    sc, state = case["sc"], C.state(name)
    assert C.digest(state) == bytes(gold[f"{name}.sha"]).decode()
    fb = W.spk_mel_filter_bank(sc)
    for n in case["lengths"]:
        mel = R.log_mel(C.seeded_clip(case["seed"], n), sc, fb)
        assert mel.shape == (sc.n_mels, W.spk_frames(sc, n))
        cols = C.column_subset(mel.shape[1])
        ref = gold[f"{name}.mel{n}"]
        err = np.abs(mel[np.ix_(C.row_subset(sc.n_mels), cols)] - ref).max() / float(gold[f"{name}.mel{n}.scale"])
        assert err <= REF_TOL, f"{name} mel {n}: {err:.2e}"
        st = R.network(mel, state, sc)
        for s in C.STAGES:
            a, ref = st[s], gold[f"{name}.{s}{n}"]
            got = a[np.ix_(C.row_subset(a.shape[0]), cols)] if a.ndim == 2 else a
            err = np.abs(got - ref).max() / float(gold[f"{name}.{s}{n}.scale"])
            assert err <= REF_TOL, f"{name} {s} {n}: {err:.2e}"


@pytest.mark.parametrize("name", list(C.CASES))
def test_float32_forward_is_inside_a_quarter_of_the_gpu_bound(gold, name):
    err = gold[f"{name}.err32"]
    assert err.shape == (len(C.CASES[name]["lengths"]), len(C.STAGES) + 1)
    print(name, "err32 (mel, stages) per clip:\n", err)
    assert err.max() <= ERR32_BOUND, err.max()


def unpack(wp, cout, cin, k):
    mp = (cout + 3) // 4 * 4
    return np.asarray(wp).reshape(cin * k, mp)[:, :cout].T.reshape(cout, cin, k)


@pytest.mark.parametrize("name", list(C.CASES))
def test_converter_round_trip(name, tmp_path):
    case = C.CASES[name]
    state = C.state(name)
    path = str(tmp_path / "spk.q3w")
    sc = C.write_container(name, path)
    meta, t = W.read_pack(path)
    assert W.spk_config_of(meta, t) == sc == case["sc"]
    assert np.array_equal(np.asarray(t["spk.mel_fb"]).view(np.float64), W.spk_mel_filter_bank(sc))
    assert t["spk.mel_fb"].shape == (sc.n_fft // 2 + 1, sc.n_mels)
    C_, cw, cm = sc.channels[0], sc.channels[0] // sc.res2net_scale, sc.channels[-1]
    assert np.array_equal(unpack(t["spk.block0.w"], C_, sc.n_mels, sc.kernel_sizes[0]), state["blocks.0.conv.weight"])
    assert np.array_equal(unpack(t["spk.block2.res1.w"], cw, cw, 3), state["blocks.2.res2net_block.blocks.1.conv.weight"])
    assert np.array_equal(unpack(t["spk.block3.tdnn2.w"], C_, C_, 1), state["blocks.3.tdnn2.conv.weight"])
    assert np.array_equal(t["spk.block1.se1.w"], state["blocks.1.se_block.conv1.weight"][:, :, 0])
    assert np.array_equal(t["spk.block1.se2.b"], state["blocks.1.se_block.conv2.bias"])
    wa = state["asp.tdnn.conv.weight"]
    assert np.array_equal(unpack(t["spk.asp.tdnn.w"], sc.attention_channels, cm, 1), wa[:, :cm])
    assert np.array_equal(t["spk.asp.tdnn.wstat"], wa[:, cm:, 0])
    assert np.array_equal(t["spk.fc.w"], state["fc.weight"][:, :, 0]) and np.array_equal(t["spk.fc.b"], state["fc.bias"])
    assert len(t) == 2 + 2 * (len(state) // 2) + 1   # geometry, bank, a weight and a bias per conv, asp.tdnn's weight split in two
    # the synthetic maker is the same path
    p2 = str(tmp_path / "spk2.q3w")
    assert W.make_synthetic_spk(p2, sc, case["seed"]) == sc
    _, t2 = W.read_pack(p2)
    assert all(np.array_equal(t[k], t2[k]) for k in t)


def test_converter_refusals():
    sc = W.tiny_spk_config()
    state = {"speaker_encoder." + k: v for k, v in W.synthetic_spk_state(sc, 1).items()}
    W.convert_speaker_encoder(state, sc=sc, verbose=False)
    with pytest.raises(KeyError, match="unknown key"):
        W.convert_speaker_encoder({**state, "speaker_encoder.blocks.1.extra.weight": np.zeros(3, np.float32)}, sc=sc, verbose=False)
    short = dict(state)
    del short["speaker_encoder.blocks.2.tdnn2.conv.bias"]
    with pytest.raises(KeyError, match="missing"):
        W.convert_speaker_encoder(short, sc=sc, verbose=False)
    with pytest.raises(KeyError):
        W.convert_speaker_encoder(state, prefix="nothing_here.", sc=sc, verbose=False)
    # keys outside the prefix are someone else's
    W.convert_speaker_encoder({**state, "talker.x": np.zeros(1, np.float32)}, sc=sc, verbose=False)


def test_converter_prints_the_geometry(capsys):
    sc = W.tiny_spk_config()
    W.convert_speaker_encoder({"speaker_encoder." + k: v for k, v in W.synthetic_spk_state(sc, 1).items()}, sc=sc)
    out = capsys.readouterr().out
    assert "channels [32, 32, 32, 32, 96]" in out and "dim 32" in out and "at least 80 samples" in out


def test_header_exports_and_hiplib():
    from qwen3_tts_axera_russian_amd import build, hiplib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qwen3tts_spk.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(spk_[a-z0-9_]+)\s*\(", src)))
    assert names == ["spk_dim", "spk_embed", "spk_frames", "spk_free", "spk_last_launches", "spk_last_ms", "spk_load",
                     "spk_min_samples", "spk_sample_rate"]
    lib = ctypes.CDLL(build.build())
    for n in names + ["enc_resample_pcm", "tfe_build_prefix_spk", "tfe_build_prefix_stream_spk"]:
        assert hasattr(lib, n), n
    assert "q3_spk.hip" in build.SOURCES
    h = hiplib.load()
    assert len(h.spk_embed.argtypes) == 5 and len(h.enc_resample_pcm.argtypes) == 10 and len(h.tfe_build_prefix_spk.argtypes) == 6
    h.spk_frames.restype = ctypes.c_int
    assert h.spk_frames(None, 24000) < 0 and h.spk_dim(None) == 0     # no handle: refused, no device touched
    assert not h.spk_load(str(os.path.join(ROOT, "nope.q3w")).encode(), 1, 24000)
    code = re.sub(r"//.*", "", open(os.path.join(ROOT, "qwen3_tts_axera_russian_amd", "csrc", "q3_spk.h")).read())
    assert "hip" not in code.split("#ifdef __HIPCC__\n#include")[0].lower().replace("__hipcc__", "")   # the host part stands alone
