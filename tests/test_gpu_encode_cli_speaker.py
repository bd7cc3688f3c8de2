"""encode_reference_audio --speaker_model on the GPU, with the tiny encoder table of tests/enc_common.py and the tiny speaker
encoder of tests/spk_common.py: under every --resample / --stream_seconds / --push_seconds mode ref_spk_embedding.npy is, bit
for bit, SpeakerEncoder.embed of the 24 kHz samples the ids come from -- the host-resampled ones, or the device front-end's --
and ref_codec_tokens.npy is what the run without the flag writes."""
import json
import os

import numpy as np
import pytest
import scipy.io.wavfile as wavfile

from qwen3_tts_axera_russian_amd import encode_reference_audio as cli
from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.encoder import Encoder
from qwen3_tts_axera_russian_amd.speaker import SpeakerEncoder
from tests import enc_common as C
from tests import spk_common as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = np.stack([C.seeded_clip(51, 8000) * 20000, C.seeded_clip(52, 8000) * 9000], 1).astype(np.int16)      # 0.5 s, 16 kHz stereo


@pytest.fixture(scope="module")
def world(gpu_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_spk")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "mimi_encode_golden.npz"))
    keys = json.loads(bytes(gold["mimi.keys"]).decode())
    state = C.seeded_state(C.CASES["mimi"]["seed"], [(k, tuple(s)) for k, s in keys])
    _, t, _ = W.state_to_enc(state, json.loads(bytes(gold["mimi.config"]).decode()), 16)
    W.write_pack(str(d / "enc.q3w"), {"enc_sample_rate": 24000.0}, t)
    S.write_container("tiny", str(d / "spk.q3w"))
    wavfile.write(str(d / "in.wav"), 16000, X)
    enc, spk = Encoder(str(d / "enc.q3w"), max_batch=1, max_samples=12000), SpeakerEncoder(str(d / "spk.q3w"), 1, 12000)
    host = cli.resample(cli.load_wav(str(d / "in.wav"))[0], 16000, 24000)
    dev = enc.resample_pcm([X], 16000, channels=2)[0]
    want = {"host": spk.embed([host])[0], "device": spk.embed([dev])[0]}
    enc.close()
    spk.close()
    assert host.size == dev.size == 12000 and not np.array_equal(want["host"], want["device"])      # two resamplers, two embeddings
    return d, want


@pytest.mark.parametrize("mode,extra", [("host", []), ("host", ["--stream_seconds", "0.2"]), ("device", ["--resample", "device"]),
                                        ("device", ["--resample", "device", "--push_seconds", "0.15"])])
def test_the_embedding_of_the_samples_the_ids_come_from(world, mode, extra, tmp_path):
    d, want = world
    base = ["--audio", str(d / "in.wav"), "--model", str(d / "enc.q3w")] + extra
    assert cli.main(base + ["--output_dir", str(tmp_path / "with"), "--speaker_model", str(d / "spk.q3w")]) == 0
    assert cli.main(base + ["--output_dir", str(tmp_path / "without")]) == 0
    emb = np.load(tmp_path / "with" / "ref_spk_embedding.npy")
    assert emb.dtype == np.float32 and emb.shape == (32,)
    assert np.array_equal(emb.view(np.uint32), want[mode].view(np.uint32))
    assert sorted(os.listdir(tmp_path / "without")) == ["ref_codec_tokens.npy"]
    assert np.array_equal(np.load(tmp_path / "with" / "ref_codec_tokens.npy"), np.load(tmp_path / "without" / "ref_codec_tokens.npy"))


def test_a_clip_the_speaker_encoder_refuses(world, tmp_path, capsys):
    d, _ = world
    wavfile.write(str(tmp_path / "short.wav"), 24000, X[:60, 0])
    rc = cli.main(["--audio", str(tmp_path / "short.wav"), "--model", str(d / "enc.q3w"), "--output_dir", str(tmp_path / "o"),
                   "--speaker_model", str(d / "spk.q3w")])
    assert rc == 2 and "needs 80" in capsys.readouterr().err and not os.path.exists(tmp_path / "o" / "ref_spk_embedding.npy")
