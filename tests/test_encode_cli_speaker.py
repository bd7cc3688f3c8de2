"""encode_reference_audio --speaker_model with stub encoders (no GPU): ref_spk_embedding.npy (float32 [dim]) is written next
to ref_codec_tokens.npy, from the SAME 24 kHz samples the ids come from -- the host-resampled ones, or the device front-end's
(Encoder.resample_pcm) -- under every --resample / --stream_seconds / --push_seconds mode; without the flag nothing new is
written; a clip the speaker encoder refuses is an error.  CPU only."""
import os

import numpy as np
import scipy.io.wavfile as wavfile

from qwen3_tts_axera_russian_amd import encode_reference_audio as cli

CODES = (np.arange(3)[:, None] * 16 + np.arange(16)[None, :]).astype(np.int64)


class StubEnc:
    sample_rate = 24000

    def __init__(self):
        self.calls = []

    def encode(self, clips):
        self.calls.append("encode")
        self.samples = np.asarray(clips[0])
        return [CODES]

    def encode_streaming(self, x, push):
        self.calls.append("encode_streaming")
        self.samples = np.asarray(x)
        return CODES

    def encode_pcm(self, clips, rate, channels=1):
        self.calls.append("encode_pcm")
        return [CODES]

    def encode_streaming_pcm(self, x, rate, channels=1, push_frames=None, max_push_samples=0):
        self.calls.append("encode_streaming_pcm")
        return CODES

    def resample_pcm(self, clips, rate, channels=1):
        """a recognisable stand-in for the front-end's samples: the first channel, every (rate / 8000)-th frame, / 32768"""
        self.calls.append("resample_pcm")
        x = np.asarray(clips[0]).reshape(len(clips[0]), -1)[:, 0]
        self.samples = (x[::rate // 8000].astype(np.float32) / 32768.0)
        return [self.samples]

    def last_ms(self):
        return 0.0


class StubSpk:
    sample_rate, min_samples, dim = 24000, 1280, 8

    def __init__(self, log, sized):
        self.log = log
        sized.append(self)

    def embed(self, clips):
        self.log.append(np.asarray(clips[0]).copy())
        c = np.asarray(clips[0], np.float64)
        return np.array([[c.size, c.sum(), c[0], c[-1], 1, 2, 3, 4]], np.float32)

    def last_ms(self):
        return 0.0

    def last_launches(self):
        return 0

    def close(self):
        self.closed = True


def run(tmp_path, data, sr, extra, out_dir=True):
    wav = tmp_path / "in.wav"
    wavfile.write(str(wav), sr, data)
    enc, log, made = StubEnc(), [], []
    dst = ["--output_dir", str(tmp_path / "p")] if out_dir else ["--output", str(tmp_path / "o" / "codes.npy")]
    if not out_dir:
        os.makedirs(tmp_path / "o")
    rc = cli.main(["--audio", str(wav), "--model", "x.q3w"] + dst + list(extra), encoder_factory=lambda m, n: enc,
                  speaker_factory=lambda m, n: StubSpk(log, made) if m == "spk.q3w" else None)
    return rc, enc, log, made


X16 = np.random.default_rng(4).integers(-20000, 20000, size=(16000, 2)).astype(np.int16)


def check(tmp_path, log, made, samples):
    emb = np.load(tmp_path / "p" / "ref_spk_embedding.npy")
    assert emb.dtype == np.float32 and emb.shape == (8,)
    assert len(log) == 1 and log[0].dtype == np.float32 and np.array_equal(log[0], samples)
    assert emb[0] == samples.size and made[0].closed
    assert np.array_equal(np.load(tmp_path / "p" / "ref_codec_tokens.npy"), CODES)


def test_host_path_embeds_the_samples_the_encoder_got(tmp_path):
    rc, enc, log, made = run(tmp_path, X16, 16000, ["--speaker_model", "spk.q3w"])
    assert rc == 0 and enc.calls == ["encode"] and enc.samples.size == 24000
    check(tmp_path, log, made, enc.samples)


def test_host_streamed(tmp_path):
    rc, enc, log, made = run(tmp_path, X16, 16000, ["--speaker_model", "spk.q3w", "--stream_seconds", "0.25"])
    assert rc == 0 and enc.calls == ["encode_streaming"]
    check(tmp_path, log, made, enc.samples)


def test_device_path_embeds_the_front_ends_samples(tmp_path):
    rc, enc, log, made = run(tmp_path, X16, 16000, ["--speaker_model", "spk.q3w", "--resample", "device"])
    assert rc == 0 and enc.calls == ["encode_pcm", "resample_pcm"]
    check(tmp_path, log, made, enc.samples)


def test_device_pushes(tmp_path):
    rc, enc, log, made = run(tmp_path, X16, 16000, ["--speaker_model", "spk.q3w", "--resample", "device", "--push_seconds", "0.3"])
    assert rc == 0 and enc.calls == ["encode_streaming_pcm", "resample_pcm"]
    check(tmp_path, log, made, enc.samples)


def test_next_to_a_plain_output_file(tmp_path):
    rc, enc, log, made = run(tmp_path, X16, 16000, ["--speaker_model", "spk.q3w"], out_dir=False)
    assert rc == 0 and sorted(os.listdir(tmp_path / "o")) == ["codes.npy", "ref_spk_embedding.npy"]


def test_without_the_flag_nothing_changes(tmp_path):
    rc, enc, log, made = run(tmp_path, X16, 16000, [])
    assert rc == 0 and not log and not made and sorted(os.listdir(tmp_path / "p")) == ["ref_codec_tokens.npy"]


def test_a_clip_too_short_for_the_speaker_encoder(tmp_path, capsys):
    rc, enc, log, made = run(tmp_path, X16[:500], 16000, ["--speaker_model", "spk.q3w"])
    assert rc == 2 and not log and "needs 1280" in capsys.readouterr().err and made[0].closed
    assert not os.path.exists(tmp_path / "p" / "ref_spk_embedding.npy")
