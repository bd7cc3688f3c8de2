"""encode_reference_audio --resample device with a stub encoder (no GPU): the file's samples reach Encoder.encode_pcm as the
file holds them (int16 / float32, channels interleaved, the file's rate), the handle is sized for the 24 kHz length, the
output is saved as on the host path, and what the device path does not take is an error.  --resample host stays the
default.  CPU only."""
import numpy as np
import scipy.io.wavfile as wavfile

from qwen3_tts_axera_russian_amd import encode_reference_audio as cli
from qwen3_tts_axera_russian_amd.encoder import Encoder


class Stub:
    sample_rate = 24000

    def __init__(self):
        self.pcm, self.host, self.sized = [], [], []

    def encode_pcm(self, clips, rate, channels=1):
        fmt, n, flat = Encoder._pcm_payload(clips, channels)      # (the real argument checks)
        self.pcm.append((clips[0], rate, channels))
        T = -(-(-(-int(n[0]) * 24000 // rate)) // 1920)
        return [(np.arange(T)[:, None] * 16 + np.arange(16)[None, :]).astype(np.int64)]

    def encode(self, clips):
        self.host += list(clips)
        return [np.zeros((1, 16), np.int64)]

    def last_ms(self):
        return 0.0


def run(tmp_path, data, sr, extra=("--resample", "device")):
    wav = tmp_path / "in.wav"
    wavfile.write(str(wav), sr, data)
    stub = Stub()

    def factory(model, n):
        stub.sized.append(n)
        return stub
    rc = cli.main(["--audio", str(wav), "--model", "x.q3w", "--output", str(tmp_path / "out.npy")] + list(extra), encoder_factory=factory)
    return rc, stub


def test_stereo_int16_goes_as_it_is(tmp_path):
    x = np.random.default_rng(1).integers(-32768, 32768, size=(16000, 2)).astype(np.int16)
    rc, stub = run(tmp_path, x, 16000)
    assert rc == 0 and not stub.host and stub.sized == [24000]
    got, rate, ch = stub.pcm[0]
    assert got.dtype == np.int16 and np.array_equal(got, x) and (rate, ch) == (16000, 2)
    assert np.load(tmp_path / "out.npy").shape == (13, 16)


def test_mono_float32_and_truncation(tmp_path):
    x = np.linspace(-1, 1, 44100).astype(np.float32)
    rc, stub = run(tmp_path, x, 44100, extra=("--resample", "device", "--max_tokens", "5"))
    got, rate, ch = stub.pcm[0]
    assert rc == 0 and got.dtype == np.float32 and np.array_equal(got, x) and (rate, ch) == (44100, 1) and stub.sized == [24000]
    assert np.load(tmp_path / "out.npy").shape == (5, 16)


def test_what_the_device_path_does_not_take(tmp_path, capsys):
    rc, stub = run(tmp_path, np.zeros(1000, np.int32), 16000)
    assert rc != 0 and not stub.pcm and "--resample host" in capsys.readouterr().err
    wav = tmp_path / "in.wav"
    wavfile.write(str(wav), 16000, np.zeros(100, np.int16))
    try:
        cli.main(["--audio", str(wav), "--model", "x.q3w", "--resample", "device", "--stream_seconds", "1"], encoder_factory=lambda m, n: Stub())
        assert False, "--stream_seconds with --resample device must be refused"
    except SystemExit:
        pass


def test_host_stays_the_default(tmp_path):
    x = (0.1 * np.ones(16000)).astype(np.float32)
    rc, stub = run(tmp_path, x, 16000, extra=())
    assert rc == 0 and not stub.pcm and stub.host[0].size == 24000 and stub.host[0].dtype == np.float32
    assert np.array_equal(stub.host[0], cli.resample(x, 16000, 24000))
