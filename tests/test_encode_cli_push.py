"""encode_reference_audio --resample device --push_seconds with a stub encoder (no GPU): the file's own frames reach
Encoder.encode_streaming_pcm as the file holds them, in pushes of round(S * the file's rate) frames, on a handle sized for
one push whatever the file's length; --push_seconds without --resample device and --stream_seconds with it are refused, and
the refusal of the latter names --push_seconds.  CPU only."""
import numpy as np
import pytest
import scipy.io.wavfile as wavfile

from qwen3_tts_axera_russian_amd import encode_reference_audio as cli


class Stub:
    sample_rate = 24000

    def __init__(self):
        self.calls = []

    def encode_streaming_pcm(self, x, rate, channels=1, push_frames=None, max_push_samples=24000):
        self.calls.append((x, rate, channels, push_frames, max_push_samples))
        return np.zeros((7, 16), np.int64)


def run(tmp_path, data, sr, extra):
    wav = tmp_path / "in.wav"
    wavfile.write(str(wav), sr, data)
    stub, sized = Stub(), []

    def factory(model, n):
        sized.append(n)
        return stub
    rc = cli.main(["--audio", str(wav), "--model", "x.q3w", "--output", str(tmp_path / "out.npy")] + list(extra), encoder_factory=factory)
    return rc, stub, sized


def test_the_files_frames_in_pushes(tmp_path):
    x = np.random.default_rng(1).integers(-32768, 32768, size=(100000, 2)).astype(np.int16)
    rc, stub, sized = run(tmp_path, x, 44100, ("--resample", "device", "--push_seconds", "0.3"))
    assert rc == 0 and len(stub.calls) == 1
    got, rate, ch, push, room = stub.calls[0]
    assert got.dtype == np.int16 and np.array_equal(got, x) and (rate, ch, push) == (44100, 2, 13230)
    # one push's samples and the filter's tail fit, and the handle is sized for that, not for the file
    assert room == sized[0] == -(-13230 * 24000 // 44100) + 32 < 100000 * 24000 // 44100
    assert np.load(tmp_path / "out.npy").shape == (7, 16)


def test_refusals(tmp_path, capsys):
    x = np.zeros(1000, np.int16)
    for extra, word in ((("--push_seconds", "0.3"), "--resample device"),
                        (("--resample", "device", "--stream_seconds", "1"), "--push_seconds"),
                        (("--resample", "device", "--push_seconds", "0"), "> 0")):
        with pytest.raises(SystemExit):
            run(tmp_path, x, 16000, extra)
        assert word in capsys.readouterr().err, extra
