"""python -m qwen3_tts_axera_russian_amd.encode_reference_audio with a stub encoder (no GPU): the reference's WAV rules
(int16 / 32768, int32 / 2^31, other dtypes cast unscaled, channels averaged), resampling to 24 kHz, the output layout
and truncation, the prompt_dir files, the error for an unreadable file.  CPU only."""
import numpy as np
import pytest
import scipy.io.wavfile as wavfile

from qwen3_tts_axera_russian_amd import encode_reference_audio as cli


class StubEncoder:
    """Encoder's interface: ids [ceil(n / 1920)][16] with id = frame * 16 + group; remembers what it was given."""
    sample_rate = 24000

    def __init__(self):
        self.got = []

    def encode(self, clips):
        self.got += [np.asarray(c) for c in clips]
        out = []
        for c in clips:
            T = -(-c.size // 1920)
            out.append((np.arange(T)[:, None] * 16 + np.arange(16)[None, :]).astype(np.int64))
        return out

    def last_ms(self):
        return 0.0


def run(tmp_path, data, sr=24000, extra=()):
    wav = tmp_path / "in.wav"
    wavfile.write(str(wav), sr, data)
    stub = StubEncoder()
    rc = cli.main(["--audio", str(wav), "--model", "unused.q3w", "--output", str(tmp_path / "out.npy")] + list(extra),
                  encoder_factory=lambda model, n: stub)
    return rc, stub


def test_int16_is_scaled(tmp_path):
    x = np.array([0, 16384, -32768, 32767, 100] * 500, np.int16)
    rc, stub = run(tmp_path, x)
    assert rc == 0
    np.testing.assert_array_equal(stub.got[0], x.astype(np.float32) / 32768.0)
    assert stub.got[0].dtype == np.float32


def test_int32_is_scaled(tmp_path):
    x = np.array([0, 1 << 30, -(1 << 31), 12345] * 500, np.int32)
    rc, stub = run(tmp_path, x)
    assert rc == 0
    np.testing.assert_array_equal(stub.got[0], x.astype(np.float32) / 2147483648.0)


def test_other_dtypes_are_cast_unscaled(tmp_path):
    x = np.array([0, 1, 128, 255] * 500, np.uint8)
    rc, stub = run(tmp_path, x)
    assert rc == 0
    np.testing.assert_array_equal(stub.got[0], x.astype(np.float32))
    f = np.linspace(-2, 2, 3000).astype(np.float32)     # float32: as it is, out-of-range values kept
    rc, stub = run(tmp_path, f)
    np.testing.assert_array_equal(stub.got[0], f)


def test_channels_are_averaged(tmp_path):
    x = np.stack([np.full(2000, 1000, np.int16), np.full(2000, -3000, np.int16)], 1)
    rc, stub = run(tmp_path, x)
    assert rc == 0
    np.testing.assert_allclose(stub.got[0], (1000 / 32768 - 3000 / 32768) / 2, rtol=1e-6)
    assert stub.got[0].shape == (2000,)


def test_other_rates_are_resampled(tmp_path):
    x = (0.3 * np.sin(np.arange(16000) * 2 * np.pi * 200 / 16000)).astype(np.float32)
    rc, stub = run(tmp_path, x, sr=16000)
    assert rc == 0
    assert stub.got[0].size == 24000 and stub.got[0].dtype == np.float32
    assert abs(float(np.sqrt((stub.got[0][1000:-1000] ** 2).mean())) - 0.3 / np.sqrt(2)) < 0.01


def test_output_layout_and_truncation(tmp_path):
    x = np.zeros(1920 * 10 + 7, np.int16)                 # 11 frames
    rc, _ = run(tmp_path, x)
    codes = np.load(tmp_path / "out.npy")
    assert rc == 0 and codes.dtype == np.int64 and codes.shape == (11, 16)
    assert (codes[:, 0] == np.arange(11) * 16).all()     # frame-major, semantic id first
    rc, _ = run(tmp_path, x, extra=["--max_tokens", "4"])
    codes = np.load(tmp_path / "out.npy")
    assert codes.shape == (4, 16) and (codes == np.arange(64).reshape(4, 16)).all()


def test_prompt_dir(tmp_path):
    x = np.zeros(5000, np.int16)
    d = tmp_path / "prompt"
    rc, _ = run(tmp_path, x, extra=["--output_dir", str(d), "--ref_text", "Привет, мир."])
    assert rc == 0
    assert np.load(d / "ref_codec_tokens.npy").shape == (3, 16)
    assert (d / "ref_text.txt").read_text() == "Привет, мир."
    assert not (tmp_path / "out.npy").exists()            # --output_dir replaces --output
    d2 = tmp_path / "prompt2"
    rc, _ = run(tmp_path, x, extra=["--output_dir", str(d2)])
    assert rc == 0 and not (d2 / "ref_text.txt").exists()


def test_unreadable_file(tmp_path, capsys):
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"not a wav file at all")
    called = []
    rc = cli.main(["--audio", str(bad), "--model", "x.q3w"], encoder_factory=lambda m, n: called.append(1))
    assert rc != 0 and not called
    assert "cannot read" in capsys.readouterr().err
    rc = cli.main(["--audio", str(tmp_path / "missing.wav"), "--model", "x.q3w"], encoder_factory=lambda m, n: called.append(1))
    assert rc != 0 and not called


def test_decode_back_needs_vocoder(tmp_path):
    wav = tmp_path / "in.wav"
    wavfile.write(str(wav), 24000, np.zeros(100, np.int16))
    with pytest.raises(SystemExit):
        cli.main(["--audio", str(wav), "--model", "x.q3w", "--decode_back", str(tmp_path / "o.wav")],
                 encoder_factory=lambda m, n: StubEncoder())
