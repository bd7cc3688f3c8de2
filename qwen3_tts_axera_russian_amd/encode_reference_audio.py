"""Encode a reference WAV into 16-group codec ids for a voice-clone prompt (the reference's
scripts/encode_reference_audio.py, on the GPU encoder).

    python -m qwen3_tts_axera_russian_amd.encode_reference_audio --audio ref.wav --model enc.q3w --output_dir prompt/ \
        [--ref_text "..."] [--max_tokens 256] [--decode_back ref_decoded.wav --vocoder voc.q3w] [--stream_seconds 1.0]
        [--resample host|device] [--push_seconds 0.5] [--speaker_model spk.q3w]

Writes ref_codec_tokens.npy (int64 [min(T, max_tokens)][16], the semantic id first) to --output, or, with --output_dir,
a prompt_dir holding ref_codec_tokens.npy and (with --ref_text) ref_text.txt.  --model is an encoder container
(weights.convert_speech_tokenizer_encoder) or a speech_tokenizer/ directory, converted on the fly.  --stream_seconds S
encodes the clip in pushes of S seconds through the streaming encode (Encoder.encode_streaming): device memory is that of
one push, whatever the WAV's length.

WAV loading follows the reference's load_wav: int16 / 32768, int32 / 2^31, any other dtype cast to float32 unscaled,
channels averaged.  Audio at another rate than the encoder's is resampled on the host with scipy.signal.resample_poly in
float32 (--resample host, the default: unchanged, bit for bit), or, with --resample device, handed to the encoder as the
file holds it -- int16 or float32 samples, the channels interleaved -- and decoded, downmixed and resampled on the GPU
(Encoder.encode_pcm / enc_encode_pcm).  The device path is pinned: scipy.signal.resample_poly's rules evaluated in float64 and
rounded once to float32, so every host that opens the library gets the same ids for the same file; the host path depends on
the host's scipy and its float32 arithmetic and is pinned to nothing.  --resample device --push_seconds S sends the file's own
frames through the streaming encode in pushes of round(S * the file's rate) frames (Encoder.encode_streaming_pcm /
enc_stream_push_pcm): the same pinned samples bit for bit whatever S, device memory that of one push, a WAV of any length.
qwen_tts's own resampler is not available here:
neither path is pinned to it.

--speaker_model SPK.q3w (a speaker-encoder container, weights.convert_speaker_encoder / make_synthetic_spk) additionally
writes ref_spk_embedding.npy, float32 [dim], next to ref_codec_tokens.npy: the x-vector of the SAME 24 kHz samples the ids
come from (SpeakerEncoder.embed / spk_embed), in every mode above -- the host-resampled samples, or the device front-end's
(Encoder.resample_pcm / enc_resample_pcm; the streamed modes embed the whole clip once the ids are out, so the clip must
then fit the device).  The whole clip is embedded, whatever --max_tokens keeps of the ids."""
from __future__ import annotations

import argparse
import math
import os
import sys
import tempfile
import time
import wave

import numpy as np


def load_wav(path):
    """-> (float32 mono samples, sample rate), the reference's rules."""
    import scipy.io.wavfile as wavfile
    sr, data = wavfile.read(path)
    if data.dtype == np.int16:
        data = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        data = data.astype(np.float32) / 2147483648.0
    elif data.dtype != np.float32:
        data = data.astype(np.float32)
    if data.ndim > 1:
        data = data.mean(axis=1)
    return np.ascontiguousarray(data, dtype=np.float32), int(sr)


def load_wav_raw(path):
    """-> (the samples as the file holds them, int16 or float32, [n] or [n][channels]; sample rate) for --resample device"""
    import scipy.io.wavfile as wavfile
    sr, data = wavfile.read(path)
    if data.dtype not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError(f"--resample device takes int16 or float32 WAV data, this file holds {data.dtype} (use --resample host)")
    return np.ascontiguousarray(data), int(sr)


def resample(x, sr, target):
    if sr == target:
        return x
    from scipy.signal import resample_poly
    g = math.gcd(int(sr), int(target))
    return resample_poly(x, target // g, sr // g).astype(np.float32)


def open_encoder(model, max_samples):
    """An encoder container, or a speech_tokenizer/ directory (converted into a temporary container)."""
    from .encoder import Encoder
    if os.path.isdir(model):
        from . import weights as W
        tmp = tempfile.NamedTemporaryFile(suffix=".q3w", delete=False)
        tmp.close()
        try:
            _, report = W.convert_speech_tokenizer_encoder(model, tmp.name)
            for line in report:
                print(f"  {line}")
            return Encoder(tmp.name, max_batch=1, max_samples=max_samples)
        finally:
            os.unlink(tmp.name)
    return Encoder(model, max_batch=1, max_samples=max_samples)


def open_speaker(model, max_samples):
    from .speaker import SpeakerEncoder
    return SpeakerEncoder(model, max_batch=1, max_samples=max_samples)


def embed_speaker(a, samples, speaker_factory):
    """--speaker_model: the x-vector of the clip's 24 kHz samples -> float32 [dim]; None without the flag"""
    if not a.speaker_model:
        return None
    samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    # (at least a second of room: a clip below the encoder's shortest is then refused by the check below, with its reason)
    spk = speaker_factory(a.speaker_model, max(int(samples.size), 24000))
    try:
        if spk.sample_rate != 24000:
            raise ValueError(f"the speaker encoder takes {spk.sample_rate} Hz, the samples are at 24000 Hz")
        if samples.size < spk.min_samples:
            raise ValueError(f"the clip has {samples.size} samples at 24 kHz, the speaker encoder needs {spk.min_samples}")
        t0 = time.time()
        emb = spk.embed([samples])[0]
        print(f"Speaker embedding: {emb.size} values, {time.time() - t0:.3f}s (GPU {spk.last_ms():.2f} ms, {spk.last_launches()} launches)")
        return np.ascontiguousarray(emb, dtype=np.float32)
    finally:
        spk.close()


def decode_back(codes, vocoder, out_wav):
    """The reference's "decode back" step: codes -> voc_synthesize (int16, 24 kHz) -> WAV."""
    from .vocoder import Vocoder
    voc = Vocoder(vocoder)
    try:
        pcm = voc.synthesize(codes, int16=True)
    finally:
        voc.close()
    with wave.open(out_wav, "w") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(24000)
        wf.writeframes(pcm.tobytes())
    return len(pcm)


def _save(a, codes, emb=None):
    n_tokens, n_groups = codes.shape
    print(f"Tokens: {n_tokens}, Groups: {n_groups}")
    keep = np.ascontiguousarray(codes[:min(n_tokens, a.max_tokens)], dtype=np.int64)
    if a.output_dir:
        os.makedirs(a.output_dir, exist_ok=True)
        np.save(os.path.join(a.output_dir, "ref_codec_tokens.npy"), keep)
        if a.ref_text:
            with open(os.path.join(a.output_dir, "ref_text.txt"), "w") as f:
                f.write(a.ref_text)
        if emb is not None:
            np.save(os.path.join(a.output_dir, "ref_spk_embedding.npy"), emb)
        print(f"Saved prompt_dir: {a.output_dir}")
    else:
        np.save(a.output, keep)
        print(f"Saved: {a.output}")
        if emb is not None:
            dst = os.path.join(os.path.dirname(os.path.abspath(a.output)), "ref_spk_embedding.npy")
            np.save(dst, emb)
            print(f"Saved: {dst}")
    if a.decode_back:
        n = decode_back(keep, a.vocoder, a.decode_back)
        print(f"Saved decoded: {a.decode_back} ({n} samples)")
    return 0


def main(argv=None, encoder_factory=open_encoder, speaker_factory=open_speaker):
    p = argparse.ArgumentParser(description="Encode reference audio to codec tokens (GPU speech-tokenizer encoder)")
    p.add_argument("--audio", required=True, help="reference audio WAV file")
    p.add_argument("--model", "--model_dir", dest="model", required=True,
                   help="encoder container (.q3w) or a speech_tokenizer/ directory")
    p.add_argument("--output", default="ref_codec_tokens.npy")
    p.add_argument("--output_dir", default=None, help="output directory (creates the prompt_dir structure)")
    p.add_argument("--ref_text", default=None, help="text spoken in the reference audio")
    p.add_argument("--max_tokens", type=int, default=256)
    p.add_argument("--decode_back", default=None, help="also decode the saved ids to this WAV through the vocoder")
    p.add_argument("--vocoder", default=None, help="vocoder container for --decode_back")
    p.add_argument("--stream_seconds", type=float, default=None,
                   help="encode in pushes of this many seconds through the streaming encode (a WAV of any length)")
    p.add_argument("--resample", choices=("host", "device"), default="host",
                   help="host: scipy.signal.resample_poly in float32 before the encoder (default); device: decode, downmix and "
                        "resample on the GPU, pinned to resample_poly's float64 result")
    p.add_argument("--push_seconds", type=float, default=None,
                   help="with --resample device: stream the file's own frames in pushes of this many seconds (a WAV of any length)")
    p.add_argument("--speaker_model", default=None,
                   help="speaker-encoder container (.q3w): also write ref_spk_embedding.npy, the x-vector of the same 24 kHz samples")
    a = p.parse_args(argv)
    if a.resample == "device" and a.stream_seconds is not None:
        p.error("--resample device streams with --push_seconds (--stream_seconds pushes host-resampled 24 kHz samples)")
    if a.push_seconds is not None and a.resample != "device":
        p.error("--push_seconds needs --resample device (--stream_seconds streams the host path)")
    if a.push_seconds is not None and not a.push_seconds > 0:
        p.error("--push_seconds must be > 0")
    if a.decode_back and not a.vocoder:
        p.error("--decode_back needs --vocoder")
    if a.stream_seconds is not None and not a.stream_seconds > 0:
        p.error("--stream_seconds must be > 0")
    if a.max_tokens < 1:
        p.error("--max_tokens must be >= 1")
    try:
        x, sr = load_wav(a.audio) if a.resample == "host" else load_wav_raw(a.audio)
    except Exception as e:   # (missing, unreadable, not a WAV)
        print(f"error: cannot read {a.audio}: {e}", file=sys.stderr)
        return 2
    if x.size == 0:
        print(f"error: {a.audio} holds no samples", file=sys.stderr)
        return 2
    print(f"Audio: {a.audio}\n  Duration: {x.shape[0] / sr:.2f}s, SR: {sr}")
    if a.resample == "device" and a.push_seconds is not None:
        push = max(int(round(a.push_seconds * sr)), 1)
        room = -(-push * 24000 // sr) + 32          # 24 kHz samples one push may settle (32: the filter's tail at a finish)
        enc = encoder_factory(a.model, room)        # (the handle's whole-clip buffers are not used: sized for one push)
        t0 = time.time()
        try:
            codes = enc.encode_streaming_pcm(x, sr, channels=1 if x.ndim == 1 else x.shape[1], push_frames=push, max_push_samples=room)
        except (ValueError, RuntimeError) as e:
            print(f"error: {e}", file=sys.stderr)
            return 2
        print(f"Encode time: {time.time() - t0:.3f}s (streamed, pushes of up to {push} frames at {sr} Hz, front-end on the device)")
        emb = None
        if a.speaker_model:   # the whole clip through the same front-end (the stream's samples bit for bit), then embedded
            try:
                whole = encoder_factory(a.model, -(-x.shape[0] * 24000 // sr))
                emb = embed_speaker(a, whole.resample_pcm([x], sr, channels=1 if x.ndim == 1 else x.shape[1])[0], speaker_factory)
            except (ValueError, RuntimeError) as e:
                print(f"error: {e}", file=sys.stderr)
                return 2
        return _save(a, codes, emb)
    if a.resample == "device":
        enc = encoder_factory(a.model, -(-x.shape[0] * 24000 // sr))
        t0 = time.time()
        try:
            codes = enc.encode_pcm([x], sr, channels=1 if x.ndim == 1 else x.shape[1])[0]
            ms = enc.last_ms()
            emb = embed_speaker(a, enc.resample_pcm([x], sr, channels=1 if x.ndim == 1 else x.shape[1])[0], speaker_factory) \
                if a.speaker_model else None
        except (ValueError, RuntimeError) as e:
            print(f"error: {e}", file=sys.stderr)
            return 2
        print(f"Encode time: {time.time() - t0:.3f}s (GPU {ms:.2f} ms, front-end on the device)")
        return _save(a, codes, emb)
    x = resample(x, sr, 24000)
    if a.stream_seconds is None:
        enc = encoder_factory(a.model, max(int(x.size), 1))
    else:   # the handle's whole-clip buffers are not used: sized for one push
        enc = encoder_factory(a.model, max(int(round(a.stream_seconds * 24000)), 1))
    if enc.sample_rate != 24000:
        x = resample(x, 24000, enc.sample_rate)
    t0 = time.time()
    if a.stream_seconds is None:
        codes = enc.encode([x])[0]
        print(f"Encode time: {time.time() - t0:.3f}s (GPU {enc.last_ms():.2f} ms)")
    else:
        push = max(int(round(a.stream_seconds * enc.sample_rate)), 1)
        codes = enc.encode_streaming(x, push)
        print(f"Encode time: {time.time() - t0:.3f}s (streamed, {-(-x.size // push)} pushes of {push} samples)")
    try:
        emb = embed_speaker(a, x, speaker_factory)
    except (ValueError, RuntimeError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    return _save(a, codes, emb)


if __name__ == "__main__":
    sys.exit(main())
