"""What a request of batch_server means: its keys beside texts / token_ids (batch_wire), the checks that answer a malformed
one with -2, and the utterance the server queues for the scheduler.  No socket, no GPU.

Sampling (`--concurrent`): requests may carry the keys "temperature", "top_k", "top_p", "cp_temperature", "cp_top_k" and "seed"
(a missing key takes the server's value; the other modes keep the server's settings and ignore them).

A request may carry "vocoder": "incremental" (default "walk"; any other value is answered with -2): its PCM then comes from the
carry-state incremental decode (voc_incr_push: the samples of every check's new frames at once, one seamless decode per
utterance) instead of the chunk walk -- streamed, or unstreamed through Vocoder.synthesize_incremental, the same bits either way.
Such a request may also carry "vocoder_arithmetic": "exact" (the default) or "split" (the split-fp16 convolutions,
voc_incr_set_arithmetic); any other value, or the key on a request that is not "vocoder": "incremental", is answered with -2.
Records, framing and the single-writer worker are the same.

Codec prompts (`--concurrent` only): a request may carry "prompt_codes" -- one [T][16] list of codec ids shared by its
utterances, or a list of one such list per utterance -- and every utterance then CONTINUES that audio: the frames count as
frames it has already emitted (include/qwen3tts_engine.h, q3e_admit_prompted), and the reply holds the generated frames
and their audio only.  "prompt_token_ids" / "prompt_text" (optional) is the text spoken in the prompt: it is put in front
of each utterance's text ids, and the EOS heuristics count both.  `--voice NAME=DIR` (repeatable; DIR as
encode_reference_audio --output_dir writes it: ref_codec_tokens.npy and, if there, ref_text.txt) names such a pair, and a
request's "voice": "NAME" stands for the same two keys.  With "vocoder": "incremental" the prompt's frames are pushed into
the utterance's stream first and their voc_incr_samples(T) samples dropped, so the audio continues the prompt seamlessly;
the chunk walk (the default) decodes the generated frames on their own.  A prompt in any other mode, together with
"text_stream" (without `--text_voice`, batch_server), an unknown voice, malformed codes, or one that does not fit n_ctx is
answered with -2 for that request alone, before any of it is queued.  Prompt text in front of the target text is a
recollection of the model's in-context mode: parity with real weights is not pinned.  With `--prefix_cache` the key of a
prompted utterance is of the kind b"prompt" and digests the ids and the prompt's codes.

Sampler rules (`--concurrent --sampler_rules`): a request may carry "repetition_penalty" (>= 1), "repetition_window" (1..30
last ids, 0 = every id the utterance has emitted), "eos_boost" (>= 0), "eos_force" (>= 0, 0 = never), "min_tokens" (frames
generated before EOS may be chosen) and "cp_top_p" ((0, 1]) -- q3e_slot_rules, include/qwen3tts_engine.h -- and "sampler":
"reference" (the defaults: the reference's constants, what a request without any of these keys gets) or "upstream"
(SAMPLER_PRESETS: a recollection of the upstream model's generation settings, NOT pinned against its shipped config);
explicit keys override the preset.  Every utterance of the request runs under the same rules.  Without the flag a request
that carries any of these keys, and with it a wrong type or a value out of range, is answered -2 for that request alone.

Audio prompts (`--concurrent --encoder ENC.q3w`): instead of "prompt_codes" a request may carry "prompt_audio": {"format":
"s16" | "f32", "rate": R, "channels": C, "frames": n, "max_frames": K (optional)} -- or a list of such objects, one per
utterance -- and the clips' raw little-endian interleaved bytes (n * C * itemsize per descriptor, in order) right behind the
JSON on the same connection, before any text record.  The server encodes them on the GPU (Encoder.encode_pcm: the PCM
front-end pinned to scipy.signal.resample_poly's float64 result, then the speech-tokenizer encoder), keeps the first K
frames, and from there on the request IS the request with "prompt_codes" equal to those ids: the same checks, the same prefix
key, the same reply bit for bit.  What the JSON alone shows to be wrong (no encoder, a malformed descriptor, a rate, channel
count or length outside the front-end's limits or beyond --prompt_audio_seconds, "prompt_audio" beside "prompt_codes" /
"voice") is answered -2 before any payload byte is read, and the connection closes; a payload that ends early fails that
request alone.  Encoded ids are kept in an LRU (PromptAudioCache, --prompt_audio_cache entries) under a digest of the
descriptor and the payload: a repeated clip runs no encode.  "register_voice": "NAME" (with one "prompt_audio" object) stores
the ids and the prompt's text under NAME for later "voice": "NAME" requests; with "texts": [] the request only registers and is
answered i32 0.  A --voice name cannot be replaced, a run-time one can, and at most --max_voices run-time names are kept.

Speaker embedding (`--concurrent`): a request may carry "speaker_embedding" -- a list of `hidden` finite numbers shared by its
utterances, or a list of such lists, one per utterance -- and every utterance's prefix then carries ONE more row, tts_pad_embed
+ the embedding, after the tts_pad + codec_think_eos row (frontend.build_prefix(speaker=); the row's position is a
recollection of the model's voice-clone prefix, not pinned).  Alone it is the "x-vector only" mode, which needs no transcript;
beside "prompt_codes" / "voice" the utterance gets both halves of a cloned voice.  `--voice NAME=DIR` picks up
ref_spk_embedding.npy (encode_reference_audio --speaker_model) when DIR has one, and a "voice" request then gets both halves;
"speaker": "off" in the request leaves the embedding out.  `--speaker_encoder SPK.q3w` (needs `--encoder`): a "prompt_audio"
request may carry "speaker": "with_prompt" (the embedding of the clip's 24 kHz samples -- enc_resample_pcm, the samples the
codec prompt is encoded from -- beside its codec prompt), "only" (the clip feeds the speaker encoder alone: no codec prompt, no
prompt text, no vocoder warm-up) or "off" (the default: today's behaviour); from there on the request IS the request with the
embedding (and the codes) sent inline.  "register_voice" keeps the embedding with the voice, the prompt-audio LRU keeps it with
the ids under the same digest and counters.  The prefix key of such an utterance also digests the embedding's bytes.  A wrong
length, a non-finite value, "speaker" without --speaker_encoder (or without "prompt_audio"), "only" beside "prompt_codes" or
"register_voice", a clip below the speaker encoder's shortest, and any mode but --concurrent are answered -2 for that request
alone.  No claim about voice similarity is made.

Log-probabilities (`--concurrent --logprobs`): a request may carry "logprobs": true, and its reply then holds, beside every
utterance's codes, one float32 per id: the model's log-probability, at temperature 1, of the id the stream continued with
(include/qwen3tts_engine.h, q3e_scores_reserve: the model's distribution, not the sampler's -- no sampling key or sampler
rule enters it).  They align with the codes the reply holds: a prompted utterance's generated frames, not its prompt's.
batch_wire says where they stand in the reply; "logprobs": false is a request without the key.  The key without the flag (in
any other mode too), or with a value that is not a boolean, is answered -2 for that request alone.
"""
from __future__ import annotations

import collections
import dataclasses
import hashlib
import math
import os
import struct
import threading

import numpy as np

VOCODER_MODES = ("walk", "incremental")
VOCODER_ARITHMETICS = ("exact", "split")
PROMPT_KEYS = ("prompt_codes", "prompt_token_ids", "prompt_text", "voice", "prompt_audio", "register_voice")
PROMPT_AUDIO_FORMATS = {"s16": np.dtype("<i2"), "f32": np.dtype("<f4")}
# the PCM front-end's limits (include/qwen3tts_enc_pcm.h, csrc/q3_enc_pcm_host.h)
PCM_RATE, PCM_MIN_RATE, PCM_MAX_RATE, PCM_MAX_CHANNELS, PCM_MAX_FACTOR = 24000, 8000, 192000, 8, 640
SPEAKER_KEYS = ("speaker_embedding", "speaker")
SPEAKER_MODES = ("off", "only", "with_prompt")
_PARAM_KEYS = ("temperature", "top_k", "top_p", "cp_temperature", "cp_top_k", "seed")   # request keys = SlotParams fields
# request key -> SlotRules field
_RULE_KEYS = {"repetition_penalty": "rep_penalty", "repetition_window": "rep_window", "eos_boost": "eos_boost",
              "eos_force": "eos_force", "min_tokens": "min_frames", "cp_top_p": "cp_top_p"}
RULE_KEYS = tuple(_RULE_KEYS) + ("sampler",)
# "upstream": a mild penalty over the whole emitted history, a minimum length, no length-based EOS heuristics -- as far as
# this repository recollects the upstream model's generation settings; not pinned
SAMPLER_PRESETS = {"reference": {}, "upstream": dict(rep_penalty=1.05, rep_window=0, eos_boost=0.0, eos_force=0.0, min_frames=2)}


def prefix_key(kind, token_ids, prompt_codes=None, speaker=None):
    """The prefix cache's key of an utterance: the first 16 bytes of a SHA-256 over the kind of prefix (b"full": the
    dual-stream prefix of the whole text, b"stream": the streaming prefix, b"prompt": the dual-stream prefix followed by
    the rows of a codec prompt) and the int32 token ids that determine its rows -- for b"stream" the first token alone,
    for b"prompt" the ids (the prompt's text first), their number, and the prompt's [T][16] codes.  speaker (the float32
    embedding of a prefix with a speaker row): the kind becomes kind + b"+spk" and a SHA-256 of the embedding's bytes is
    digested too; None leaves the key as it always was."""
    ids = np.asarray(token_ids, dtype="<i4").reshape(-1)
    tail = b""
    if speaker is not None:
        kind = bytes(kind) + b"+spk"
        tail = hashlib.sha256(np.ascontiguousarray(speaker, dtype="<f4").tobytes()).digest()
    if prompt_codes is None:
        return hashlib.sha256(bytes(kind) + b"\0" + ids.tobytes() + tail).digest()[:16]
    codes = np.asarray(prompt_codes, dtype="<i4").reshape(-1, 16)
    return hashlib.sha256(bytes(kind) + b"\0" + struct.pack("<i", len(ids)) + ids.tobytes() + codes.tobytes() + tail).digest()[:16]


def request_has_speaker(msg):
    """Whether a request carries a speaker key."""
    return any(msg.get(k) is not None for k in SPEAKER_KEYS)


def request_speaker_mode(msg):
    """A request's "speaker" key -> "off" (the default), "only" or "with_prompt"; raises ValueError on any other value."""
    v = msg.get("speaker")
    if v is None:
        return "off"
    if not isinstance(v, str) or v not in SPEAKER_MODES:
        raise ValueError(f"speaker must be one of {SPEAKER_MODES} (got {v!r})")
    return v


def request_speaker_embedding(value, n_utts, hidden):
    """A request's "speaker_embedding" -> one float32 [hidden] array per utterance: one list of `hidden` finite numbers shared
    by the utterances, or a list of n_utts such lists.  Raises ValueError on any other shape, type, length or a non-finite value."""
    def one(v):
        if isinstance(v, np.ndarray):
            v = v.tolist()
        if not isinstance(v, list) or any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in v):
            raise ValueError("a speaker embedding is a list of numbers")
        if len(v) != hidden:
            raise ValueError(f"a speaker embedding of {len(v)} values, the model's hidden size is {hidden}")
        try:
            a = np.asarray(v, dtype=np.float64)
        except OverflowError:               # (a JSON integer beyond the doubles)
            raise ValueError("a speaker embedding value is out of range") from None
        with np.errstate(over="ignore"):
            a = a.astype(np.float32)
        if not np.isfinite(a).all():
            raise ValueError("a speaker embedding value is not finite (as float32)")
        return a
    if isinstance(value, np.ndarray):
        value = value.tolist()
    if not isinstance(value, list) or not value:
        raise ValueError('"speaker_embedding" is a list of numbers, or a list of such lists, one per utterance')
    if not isinstance(value[0], list):
        return [one(value)] * n_utts
    if len(value) != n_utts:
        raise ValueError(f'"speaker_embedding" holds {len(value)} embeddings for {n_utts} utterances')
    return [one(v) for v in value]


@dataclasses.dataclass(eq=False)
class Utterance:
    """An utterance as the server's _prepare queues it for the scheduler."""
    utt: int                        # its index in the request
    prefix: np.ndarray              # prefix rows [n][hidden]
    n_text: int
    params: object                  # engine.SlotParams
    feed: object = None             # TextFeed of a "text_stream" request
    prefix_key: bytes = None        # the prefix cache's key of its prefix (None: admitted uncached)
    prompt: np.ndarray = None       # its codec prompt [T][16] int32 (None: it has none; an empty one counts as none)
    rules: object = None            # engine.SlotRules of a request with sampler rules (None: the defaults)

    def __post_init__(self):
        if self.prompt is not None and not len(self.prompt):
            self.prompt = None


def request_vocoder(msg):
    """A request's "vocoder" key -> "walk" (the default) or "incremental"; raises ValueError on any other value."""
    v = msg.get("vocoder", "walk")
    if not isinstance(v, str) or v not in VOCODER_MODES:
        raise ValueError(f"vocoder must be one of {VOCODER_MODES} (got {v!r})")
    return v


def request_vocoder_arithmetic(msg):
    """A request's "vocoder_arithmetic" key -> "exact" (the default) or "split"; raises ValueError on any other value, and on
    the key in a request that is not "vocoder": "incremental"."""
    vocoder = request_vocoder(msg)
    if "vocoder_arithmetic" not in msg:
        return "exact"
    a = msg["vocoder_arithmetic"]
    if not isinstance(a, str) or a not in VOCODER_ARITHMETICS:
        raise ValueError(f"vocoder_arithmetic must be one of {VOCODER_ARITHMETICS} (got {a!r})")
    if vocoder != "incremental":
        raise ValueError('vocoder_arithmetic needs "vocoder": "incremental"')
    return a


def request_has_prompt(msg):
    """Whether a request carries a codec prompt, or any key that belongs to one."""
    return any(msg.get(k) is not None for k in PROMPT_KEYS)


def request_prompt_codes(codes, n_utts, cp_vocab=2048):
    """A request's "prompt_codes" -> one [T][16] int32 array per utterance: one [T][16] list shared by the utterances, or a
    list of n_utts such lists.  Column 0 holds audio ids (0..2047), the others ids of the code predictor's vocabulary;
    raises ValueError on any other shape, type or value."""
    def one(c):
        if isinstance(c, np.ndarray):
            c = c.tolist()
        if not isinstance(c, list) or any(not isinstance(f, list) or len(f) != 16 for f in c):
            raise ValueError("a codec prompt is a list of frames of 16 ids")
        if any(isinstance(t, bool) or not isinstance(t, int) for f in c for t in f):
            raise ValueError("codec prompt ids are integers")
        a = np.asarray(c, np.int64).reshape(-1, 16)
        if len(a) and (a.min() < 0 or a[:, 0].max() >= 2048 or a[:, 1:].max() >= cp_vocab):
            raise ValueError(f"codec prompt ids lie in 0..2047 (column 0) and 0..{cp_vocab - 1} (the others)")
        return a.astype(np.int32)
    if isinstance(codes, np.ndarray):
        codes = codes.tolist()
    if not isinstance(codes, list):
        raise ValueError('"prompt_codes" is a list')
    shared = all(isinstance(f, list) and len(f) == 16 and not any(isinstance(t, list) for t in f) for f in codes)
    if shared:                          # [T][16] (or an empty prompt)
        return [one(codes)] * n_utts
    if len(codes) != n_utts:
        raise ValueError(f'"prompt_codes" holds {len(codes)} prompts for {n_utts} utterances')
    return [one(c) for c in codes]


@dataclasses.dataclass(frozen=True)
class AudioDescriptor:
    """One clip of a request's "prompt_audio", checked."""
    format: str
    rate: int
    channels: int
    frames: int
    max_frames: int = None          # keep the first K ids (None: all)

    @property
    def dtype(self):
        return PROMPT_AUDIO_FORMATS[self.format]

    @property
    def nbytes(self):
        return self.frames * self.channels * self.dtype.itemsize

    @property
    def samples_24k(self):
        """the clip's length after the front-end: ceil(frames * up / down)"""
        g = math.gcd(self.rate, PCM_RATE)
        return -(-self.frames * (PCM_RATE // g) // (self.rate // g))

    def array(self, payload):
        """the payload's bytes -> the clip as Encoder.encode_pcm takes it"""
        a = np.frombuffer(payload, self.dtype)
        return a if self.channels == 1 else a.reshape(-1, self.channels)


def request_prompt_audio(spec, n_utts, max_samples):
    """A request's "prompt_audio" -> (its AudioDescriptors, shared): one object shared by the utterances (shared = True), or a
    list of n_utts objects.  max_samples: the 24 kHz samples the server's encoder takes per clip (--prompt_audio_seconds).
    Raises ValueError on anything the front-end or the server would refuse -- all of it visible in the JSON alone."""
    def integer(d, key, lo, hi, required=True):
        v = d.get(key)
        if v is None and not required:
            return None
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'"prompt_audio": "{key}" is an integer in {lo}..{hi} (got {v!r})')
        return v

    def one(d):
        if not isinstance(d, dict):
            raise ValueError('"prompt_audio" is an object (or a list of objects, one per utterance)')
        unknown = set(d) - {"format", "rate", "channels", "frames", "max_frames"}
        if unknown:
            raise ValueError(f'"prompt_audio": unknown keys {sorted(unknown)}')
        fmt = d.get("format")
        if not isinstance(fmt, str) or fmt not in PROMPT_AUDIO_FORMATS:
            raise ValueError(f'"prompt_audio": "format" is one of {tuple(PROMPT_AUDIO_FORMATS)} (got {fmt!r})')
        rate = integer(d, "rate", PCM_MIN_RATE, PCM_MAX_RATE)
        g = math.gcd(rate, PCM_RATE)
        if max(PCM_RATE // g, rate // g) > PCM_MAX_FACTOR:
            raise ValueError(f'"prompt_audio": {rate} Hz resamples by {PCM_RATE // g}/{rate // g}, a factor above {PCM_MAX_FACTOR}')
        desc = AudioDescriptor(fmt, rate, integer(d, "channels", 1, PCM_MAX_CHANNELS), integer(d, "frames", 1, 2 ** 31 - 1),
                               integer(d, "max_frames", 1, 2 ** 31 - 1, required=False))
        if desc.samples_24k > max_samples:
            raise ValueError(f'"prompt_audio": {desc.frames} frames at {rate} Hz are {desc.samples_24k / PCM_RATE:.2f} s, the '
                             f"server takes {max_samples / PCM_RATE:.2f} s (--prompt_audio_seconds)")
        return desc
    if isinstance(spec, list):
        if len(spec) != n_utts:
            raise ValueError(f'"prompt_audio" holds {len(spec)} clips for {n_utts} utterances')
        return [one(d) for d in spec], False
    return [one(spec)], True


def prompt_audio_digest(desc, payload):
    """The id cache's key of a clip: SHA-256 over (format, channels, rate, K, the payload's bytes)."""
    head = struct.pack("<4siiq", desc.format.encode(), desc.channels, desc.rate, -1 if desc.max_frames is None else desc.max_frames)
    return hashlib.sha256(head + bytes(payload)).digest()


class PromptAudioCache:
    """LRU of encoded prompts: digest -> int64 ids [T][16] (after "max_frames") and, beside them under the same digest, the
    clip's speaker embedding (float32 [hidden]) once a request has asked for it.  Only the thread that resolves audio prompts
    touches it.  n = 0: nothing is kept (every clip is a miss)."""

    def __init__(self, n):
        if int(n) < 0:
            raise ValueError("--prompt_audio_cache takes a number of entries >= 0")
        self.n, self.hits, self.misses, self.evictions = int(n), 0, 0, 0
        self._lru = collections.OrderedDict()      # digest -> [ids or None, speaker embedding or None]

    def lookup(self, key, want_ids=True, want_speaker=False):
        """-> (ids, speaker) as far as the entry holds them (None each otherwise).  A hit when everything wanted is there:
        nothing then runs on the GPU for this clip; a miss otherwise (the caller computes what is missing and puts it)."""
        e = self._lru.get(key)
        if e is None or (want_ids and e[0] is None) or (want_speaker and e[1] is None):
            self.misses += 1
            return (None, None) if e is None else (e[0], e[1])
        self._lru.move_to_end(key)
        self.hits += 1
        return e[0], e[1]

    def get(self, key):
        return self.lookup(key)[0]

    def put(self, key, ids=None, speaker=None):
        """what has been computed for the clip, beside what its entry already holds"""
        if not self.n:
            return
        e = self._lru.setdefault(key, [None, None])
        if ids is not None:
            e[0] = ids
        if speaker is not None:
            e[1] = speaker
        self._lru.move_to_end(key)
        while len(self._lru) > self.n:
            self._lru.popitem(last=False)
            self.evictions += 1

    def __len__(self):
        return len(self._lru)


class VoiceTable:
    """The voices a request may name: the start-up ones (--voice NAME=DIR, fixed) and up to max_runtime registered at run time
    ("register_voice", replaceable).  name -> (codes as "prompt_codes" takes them, the prompt's text: a str, token ids, or
    None).  Read and written under one lock."""

    def __init__(self, startup=None, max_runtime=64):
        if int(max_runtime) < 0:
            raise ValueError("--max_voices takes a number >= 0")
        self._startup, self._runtime, self.max_runtime = dict(startup or {}), {}, int(max_runtime)
        self._speakers = {}             # name -> the voice's speaker embedding (float32 [hidden]), for the names that have one
        self._lock = threading.Lock()

    def get(self, name):
        with self._lock:
            return self._startup.get(name) or self._runtime.get(name)

    def __contains__(self, name):
        return self.get(name) is not None

    def check_register(self, name):
        """raises ValueError if `name` cannot be registered now"""
        if not isinstance(name, str) or not name:
            raise ValueError('"register_voice" is a non-empty string')
        with self._lock:
            if name in self._startup:
                raise ValueError(f"voice {name!r} was given at start-up (--voice): it cannot be replaced")
            if name not in self._runtime and len(self._runtime) >= self.max_runtime:
                raise ValueError(f"{len(self._runtime)} voices are registered (--max_voices {self.max_runtime})")

    def register(self, name, codes, text, speaker=None):
        self.check_register(name)
        with self._lock:
            self._runtime[name] = (codes, text)
            self._speakers.pop(name, None)
            if speaker is not None:
                self._speakers[name] = np.ascontiguousarray(speaker, np.float32)

    def set_startup_speaker(self, name, speaker):
        with self._lock:
            self._speakers[name] = np.ascontiguousarray(speaker, np.float32)

    def speaker(self, name):
        """the speaker embedding kept with voice `name` (None: it has none)"""
        with self._lock:
            return self._speakers.get(name)

    def runtime_names(self):
        with self._lock:
            return list(self._runtime)


def load_voice(prompt_dir):
    """A directory as encode_reference_audio --output_dir writes it -> (codes as "prompt_codes" takes them, the text of
    ref_text.txt or None)."""
    codes = np.load(os.path.join(prompt_dir, "ref_codec_tokens.npy"))
    if codes.ndim != 2 or codes.shape[1] != 16 or not np.issubdtype(codes.dtype, np.integer):
        raise ValueError(f"{prompt_dir}: ref_codec_tokens.npy is not an integer array [T][16]")
    text = None
    if os.path.exists(os.path.join(prompt_dir, "ref_text.txt")):
        with open(os.path.join(prompt_dir, "ref_text.txt")) as f:
            text = f.read()
    return codes.astype(np.int64).tolist(), text


def load_voice_speaker(prompt_dir, hidden):
    """ref_spk_embedding.npy of a voice directory (encode_reference_audio --speaker_model) -> float32 [hidden], or None when
    the directory has none; raises ValueError on a wrong shape or a non-finite value."""
    path = os.path.join(prompt_dir, "ref_spk_embedding.npy")
    if not os.path.exists(path):
        return None
    a = np.load(path)
    if a.ndim != 1 or a.shape[0] != hidden or not np.issubdtype(a.dtype, np.floating) or not np.isfinite(a).all():
        raise ValueError(f"{prompt_dir}: ref_spk_embedding.npy is not a finite float array [{hidden}]")
    return np.ascontiguousarray(a, np.float32)


def request_logprobs(msg, enabled):
    """A request's "logprobs" key -> whether its reply carries the log-probabilities.  Raises ValueError on the key when the
    server runs without --logprobs (`enabled` false) and on a value that is not a boolean."""
    v = msg.get("logprobs")
    if v is None:
        return False
    if not isinstance(v, bool):
        raise ValueError(f"logprobs must be true or false (got {v!r})")
    if not enabled:
        raise ValueError("logprobs need a --concurrent --logprobs server")
    return v


def request_has_rules(msg):
    """Whether a request carries a sampler-rules key."""
    return any(msg.get(k) is not None for k in RULE_KEYS)


def request_slot_rules(msg, enabled):
    """A request's sampler-rules keys -> engine.SlotRules, or None for a request without any of them.  The "sampler" preset
    first, explicit keys over it.  Raises ValueError on such a key when the server runs without --sampler_rules (`enabled`
    false), on an unknown preset, a wrong type or a value out of range."""
    from .engine import SlotRules
    if not request_has_rules(msg):
        return None
    if not enabled:
        raise ValueError("sampler rules need a --concurrent --sampler_rules server")
    kw = {}
    preset = msg.get("sampler")
    if preset is not None:
        if not isinstance(preset, str) or preset not in SAMPLER_PRESETS:
            raise ValueError(f"sampler must be one of {tuple(SAMPLER_PRESETS)} (got {preset!r})")
        kw.update(SAMPLER_PRESETS[preset])
    for key, field in _RULE_KEYS.items():
        v = msg.get(key)
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{key} must be a number (got {v!r})")
        if field in ("rep_window", "min_frames"):
            if not (isinstance(v, int) or float(v).is_integer()):
                raise ValueError(f"{key} must be an integer (got {v!r})")
            kw[field] = int(v)
        else:
            try:
                kw[field] = float(v)
            except OverflowError:       # (a JSON integer beyond the doubles)
                raise ValueError(f"{key} is out of range (got {v!r})") from None
    rules = SlotRules(**kw)
    rules.check()
    return rules


def request_slot_params(msg, defaults, max_tokens_cap):
    """--concurrent: a request's sampling keys and max_tokens over the server's defaults -> SlotParams (utt 0); raises
    ValueError on a value out of range or of the wrong type."""
    kw = {}
    for key in _PARAM_KEYS:
        v = msg.get(key)
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{key} must be a number (got {v!r})")
        if key in ("top_k", "cp_top_k", "seed") and not (isinstance(v, int) or float(v).is_integer()):
            raise ValueError(f"{key} must be an integer (got {v!r})")
        kw[key] = int(v) if key in ("top_k", "cp_top_k", "seed") else float(v)
    mt = msg.get("max_tokens")
    if mt is not None and (isinstance(mt, bool) or not isinstance(mt, int)):
        raise ValueError(f"max_tokens must be an integer (got {mt!r})")
    kw["max_frames"] = min(int(mt), max_tokens_cap) if mt else defaults.max_frames
    p = dataclasses.replace(defaults, **kw)
    p.check(max_tokens_cap)
    return p
