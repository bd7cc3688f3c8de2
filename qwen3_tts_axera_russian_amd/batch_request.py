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
"""
from __future__ import annotations

import dataclasses
import hashlib
import os
import struct

import numpy as np

VOCODER_MODES = ("walk", "incremental")
VOCODER_ARITHMETICS = ("exact", "split")
PROMPT_KEYS = ("prompt_codes", "prompt_token_ids", "prompt_text", "voice")
_PARAM_KEYS = ("temperature", "top_k", "top_p", "cp_temperature", "cp_top_k", "seed")   # request keys = SlotParams fields
# request key -> SlotRules field
_RULE_KEYS = {"repetition_penalty": "rep_penalty", "repetition_window": "rep_window", "eos_boost": "eos_boost",
              "eos_force": "eos_force", "min_tokens": "min_frames", "cp_top_p": "cp_top_p"}
RULE_KEYS = tuple(_RULE_KEYS) + ("sampler",)
# "upstream": a mild penalty over the whole emitted history, a minimum length, no length-based EOS heuristics -- as far as
# this repository recollects the upstream model's generation settings; not pinned
SAMPLER_PRESETS = {"reference": {}, "upstream": dict(rep_penalty=1.05, rep_window=0, eos_boost=0.0, eos_force=0.0, min_frames=2)}


def prefix_key(kind, token_ids, prompt_codes=None):
    """The prefix cache's key of an utterance: the first 16 bytes of a SHA-256 over the kind of prefix (b"full": the
    dual-stream prefix of the whole text, b"stream": the streaming prefix, b"prompt": the dual-stream prefix followed by
    the rows of a codec prompt) and the int32 token ids that determine its rows -- for b"stream" the first token alone,
    for b"prompt" the ids (the prompt's text first), their number, and the prompt's [T][16] codes."""
    ids = np.asarray(token_ids, dtype="<i4").reshape(-1)
    if prompt_codes is None:
        return hashlib.sha256(bytes(kind) + b"\0" + ids.tobytes()).digest()[:16]
    codes = np.asarray(prompt_codes, dtype="<i4").reshape(-1, 16)
    return hashlib.sha256(bytes(kind) + b"\0" + struct.pack("<i", len(ids)) + ids.tobytes() + codes.tobytes()).digest()[:16]


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
