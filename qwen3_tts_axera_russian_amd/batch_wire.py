"""The batched protocol of batch_server and its clients (standard library, numpy and protocol only: no engine, no GPU).

Extension of the reference's wire protocol, same conventions (little-endian, u32 length + UTF-8 JSON):

    request   u32 len + JSON {"texts": [...], "language": "...", "max_tokens": N}   or {"token_ids": [[...], ...]}
    reply     i32 n_utterances (or -2 on error), then per utterance:
              i32 n_frames, i32[n_frames*16] codes, i32 n_samples, i16[n_samples] PCM (24 kHz)

Streamed reply (the request carries "stream": true): the same synthesis, handed out while the frame loop runs, as records on
the same connection (in the order they are ready; `utt` indexes the request's utterances):

              i32 1, i32 utt, i32 n, i16[n]                  PCM of utterance utt: the next n samples
              i32 2, i32 utt, i32 n_frames, i32[n_frames*16]  utterance utt has ended: all its codes
              i32 -1                                          the request is done   (i32 -2: error, as above)

Log-probabilities (`--concurrent --logprobs`; the request carries "logprobs": true -- batch_request): in the unstreamed reply
every utterance's block is followed by

              i32 n_frames, f32[n_frames*16]                  the log-probability of every id of its codes

and in the streamed reply one record, immediately before that utterance's end record:

              i32 3, i32 utt, i32 n_frames, f32[n_frames*16]

A reply to a request without the key is byte for byte what it always was.

Streamed TEXT (`--concurrent` only; the request carries "text_stream": true, which needs "stream": true and exactly one
utterance, else -2): the request's texts / token_ids hold only the first piece of the text (at least one token), and the
client goes on sending the rest on the same connection, as records

              i32 1, i32 n, n UTF-8 bytes (cut anywhere)      more text, tokenised by the server's incremental tokeniser
              i32 2, i32 n, i32[n]                             more token ids
              i32 0, i32 0                                     end of text

while the audio records already come back.  The request's other keys: batch_request.

Audio prompt (`--concurrent --encoder`): a request that carries "prompt_audio" (one descriptor {"format", "rate", "channels",
"frames"[, "max_frames"]}, or a list of them, one per utterance) is followed on the same connection by the clips' raw
little-endian interleaved PCM -- frames * channels * itemsize bytes per descriptor, in order, no framing -- before any text
record.  A request with "register_voice" and "texts": [] is answered i32 0.

Speaker embedding (`--concurrent`): "speaker_embedding" travels in the JSON as numbers (a float32 survives the trip bit for
bit), "speaker" beside "prompt_audio" names where the server takes it from; there is no new record and no new payload.
"""
from __future__ import annotations

import json
import socket
import struct
import threading

import numpy as np

from . import protocol as P

REC_AUDIO, REC_END, REC_SCORES = 1, 2, 3     # the records of a streamed reply


def pack_batch_request(texts=None, token_ids=None, language="russian", max_tokens=None, stream=False, temperature=None,
                       top_k=None, top_p=None, cp_temperature=None, cp_top_k=None, seed=None, vocoder=None,
                       vocoder_arithmetic=None, text_stream=False, prompt_codes=None, prompt_token_ids=None, prompt_text=None,
                       voice=None, sampler=None, repetition_penalty=None, repetition_window=None, eos_boost=None, eos_force=None,
                       min_tokens=None, cp_top_p=None, prompt_audio=None, prompt_audio_max_frames=None, register_voice=None,
                       logprobs=None, speaker_embedding=None, speaker=None) -> bytes:
    """The request of the batched protocol; the sampling keys (honoured by --concurrent), the vocoder mode ("walk" /
    "incremental") and the incremental mode's arithmetic ("exact" / "split") are sent only when given.  text_stream: the
    request carries only the first piece of its one utterance's text; the rest follows as text records.  prompt_codes ([T][16], or
    one such per utterance), prompt_token_ids / prompt_text, voice: the codec prompt the utterances continue (--concurrent).
    sampler ("reference" / "upstream"), repetition_penalty, repetition_window, eos_boost, eos_force, min_tokens, cp_top_p: the
    request's sampler rules (--concurrent --sampler_rules; batch_request).  prompt_audio: (array, rate) -- a numpy int16 or float32
    array [n] or [n][channels] -- or a list of such pairs, one per utterance: the audio whose voice the utterances continue
    (--concurrent --encoder); its descriptor goes into the JSON ("max_frames": prompt_audio_max_frames) and its bytes behind
    it, so the result is JSON plus payload.  register_voice: the name the server keeps that prompt under.  logprobs: True
    asks for the log-probability of every emitted id (--concurrent --logprobs).  speaker_embedding: [hidden] floats (or one such
    per utterance), the x-vector whose row the prefix carries (--concurrent; float32 values travel exactly); speaker: "only" /
    "with_prompt" / "off" -- where a prompt_audio request's embedding comes from (--speaker_encoder; batch_request)."""
    msg = {"language": language}
    if stream:
        msg["stream"] = True
    if text_stream:
        msg["text_stream"] = True
    if token_ids is not None:
        msg["token_ids"] = [[int(t) for t in ids] for ids in token_ids]
    else:
        msg["texts"] = list(texts)
    if max_tokens:
        msg["max_tokens"] = int(max_tokens)
    if prompt_codes is not None:
        prompt_codes = np.asarray(prompt_codes).tolist() if not isinstance(prompt_codes, list) else \
            [np.asarray(c).tolist() if isinstance(c, np.ndarray) else c for c in prompt_codes]
    if prompt_token_ids is not None:
        prompt_token_ids = [int(t) for t in prompt_token_ids]
    if speaker_embedding is not None:
        a = np.asarray(speaker_embedding, dtype=np.float32)
        speaker_embedding = [float(x) for x in a] if a.ndim == 1 else [[float(x) for x in row] for row in a]
    for key, v in (("speaker_embedding", speaker_embedding), ("speaker", speaker), ("temperature", temperature), ("top_k", top_k), ("top_p", top_p), ("cp_temperature", cp_temperature),
                   ("cp_top_k", cp_top_k), ("seed", seed), ("vocoder", vocoder), ("vocoder_arithmetic", vocoder_arithmetic),
                   ("prompt_codes", prompt_codes), ("prompt_token_ids", prompt_token_ids), ("prompt_text", prompt_text),
                   ("voice", voice), ("sampler", sampler), ("repetition_penalty", repetition_penalty),
                   ("repetition_window", repetition_window), ("eos_boost", eos_boost), ("eos_force", eos_force),
                   ("min_tokens", min_tokens), ("cp_top_p", cp_top_p), ("logprobs", logprobs)):
        if v is not None:
            msg[key] = v
    payload = b""
    if prompt_audio is not None:
        shared = isinstance(prompt_audio, tuple)
        descs, parts = zip(*(prompt_audio_descriptor(a, r, prompt_audio_max_frames) for a, r in ([prompt_audio] if shared else prompt_audio)))
        msg["prompt_audio"] = descs[0] if shared else list(descs)
        payload = b"".join(parts)
    if register_voice is not None:
        msg["register_voice"] = register_voice
    raw = json.dumps(msg).encode()
    return struct.pack("<I", len(raw)) + raw + payload


def prompt_audio_descriptor(array, rate, max_frames=None):
    """A clip as a client has it (numpy int16 / float32, [n] or [n][channels]) -> (its "prompt_audio" descriptor, its bytes)"""
    a = np.asarray(array)
    fmt = {np.dtype(np.int16): "s16", np.dtype(np.float32): "f32"}.get(a.dtype)
    if fmt is None or a.ndim not in (1, 2):
        raise TypeError("prompt audio is an int16 or float32 array of shape [n] or [n][channels]")
    d = {"format": fmt, "rate": int(rate), "channels": 1 if a.ndim == 1 else int(a.shape[1]), "frames": int(a.shape[0])}
    if max_frames is not None:
        d["max_frames"] = int(max_frames)
    return d, np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("<")).tobytes()


def pack_batch_reply(results, scores=None) -> bytes:
    """scores (a "logprobs" request): one float32 [n_frames][16] per utterance, written behind its block."""
    parts = [struct.pack("<i", len(results))]
    for u, (codes, pcm) in enumerate(results):
        c = np.ascontiguousarray(codes, dtype="<i4").reshape(-1, 16)
        a = np.ascontiguousarray(pcm, dtype="<i2")
        parts += [struct.pack("<i", c.shape[0]), c.tobytes(), struct.pack("<i", a.shape[0]), a.tobytes()]
        if scores is not None:
            s = np.ascontiguousarray(scores[u], dtype="<f4").reshape(-1, 16)
            if s.shape[0] != c.shape[0]:
                raise ValueError(f"utterance {u}: {s.shape[0]} frames of log-probabilities for {c.shape[0]} frames of codes")
            parts += [struct.pack("<i", s.shape[0]), s.tobytes()]
    return b"".join(parts)


def read_batch_reply(conn, logprobs=False):
    """-> list of (codes [n][16] int32, pcm int16), with logprobs (the request asked for them) of (codes, pcm, scores [n][16]
    float32); raises on the error sentinel / a short read."""
    head = P.recv_exact(conn, 4)
    if len(head) < 4:
        raise RuntimeError("connection closed")
    (n,) = struct.unpack("<i", head)
    if n < 0:
        raise RuntimeError(f"server error ({n})")
    out = []
    for _ in range(n):
        (nf,) = struct.unpack("<i", P.recv_exact(conn, 4))
        codes = np.frombuffer(P.recv_exact(conn, nf * 16 * 4), dtype="<i4").reshape(nf, 16)
        (ns,) = struct.unpack("<i", P.recv_exact(conn, 4))
        pcm = np.frombuffer(P.recv_exact(conn, ns * 2), dtype="<i2")
        if logprobs:
            (nl,) = struct.unpack("<i", P.recv_exact(conn, 4))
            out.append((codes, pcm, np.frombuffer(P.recv_exact(conn, nl * 16 * 4), dtype="<f4").reshape(nl, 16)))
        else:
            out.append((codes, pcm))
    return out


def pack_stream_audio(utt, pcm) -> bytes:
    a = np.ascontiguousarray(pcm, dtype="<i2").reshape(-1)
    return struct.pack("<iii", REC_AUDIO, int(utt), a.shape[0]) + a.tobytes()


def pack_stream_end(utt, codes) -> bytes:
    c = np.ascontiguousarray(codes, dtype="<i4").reshape(-1, 16)
    return struct.pack("<iii", REC_END, int(utt), c.shape[0]) + c.tobytes()


def pack_stream_scores(utt, scores) -> bytes:
    s = np.ascontiguousarray(scores, dtype="<f4").reshape(-1, 16)
    return struct.pack("<iii", REC_SCORES, int(utt), s.shape[0]) + s.tobytes()


def read_stream_record(conn):
    """One record of a streamed reply -> ("audio", utt, pcm int16) / ("end", utt, codes [n][16] int32) / ("scores", utt,
    log-probabilities [n][16] float32: a "logprobs" request, right before the utterance's "end") / ("done",); raises on the
    error sentinel, an unknown record or a short read."""
    def exact(n):
        b = P.recv_exact(conn, n)
        if len(b) < n:
            raise RuntimeError("connection closed inside a streamed reply")
        return b
    (kind,) = struct.unpack("<i", exact(4))
    if kind == P.SENTINEL_DONE:
        return ("done",)
    if kind == P.SENTINEL_ERROR:
        raise RuntimeError(f"server error ({kind})")
    if kind not in (REC_AUDIO, REC_END, REC_SCORES):
        raise RuntimeError(f"unknown record {kind} in a streamed reply")
    utt, n = struct.unpack("<ii", exact(8))
    if n < 0:
        raise RuntimeError(f"record of {n} entries")
    if kind == REC_AUDIO:
        return ("audio", utt, np.frombuffer(exact(n * 2), dtype="<i2"))
    if kind == REC_SCORES:
        return ("scores", utt, np.frombuffer(exact(n * 16 * 4), dtype="<f4").reshape(n, 16))
    return ("end", utt, np.frombuffer(exact(n * 16 * 4), dtype="<i4").reshape(n, 16))


def _send_request(s, raw):
    """The request and its payload.  A server that refuses a "prompt_audio" request from its JSON answers -2 and closes without
    reading the payload: the rest of the send then fails, and the answer is still there to be read."""
    try:
        s.sendall(raw)
    except (BrokenPipeError, ConnectionResetError):
        pass


def _stream_records(s):
    """The records of a streamed reply on `s` until the request is done."""
    while True:
        rec = read_stream_record(s)
        if rec[0] == "done":
            return
        yield rec


def synthesize_batch_stream(socket_path, texts=None, token_ids=None, language="russian", max_tokens=None, vocoder=None,
                            vocoder_arithmetic=None, **sampling):
    """Client side of the streamed request: yields its records as they arrive -- ("audio", utt, pcm) and ("end", utt, codes),
    with logprobs=True also ("scores", utt, log-probabilities) right before each "end" -- until the request is done; raises
    on the error sentinel.  vocoder="incremental": the carry-state decode (audio from the
    first check on) instead of the chunk walk, vocoder_arithmetic="split": on its split-fp16 convolutions.  sampling: the optional
    keys of pack_batch_request."""
    with socket.socket(socket.AF_UNIX, socket.SOCK_STREAM) as s:
        s.connect(socket_path)
        _send_request(s, pack_batch_request(texts, token_ids, language, max_tokens, stream=True, vocoder=vocoder,
                                            vocoder_arithmetic=vocoder_arithmetic, **sampling))
        yield from _stream_records(s)


def synthesize_text_stream(socket_path, pieces, language="russian", max_tokens=None, vocoder=None, vocoder_arithmetic=None,
                           voice=None, prompt_codes=None, prompt_token_ids=None, prompt_text=None, prompt_audio=None,
                           register_voice=None, **sampling):
    """Client side of a "text_stream" request (--concurrent servers): `pieces` is an iterable of the text's pieces as they
    become available -- str / bytes (UTF-8, cut anywhere; the server tokenises) or sequences of token ids.  The first piece
    goes out with the request (it must give at least one token), the others as text records from a sender thread that walks
    the iterable, then the end-of-text record.  Yields the records of synthesize_batch_stream, utterance 0.  voice, or
    prompt_codes with prompt_token_ids / prompt_text: the codec prompt the utterance continues (--text_voice servers);
    prompt_audio=(array, rate): that prompt as audio (--encoder servers; its bytes go out before any text record), kept under
    register_voice if given."""
    it = iter(pieces)
    first = next(it)
    as_text = isinstance(first, (str, bytes, bytearray))
    if isinstance(first, (bytes, bytearray)):
        raise TypeError("the first piece goes into the JSON request: a str, or a sequence of token ids")
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.connect(socket_path)
    sender_error = []

    def sender():
        try:
            for piece in it:
                text = isinstance(piece, (str, bytes, bytearray))
                s.sendall(P.pack_text_record(P.TEXT_BYTES if text else P.TEXT_IDS, piece))
            s.sendall(P.pack_text_record(P.TEXT_END))
        except Exception as e:      # noqa: BLE001 -- the reader sees the closed connection or the server's -2
            sender_error.append(e)

    th = threading.Thread(target=sender, daemon=True)
    try:
        _send_request(s, pack_batch_request([first] if as_text else None, None if as_text else [list(first)], language, max_tokens,
                                            stream=True, vocoder=vocoder, vocoder_arithmetic=vocoder_arithmetic, text_stream=True,
                                            prompt_codes=prompt_codes, prompt_token_ids=prompt_token_ids, prompt_text=prompt_text,
                                            voice=voice, prompt_audio=prompt_audio, register_voice=register_voice, **sampling))
        th.start()
        yield from _stream_records(s)
    finally:
        s.close()
        if th.is_alive():
            th.join(timeout=5)


def synthesize_batch(socket_path, texts=None, token_ids=None, language="russian", max_tokens=None, **sampling):
    """Client side of the batched request.  sampling: the optional keys of pack_batch_request (vocoder and vocoder_arithmetic
    among them; prompt_audio=(array, rate) and register_voice too -- with texts=[] the request only registers: -> []).
    logprobs=True: -> (codes, pcm, log-probabilities [n][16] float32) per utterance."""
    with socket.socket(socket.AF_UNIX, socket.SOCK_STREAM) as s:
        s.connect(socket_path)
        _send_request(s, pack_batch_request(texts, token_ids, language, max_tokens, **sampling))
        return read_batch_reply(s, logprobs=bool(sampling.get("logprobs")))
