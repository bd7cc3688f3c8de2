#!/usr/bin/env python3
"""Batched synthesis server: B utterances per request through the on-device frame loop.

The reference closes the autoregressive loop in its client, two socket round trips per frame and one
utterance at a time (dual_npu/tts_client.py:144-215; `listen(1)`, llamacpp_talker_server.py:314).  This
server keeps that front-end (tokenizer, text projection, dual-stream prefix: llamacpp_talker_server.py:
115-161; EOS heuristics and sampling on the device) and runs the whole loop for all utterances of a request
on the GPU (include/qwen3tts_engine.h), then the vocoder's chunk walk (vocoder_server.py:73-121, :175) per
utterance.  Extension of the wire protocol, same conventions (little-endian, u32 length + UTF-8 JSON):

    request   u32 len + JSON {"texts": [...], "language": "...", "max_tokens": N}   or {"token_ids": [[...], ...]}
    reply     i32 n_utterances (or -2 on error), then per utterance:
              i32 n_frames, i32[n_frames*16] codes, i32 n_samples, i16[n_samples] PCM (24 kHz)

One process per GPU (HIP_VISIBLE_DEVICES), like the other servers.

Streamed reply (the request carries "stream": true): the same synthesis, handed out while the frame loop runs, as records on
the same connection (in the order they are ready; `utt` indexes the request's utterances):

              i32 1, i32 utt, i32 n, i16[n]                  PCM of utterance utt: the next n samples
              i32 2, i32 utt, i32 n_frames, i32[n_frames*16]  utterance utt has ended: all its codes
              i32 -1                                          the request is done   (i32 -2: error, as above)

A request may carry "vocoder": "incremental" (default "walk"; any other value is answered with -2): its PCM then comes from the
carry-state incremental decode (voc_incr_push: the samples of every check's new frames at once, one seamless decode per
utterance) instead of the chunk walk -- streamed, or unstreamed through Vocoder.synthesize_incremental, the same bits either way.
Such a request may also carry "vocoder_arithmetic": "exact" (the default) or "split" (the split-fp16 convolutions,
voc_incr_set_arithmetic); any other value, or the key on a request that is not "vocoder": "incremental", is answered with -2.
Records, framing and the single-writer worker are the same.
Every check_every frames the new frames of every live slot go to the vocoder's streaming chunk walk (voc_stream_push, on one
worker thread with one vocoder workgroup per compute unit, as in --pipeline); a full 64-frame chunk is decoded as soon as its
frames exist, and all samples no later cross-fade can change go out at once.  An utterance's PCM records joined, and its codes,
are bit for bit what the unstreamed reply carries.

`--concurrent`: utterances of different requests share ONE running frame loop.  An accept thread reads and checks every
request (a malformed one, or one that would take the queue past max_queue utterances, gets -2 at once) and queues its
utterances; the engine thread -- the only caller of the engine -- opens max_batch slots once (q3e_open) and every check_every
frames admits queued utterances into free slots (FIFO across requests; within a request longest first, as above), each with
its own frame budget (the request's max_tokens), sampling settings and seed (q3e_admit), runs the loop, polls which slots
ended, and releases the slots of a client that went away; one vocoder worker -- the only caller of the vocoder -- streams the
new frames of streamed requests (one voc_stream per slot, reset on admission) and answers an unstreamed request with one
voc_synthesize_batch over its utterances once its last one ended.  Requests may carry the keys "temperature", "top_k", "top_p",
"cp_temperature", "cp_top_k" and "seed" (a missing key takes the server's value; the other modes keep the server's settings
and ignore them).  Determinism contract: a request's reply, codes and PCM, depends only on the request, its seed and the
server's configuration -- not on what else is in flight nor on which slots it gets.  The loop always steps max_batch rows (a
row's f32 sums depend on the row count of the pass), every utterance is prefilled in a pass of its own (the ragged prefill's
tiles depend on the rows of the pass), and utterance u of a request with seed s draws from the stream mix(s, u), keyed by
(stream, frame, group) and not by the slot (include/qwen3tts_engine.h).  With `--prefix_cache N` a reply is, bit for bit, the
reply without it.

`--prefix_cache N` (with `--concurrent`; N entries of up to `--prefix_cache_rows` prefix rows each, default 0 = off): the
engine keeps the KV rows and the frame-0 state of admitted prefixes in a device pool (q3e_prefix_cache / q3e_admit_keyed), and
an utterance whose prefix is there is admitted by one copy launch instead of a prefill: a repeated text, the k takes of a
request that lists one text k times with a seed, and every text-stream request that begins with the same token (its 8-row
streaming prefix depends on the first token alone).  The key is the server's own: the first 16 bytes of a SHA-256 over a kind
tag (b"full" / b"stream") and the int32 token ids that determine the prefix rows (prefix_key); a client never supplies one.
The prefix rows are still built on the accept thread; the wire protocol is unchanged.

Streamed TEXT (`--concurrent` only; the request carries "text_stream": true, which needs "stream": true and exactly one
utterance, else -2): the request's texts / token_ids hold only the first piece of the text (at least one token), and the
client goes on sending the rest on the same connection, as records

              i32 1, i32 n, n UTF-8 bytes (cut anywhere)      more text, tokenised by the server's incremental tokeniser
              i32 2, i32 n, i32[n]                             more token ids
              i32 0, i32 0                                     end of text

while the audio records already come back.  The utterance runs in a text slot of the frame loop (include/qwen3tts_engine.h,
q3e_push_text): its prefix holds the first token, every later token is projected (one token per call, so a row does not
depend on how the text was cut) and added to the feedback of one frame, the tts_eos row follows the last token.  Before each
check the engine thread reads, without blocking, what has arrived and pushes the rows.  A slot never runs ahead of its text,
and a starved slot stalls the WHOLE batch: when a check runs no frame because a text slot waits for a row, the engine thread
polls the starving requests' connections for at most --text_wait_ms (default 200); a client that stays connected but does not
send its text in that time fails its own request (-2, its slot is released) -- the rule a client that stops reading already
gets from --send_timeout.  The reply's codes and PCM depend on the text and not on how it was cut or when it arrived.  The
text may not have more tokens than the request's max_tokens (a row per frame).

`--text_hold` (with `--concurrent`): a starved text slot is HELD inside the frame (q3e_text_hold) and every other slot steps
on, so a text client that pauses costs the other requests no time -- their replies did not depend on the traffic, now their
timing does not either.  A held row still computes (it repeats its previous step onto itself), so held steps are frame-loop
throughput the others do not get back.  A text-stream request is then admitted once its first row is there (a second token,
or the end record), waiting in the queue like any queued request until then; a request whose slot has been held for
--text_wait_ms with no byte from its client fails alone (-2, its slot is released), and the others see nothing of it.

Codec prompts (`--concurrent` only): a request may carry "prompt_codes" -- one [T][16] list of codec ids shared by its
utterances, or a list of one such list per utterance -- and every utterance then CONTINUES that audio: the frames count as
frames it has already emitted (include/qwen3tts_engine.h, q3e_admit_prompted), and the reply holds the generated frames
and their audio only.  "prompt_token_ids" / "prompt_text" (optional) is the text spoken in the prompt: it is put in front
of each utterance's text ids, and the EOS heuristics count both.  `--voice NAME=DIR` (repeatable; DIR as
encode_reference_audio --output_dir writes it: ref_codec_tokens.npy and, if there, ref_text.txt) names such a pair, and a
request's "voice": "NAME" stands for the same two keys.  With "vocoder": "incremental" the prompt's frames are pushed into
the utterance's stream first and their voc_incr_samples(T) samples dropped, so the audio continues the prompt seamlessly;
the chunk walk (the default) decodes the generated frames on their own.  A prompt in any other mode, together with
"text_stream" (without `--text_voice`, below), an unknown voice, malformed codes, or one that does not fit n_ctx is answered with -2 for that request alone,
before any of it is queued.  Prompt text in front of the target text is a recollection of the model's in-context mode:
parity with real weights is not pinned.  With `--prefix_cache` the key of a prompted utterance is of the kind b"prompt" and
digests the ids and the prompt's codes.

`--text_voice` (with `--concurrent`): a "text_stream" request may carry a codec prompt -- "voice", or "prompt_codes" with an
optional "prompt_token_ids" / "prompt_text" -- and its audio then continues the prompt while its text still arrives: streamed
text in a cloned voice.  The checks are the codec prompt's, and 8 + the prompt text's tokens + T + max_tokens must fit n_ctx.
The utterance runs in a text slot that continues a prompt (q3e_slot_params.reserved == 3): its prefix is rows 0..6 of the
streaming prefix, one `text + codec_pad` row per token of the prompt's text, then the first token + codec_bos
(build_prefix_stream(first, head)); the prompt's T frames follow as they do for any prompted utterance; and row i of the
streamed text rides on GENERATED frame i.  Its text length for the EOS heuristics counts the prompt's text, as the unstreamed
prompted request of the same texts does, and its prefix key is prefix_key(b"stream", prompt text ids + first token, codes).
The vocoder follows the streamed reply of a prompted request: "incremental" warms the utterance's stream up with the prompt's
frames and drops their samples, the chunk walk decodes the generated frames alone.  `--text_hold`, `--text_wait_ms` and
`--prefix_cache` work as they do for any text-stream request; the wire protocol has no new record.  Like both of its halves
the layout is a recollection of the model's in-context mode: parity with real weights is not pinned.  Without the flag such a
request is answered -2, as before.

`--voice_warm N` (with `--concurrent`; default 0 = off): the incremental vocoder's warm-up per codec prompt is cached.  The
state a stream carries after the prompt's T frames is a function of the frames and the arithmetic alone, so the server keeps it
in N snapshot slots of its vocoder handle (voc_incr_snapshots; voice_warm.VoiceWarmCache is the LRU over them, keyed by a digest
of the prompt's ids and T and by the arithmetic -- a named voice and the same codes sent inline share an entry).  A miss warms
the stream up as before and saves it; a hit pushes no prompt frame: all hits of one check go into one voc_incr_restore, and an
unstreamed reply starts from the slot (synthesize_incremental(start_slot=)).  Several slots admitted together with the same new
voice: the first is the miss, the rest hit.  Every reply -- codes and PCM, streamed and not, both arithmetics as long as no
push is redone exactly -- is bit for bit the reply without the flag; requests without a prompt, or not "incremental", touch
nothing.  The counters voice_warm_hits / voice_warm_misses / voice_warm_evictions are on the server object, hits and misses in the
per-request line.  Only the vocoder worker touches the cache.

`--pipeline`: the vocoder of request k runs on a worker thread (and replies on k's connection) while the frame loop of request
k + 1 already runs -- the reference's client does the same per 64-frame block of ONE utterance (tts_client.py:188-197).  The
vocoder then launches one persistent workgroup per compute unit (voc_set_max_workgroups(-1)), which leaves the frame loop's
workgroups room beside it (244 -> 209 ms per 32 x 64-frame step); results are bit-identical.
"""
from __future__ import annotations

import argparse
import collections
import dataclasses
import hashlib
import os
import select
import signal
import socket
import struct
import threading
import time

import numpy as np

from . import hiplib
from . import protocol as P
from .engine import FrameEngine, SlotParams
from .frontend import TextFrontEnd
from .vocoder import Vocoder
from .voice_warm import VoiceWarmCache
from .weights import ModelConfig, read_pack


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


class QueuedUtterance(tuple):
    """An utterance as _prepare queues it -- the tuple (request index, prefix, n_text, SlotParams[, TextFeed]) the scheduler
    has always taken -- with the prefix cache's key of its prefix, and its codec prompt ([T][16] int32, or None), beside it."""
    prefix_key = None
    prompt = None

    def __new__(cls, fields, prefix_key=None, prompt=None):
        self = super().__new__(cls, fields)
        self.prefix_key = prefix_key
        self.prompt = prompt
        return self


class BatchSynthesisServer:
    def __init__(self, model_path, vocoder_path, socket_path="/tmp/qwen3_batch.sock", max_batch=32, n_ctx=512,
                 max_tokens=200, temperature=0.0, top_k=50, cp_temperature=0.0, tokenizer=None, seed=0,
                 install_signal_handlers=True, max_request=None, pipeline=False, concurrent=False, max_queue=None, top_p=0.95,
                 cp_top_k=None, check_every=8, send_timeout=30.0, text_wait_ms=200.0, text_hold=False, prefix_cache=0,
                 prefix_cache_rows=64, voices=None, text_voice=False, voice_warm=0):
        if concurrent and pipeline:
            raise ValueError("--concurrent runs its own vocoder worker: it does not combine with --pipeline")
        self.socket_path, self.max_batch, self.max_tokens = socket_path, max_batch, max_tokens
        cp_top_k = top_k if cp_top_k is None else cp_top_k
        # the settings a request of --concurrent inherits for every key it leaves out
        self.defaults = SlotParams(max_frames=max_tokens, temperature=float(temperature), top_k=int(top_k), top_p=float(top_p),
                                   cp_temperature=float(cp_temperature), cp_top_k=int(cp_top_k), seed=int(seed))
        self.defaults.check(max_tokens)
        self.concurrent = bool(concurrent)
        self.max_queue = int(max_queue) if max_queue else 16 * max_batch
        self.check_every = int(check_every)
        self.send_timeout = float(send_timeout)
        self.text_wait_ms = float(text_wait_ms)
        if text_hold and not concurrent:
            raise ValueError("--text_hold holds text slots of the shared frame loop: it needs --concurrent")
        self.text_hold = bool(text_hold)
        if int(prefix_cache) < 0 or int(prefix_cache_rows) <= 0:
            raise ValueError("--prefix_cache takes a number of entries >= 0, --prefix_cache_rows a number of rows >= 1")
        if prefix_cache and not concurrent:
            raise ValueError("--prefix_cache serves the per-slot admissions of the shared frame loop: it needs --concurrent")
        self.prefix_cache, self.prefix_cache_rows = int(prefix_cache), int(prefix_cache_rows)
        if voices and not concurrent:
            raise ValueError("--voice names codec prompts of the shared frame loop's admissions: it needs --concurrent")
        self.voices = {name: load_voice(d) for name, d in dict(voices or {}).items()}   # name -> (codes [T][16], text or None)
        if text_voice and not concurrent:
            raise ValueError("--text_voice lets text slots of the shared frame loop continue a codec prompt: it needs --concurrent")
        self.text_voice = bool(text_voice)
        if int(voice_warm) < 0:
            raise ValueError("--voice_warm takes a number of snapshot slots >= 0")
        if voice_warm and not concurrent:
            raise ValueError("--voice_warm caches the vocoder warm-up of the shared frame loop's codec prompts: it needs --concurrent")
        self.sched = None
        # utterances one request may queue (the server is single-threaded: an unbounded request holds it indefinitely)
        self.max_request = int(max_request) if max_request else 8 * max_batch
        meta, t = read_pack(model_path)
        self.cfg = ModelConfig.from_meta(meta)
        f32 = lambda n: np.asarray(t[n], dtype=np.float32)
        self.front = TextFrontEnd(self.cfg, t["text.embedding"], f32("text.fc1.weight"), f32("text.fc1.bias"),
                                  f32("text.fc2.weight"), f32("text.fc2.bias"), f32("talker.codec_embedding"))
        self.tokenizer = None
        if tokenizer:
            from .tokenizer import ByteLevelBPE
            self.tokenizer = ByteLevelBPE.from_dir(tokenizer)
        self.eng = FrameEngine(model_path, max_batch=max_batch, n_ctx=n_ctx, max_frames=max_tokens)
        self.eng.set_pad_embed(self.front.tts_pad_embed)
        self.eng.set_sampling(temperature, top_k, top_p, cp_temperature, cp_top_k, seed)
        self.n_ctx = n_ctx
        self._lib = hiplib.load()
        self.voc = Vocoder(vocoder_path, 64, min(max_batch, 32))
        # --voice_warm N: N snapshot slots on the vocoder handle, and the LRU over them (the vocoder worker's, like the handle)
        self._voice_warm = VoiceWarmCache(int(voice_warm))
        if self._voice_warm.n_slots:
            self.voc.snapshots(self._voice_warm.n_slots)
        self.pipeline = bool(pipeline)
        self._pool = None
        self._stream_pool = None       # the push worker of streamed requests (the pipeline's worker when there is one)
        self._vstream = None           # streaming chunk walk: one stream per slot of the frame loop
        self._istreams = {}            # carry-state incremental decode ("vocoder": "incremental"): one object per arithmetic,
                                       # made by the worker on first use
        if self.pipeline:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=1)       # ONE worker: the vocoder handle has one caller, replies keep their order
            self._lib.voc_set_max_workgroups(-1)
        self._running = True
        if install_signal_handlers:
            signal.signal(signal.SIGINT, self._signal_handler)
            signal.signal(signal.SIGTERM, self._signal_handler)

    def _signal_handler(self, signum, frame):
        self._running = False

    def _token_ids(self, msg):
        if msg.get("token_ids") is not None:
            return [[int(x) for x in ids] for ids in msg["token_ids"]]
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer configured (--tokenizer DIR) and the request has no token_ids")
        return [self.tokenizer.encode(t, add_special_tokens=False) for t in msg.get("texts", [])]

    def _queue(self, token_ids, max_tokens):
        """A request's prefixes -> (prefixes, n_text, max_tokens, order): order[k] = request index of the queue's k-th utterance."""
        B = len(token_ids)
        if B == 0:
            raise ValueError("a request needs at least one utterance")
        if B > self.max_request:
            raise ValueError(f"a request may carry at most {self.max_request} utterances (got {B})")
        max_tokens = min(int(max_tokens or self.max_tokens), self.max_tokens)
        prefixes = [self.front.build_prefix(ids) for ids in token_ids]
        if max(p.shape[0] for p in prefixes) + max_tokens > self.n_ctx:
            raise ValueError("prefix + max_tokens exceed n_ctx")
        n_text = [len(ids) for ids in token_ids]
        # more utterances than slots: continuous batching -- a finished utterance's slot takes the next one of the request
        # (q3e_refill), longest expected first (3 frames per text token, llamacpp_talker_server.py:174)
        order = sorted(range(B), key=lambda i: -n_text[i]) if B > self.max_batch else list(range(B))
        return prefixes, n_text, max_tokens, order

    def generate(self, token_ids, max_tokens=None):
        """The frame loop of a request -> list of codes int32 [n_frames][16] per utterance."""
        prefixes, n_text, max_tokens, order = self._queue(token_ids, max_tokens)
        B = len(token_ids)
        if B > self.max_batch:
            got = self.eng.generate_queue([prefixes[i] for i in order], [n_text[i] for i in order], max_tokens)
            per_utt = [None] * B
            for k, i in enumerate(order):
                per_utt[i] = got[k]
        else:
            self.eng.start(prefixes, n_text, ignore_eos=False, max_frames=max_tokens)
            self.eng.run(max_tokens)
            codes, per = self.eng.codes()
            per_utt = [codes[:int(per[b]), b, :] for b in range(B)]
        return [np.ascontiguousarray(c, dtype=np.int32) for c in per_utt]

    def vocode(self, cs, vocoder="walk", arithmetic="exact", prompts=None):
        """The vocoder of a request: every utterance's chunk walk in ONE batched call -> list of (codes, pcm int16).
        vocoder="incremental": the carry-state decode per utterance, in the request's arithmetic -- the bits a streamed reply in
        that mode carries.  prompts (one [T][16] array or None per utterance): the incremental decode runs over the prompt's
        frames and the utterance's, and the prompt's voc_incr_samples(T) samples are dropped; the chunk walk decodes the
        generated frames on their own."""
        if vocoder == "incremental":
            out = []
            for u, c in enumerate(cs):
                pr = prompts[u] if prompts is not None else None
                if pr is None or not len(pr):
                    out.append((c, self.voc.synthesize_incremental(c, int16=True, arithmetic=arithmetic)))
                    continue
                if self._voice_warm.n_slots:
                    # the prompt's state from the voice's snapshot (decoded and saved first on a miss), then the utterance alone
                    slot = self._voice_warm.slot_of(self.voc.incremental_one(arithmetic), arithmetic,
                                                    np.asarray(pr, np.int32).reshape(-1, 16), self.voc.chunk_tokens,
                                                    self.voc.incremental_samples)
                    out.append((c, self.voc.synthesize_incremental(c, int16=True, arithmetic=arithmetic, start_slot=slot)))
                    continue
                both = np.concatenate([np.asarray(pr, np.int32).reshape(-1, 16), np.asarray(c, np.int32).reshape(-1, 16)])
                pcm = self.voc.synthesize_incremental(both, int16=True, arithmetic=arithmetic)
                out.append((c, pcm[self.voc.incremental_samples(len(pr)):]))
            return out
        return list(zip(cs, self.voc.synthesize_batch(cs)))

    def synthesize(self, token_ids, max_tokens=None, vocoder="walk", arithmetic="exact"):
        """-> list of (codes int32 [n_frames][16], pcm int16) per utterance."""
        return self.vocode(self.generate(token_ids, max_tokens), vocoder, arithmetic)

    def _stream_pcm(self, state, resets, entries):
        """Worker side: the PCM a push's entries hand out, from the request's vocoder mode -- the streaming chunk walk, or the
        carry-state decode, which takes at most chunk_tokens frames per stream and call."""
        if state.get("vocoder", "walk") != "incremental":
            for b in resets:
                self._vstream.reset(b)
            return self._vstream.push([e[0] for e in entries], [e[2] for e in entries], [e[3] for e in entries]) if entries else []
        arithmetic = state.get("vocoder_arithmetic", "exact")
        if arithmetic not in self._istreams:
            self._istreams[arithmetic] = self.voc.incremental(self.max_batch, arithmetic)
        istream = self._istreams[arithmetic]
        ch = self.voc.chunk_tokens
        drop = state.setdefault("drop", {})    # samples of a slot's prompt that are still to be dropped from what it hands out
        for b in resets:
            drop.pop(b, None)
        # a slot that continues a prompt: the prompt's frames first, in pieces of at most chunk_tokens frames, none of their
        # samples going out -- or, with --voice_warm, the state those pushes leave, copied from the voice's snapshot
        prompts = {b: state.get("prompts", {}).pop(b, None) for b in resets}
        drop.update(self._voice_warm.start(istream, arithmetic, resets, prompts, ch, self.voc.incremental_samples))
        parts, j = [[] for _ in entries], 0
        while entries and (j == 0 or any(len(e[2]) > j * ch for e in entries)):
            sel = [k for k, e in enumerate(entries) if j == 0 or len(e[2]) > j * ch]
            pcm = istream.push([entries[k][0] for k in sel], [entries[k][2][j * ch:(j + 1) * ch] for k in sel],
                                     [entries[k][3] and len(entries[k][2]) <= (j + 1) * ch for k in sel])
            for k, a in zip(sel, pcm):
                parts[k].append(a.copy())
            j += 1
        out = [np.concatenate(p) for p in parts]
        for k, e in enumerate(entries):
            left = drop.get(e[0], 0)
            if left > 0:
                drop[e[0]] = left - min(left, len(out[k]))
                out[k] = out[k][left:]
        return out

    def _push(self, conn, state, resets, entries):
        """Worker side of a streamed request: start the refilled slots' streams, push every live slot's new frames to the
        streaming chunk walk, send the PCM that became final and the end records.  entries: (slot, utt, new frames,
        finished, all codes of the utterance when finished)."""
        if state["failed"]:
            return
        try:
            pcm = self._stream_pcm(state, resets, entries)
            if entries:
                out = []
                for k, (_, utt, _, finished, codes) in enumerate(entries):
                    if len(pcm[k]):
                        out.append(pack_stream_audio(utt, pcm[k]))
                    if finished:
                        out.append(pack_stream_end(utt, codes))
                if out:
                    conn.sendall(b"".join(out))
        except Exception as e:
            state["failed"] = True
            print(f"Error: {e}")
            try:
                conn.sendall(P.pack_sentinel(P.SENTINEL_ERROR))
            except OSError:
                pass

    def _close_stream(self, conn, state, t0):
        """Worker side: the last record of a streamed request, then its connection closes."""
        try:
            if not state["failed"]:
                conn.sendall(P.pack_sentinel(P.SENTINEL_DONE))
                print(f"  {state['n']} utterances, {state['frames']} frames streamed in {time.time() - t0:.3f}s{self._prefix_note()}")
        except OSError:
            pass
        finally:
            conn.close()

    def synthesize_stream(self, conn, token_ids, max_tokens=None, t0=None, vocoder="walk", arithmetic="exact"):
        """A streamed request: the frame loop runs here (generate_queue), the vocoder's pushes and every write to `conn` on the
        worker thread, at most one push in flight.  -> the worker's future of the request's last record (it closes conn)."""
        t0 = time.time() if t0 is None else t0
        state = {"failed": False, "n": len(token_ids), "frames": 0, "vocoder": vocoder, "vocoder_arithmetic": arithmetic}
        if self._pool is not None:
            pool = self._pool
        else:
            if self._stream_pool is None:
                from concurrent.futures import ThreadPoolExecutor
                self._stream_pool = ThreadPoolExecutor(max_workers=1)
            pool = self._stream_pool
        fut = None
        try:
            prefixes, n_text, max_tokens, order = self._queue(token_ids, max_tokens)
            if self._vstream is None:
                self._vstream = self.voc.stream(self.max_batch)
            if self._pool is None:
                self._lib.voc_set_max_workgroups(-1)     # the pushes run beside the frame loop (restored when the request ends)
            slot_utt = [None] * self.max_batch           # queue index each slot's stream holds
            pushed = [0] * self.max_batch

            def on_frames(codes, per, owner, ended):
                nonlocal fut
                resets, entries = [], []
                for b, o in enumerate(owner):
                    if o is None:
                        continue
                    if slot_utt[b] != o:
                        slot_utt[b], pushed[b] = o, 0
                        resets.append(b)
                    n, fin = int(per[b]), b in ended
                    if n > pushed[b] or fin:
                        new = np.ascontiguousarray(codes[pushed[b]:n, b, :])
                        whole = np.ascontiguousarray(codes[:n, b, :], dtype=np.int32) if fin else None
                        entries.append((b, order[o], new, fin, whole))
                        pushed[b] = n
                        if fin:
                            state["frames"] += n
                if not (resets or entries):
                    return
                if fut is not None:
                    fut.result()                         # one push in flight
                if state["failed"]:
                    raise RuntimeError("streamed request failed on the vocoder side")
                fut = pool.submit(self._push, conn, state, resets, entries)

            self.eng.generate_queue([prefixes[i] for i in order], [n_text[i] for i in order], max_tokens, on_frames=on_frames)
        except Exception as e:
            if fut is not None:
                fut.result()
            if not state["failed"]:
                print(f"Error: {e}")
                state["failed"] = True
                pool.submit(self._send_error, conn)
        finally:
            if fut is not None:
                fut.result()
            last = pool.submit(self._close_stream, conn, state, t0)
            if self._pool is None:
                last.result()
                self._lib.voc_set_max_workgroups(0)
        return last

    @staticmethod
    def _send_error(conn):
        try:
            conn.sendall(P.pack_sentinel(P.SENTINEL_ERROR))
        except OSError:
            pass

    def _prepare(self, msg):
        """--concurrent, accept side: a request -> its utterances in queue order as (request index, prefix, n_text,
        SlotParams), each a QueuedUtterance with its prefix key; raises on anything malformed, before any of it is queued."""
        request_vocoder_arithmetic(msg)      # (checks "vocoder" too)
        base = request_slot_params(msg, self.defaults, self.max_tokens)
        if msg.get("text_stream"):
            if request_has_prompt(msg) and not getattr(self, "text_voice", False):
                raise ValueError('a codec prompt does not combine with "text_stream"')
            return [self._prepare_text_stream(msg, base)]
        ids = self._token_ids(msg)
        if not request_has_prompt(msg):
            prefixes, n_text, max_tokens, order = self._queue(ids, base.max_frames)
            return [QueuedUtterance((i, prefixes[i], n_text[i], dataclasses.replace(base, max_frames=max_tokens, utt=i)),
                                    prefix_key(b"full", ids[i])) for i in order]
        # a codec prompt: its text (if any) in front of every utterance's, its frames behind every prefix
        prompts, head = self._request_prompts(msg, len(ids))
        ids = [head + u for u in ids]
        prefixes, n_text, max_tokens, order = self._queue(ids, base.max_frames)
        for i in order:
            rows = prefixes[i].shape[0] + len(prompts[i])
            if rows + max_tokens > self.n_ctx or rows > max(self.max_batch, 2048):
                raise ValueError("prefix + codec prompt + max_tokens exceed n_ctx (or the rows of one prefill pass)")
        return [QueuedUtterance((i, prefixes[i], n_text[i], dataclasses.replace(base, max_frames=max_tokens, utt=i)),
                                prefix_key(b"prompt", ids[i], prompts[i]) if len(prompts[i]) else prefix_key(b"full", ids[i]),
                                prompts[i] if len(prompts[i]) else None) for i in order]

    def _request_prompts(self, msg, n_utts):
        """A request's codec prompt -> (one [T][16] int32 array per utterance, the prompt text's token ids): from
        "prompt_codes" and "prompt_token_ids" / "prompt_text", or from the "voice" that names them; raises ValueError on
        anything malformed."""
        if msg.get("text_stream") and not getattr(self, "text_voice", False):
            raise ValueError('a codec prompt does not combine with "text_stream"')
        codes, text, head = msg.get("prompt_codes"), msg.get("prompt_text"), msg.get("prompt_token_ids")
        if msg.get("voice") is not None:
            if codes is not None or text is not None or head is not None:
                raise ValueError('"voice" stands for "prompt_codes" and the prompt text: give one or the other')
            name = msg["voice"]
            if not isinstance(name, str) or name not in self.voices:
                raise ValueError(f"unknown voice {name!r}")
            codes, text = self.voices[name]
        if codes is None:
            raise ValueError('a prompt text needs "prompt_codes" (or a "voice")')
        if head is not None and text is not None:
            raise ValueError('"prompt_token_ids" and "prompt_text" are the same thing: give one')
        if head is not None:
            if not isinstance(head, list) or any(isinstance(t, bool) or not isinstance(t, int) for t in head):
                raise ValueError('"prompt_token_ids" is a list of integers')
        elif text is not None:
            if not isinstance(text, str):
                raise ValueError('"prompt_text" is a string')
            if self.tokenizer is None:
                raise RuntimeError("no tokenizer configured (--tokenizer DIR) for the prompt's text")
            head = self.tokenizer.encode(text, add_special_tokens=False)
        return request_prompt_codes(codes, n_utts, self.cfg.cp_vocab), [int(t) for t in (head or [])]

    def _prepare_text_stream(self, msg, base):
        """A "text_stream" request -> its one utterance as (0, streaming prefix, 0, SlotParams of a text slot, TextFeed), a
        QueuedUtterance whose prefix key covers the first token alone.  With a codec prompt (--text_voice): the prefix holds
        the prompt's text in front of the first token (build_prefix_stream(first, head)), the utterance carries the prompt,
        its SlotParams ask for text after a prompt, its text length counts the prompt's text, and the key covers the prompt's
        text, the first token and the prompt's codes."""
        from .frontend import text_stream_rows
        if msg.get("stream") is not True:
            raise ValueError('"text_stream" needs "stream": true')
        by_ids = msg.get("token_ids") is not None
        pieces = msg["token_ids"] if by_ids else msg.get("texts", [])
        if not isinstance(pieces, list) or len(pieces) != 1:
            raise ValueError('a "text_stream" request carries exactly one utterance')
        encoder = None
        if by_ids:
            first = [int(x) for x in pieces[0]]
        else:
            if self.tokenizer is None:
                raise RuntimeError("no tokenizer configured (--tokenizer DIR) and the request has no token_ids")
            encoder = self.tokenizer.incremental()
            first = encoder.feed(pieces[0])
        if not first:
            raise ValueError('the first piece of a "text_stream" request must give at least one token')
        prompt, head = None, []
        if request_has_prompt(msg):
            prompts, head = self._request_prompts(msg, 1)
            prompt = prompts[0]
            rows = 8 + len(head) + len(prompt)
            if rows + base.max_frames > self.n_ctx or rows > max(self.max_batch, 2048):
                raise ValueError("prefix + codec prompt + max_tokens exceed n_ctx (or the rows of one prefill pass)")
        if 8 + base.max_frames > self.n_ctx:
            raise ValueError("prefix + max_tokens exceed n_ctx")
        tokeniser = self.tokenizer
        feed = TextFeed(lambda ids, final=False: text_stream_rows(self.front, ids, final), encoder,
                        None if tokeniser is None else tokeniser.incremental, first[1:], 1 + len(head))
        if prompt is None:
            params = dataclasses.replace(base, utt=0, text_stream=True)
            return QueuedUtterance((0, self.front.build_prefix_stream(first[0]), 0, params, feed), prefix_key(b"stream", first[:1]))
        params = dataclasses.replace(base, utt=0, text_stream=True, text_after_prompt=True)
        return QueuedUtterance((0, self.front.build_prefix_stream(first[0], head), 0, params, feed),
                               prefix_key(b"stream", head + first[:1], prompt), prompt if len(prompt) else None)

    def _prefix_note(self):
        """The prefix cache's and the voice warm-ups' counters so far, for the per-request line ("" without the flags)."""
        note = ""
        if self.prefix_cache and self.sched is not None:
            note = f" (prefix cache: {self.sched.prefix_hits} hits, {self.sched.prefix_misses} misses so far)"
        return note + self._voice_warm.note()

    voice_warm_hits = property(lambda self: self._voice_warm.hits)
    voice_warm_misses = property(lambda self: self._voice_warm.misses)
    voice_warm_evictions = property(lambda self: self._voice_warm.evictions)

    def _finish(self, conn, cs, t0, vocoder="walk", arithmetic="exact", prompts=None):
        """Worker side of the pipelined mode: vocode, reply on the request's own connection, close it."""
        try:
            res = self.vocode(cs, vocoder, arithmetic, prompts)
            conn.sendall(pack_batch_reply(res))
            print(f"  {len(res)} utterances, {sum(len(c) for c, _ in res)} frames in {time.time() - t0:.3f}s{self._prefix_note()}")
        except Exception as e:
            print(f"Error: {e}")
            try:
                conn.sendall(P.pack_sentinel(P.SENTINEL_ERROR))
            except OSError:
                pass
        finally:
            conn.close()

    def serve(self):
        if os.path.exists(self.socket_path):
            os.unlink(self.socket_path)
        sock = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        sock.bind(self.socket_path)
        sock.listen(128 if self.concurrent else 1)
        sock.settimeout(1.0)
        os.chmod(self.socket_path, 0o666)
        if self.concurrent:
            self._serve_concurrent(sock)
            return
        print(f"Batch synthesis server listening on {self.socket_path} ({self.max_batch} slots; longer requests run through them by continuous batching)")
        while self._running:
            try:
                conn, _ = sock.accept()
            except socket.timeout:
                continue
            except OSError:
                break
            handed_over = False
            try:
                msg = P.read_talker_request(conn)
                if msg is None:
                    continue
                t0 = time.time()
                vocoder, arithmetic = request_vocoder(msg), request_vocoder_arithmetic(msg)
                if msg.get("text_stream"):
                    raise ValueError('"text_stream" needs a --concurrent server')
                if request_has_prompt(msg):
                    raise ValueError("a codec prompt needs a --concurrent server")
                if msg.get("stream"):
                    # streamed reply: the worker writes every record and closes the connection
                    ids = self._token_ids(msg)
                    handed_over = True
                    self.synthesize_stream(conn, ids, msg.get("max_tokens"), t0, vocoder, arithmetic)
                    continue
                if self._pool is not None:
                    # pipelined: this request's vocoder runs on the worker while the loop accepts and generates the next one
                    cs = self.generate(self._token_ids(msg), msg.get("max_tokens"))
                    self._pool.submit(self._finish, conn, cs, t0, vocoder, arithmetic)
                    handed_over = True
                    continue
                res = self.synthesize(self._token_ids(msg), msg.get("max_tokens"), vocoder, arithmetic)
                conn.sendall(pack_batch_reply(res))
                frames = sum(len(c) for c, _ in res)
                print(f"  {len(res)} utterances, {frames} frames in {time.time() - t0:.3f}s")
            except Exception as e:  # like the reference's servers: report, send the error sentinel, keep serving
                print(f"Error: {e}")
                try:
                    conn.sendall(P.pack_sentinel(P.SENTINEL_ERROR))
                except OSError:
                    pass
            finally:
                if not handed_over:
                    conn.close()
        for pool in (self._pool, self._stream_pool):
            if pool is not None:
                pool.shutdown(wait=True)         # replies in flight go out before the socket disappears
        self._pool = self._stream_pool = None
        sock.close()
        if os.path.exists(self.socket_path):
            os.unlink(self.socket_path)

    def _serve_concurrent(self, sock):
        """--concurrent: this thread accepts and checks requests; the scheduler's engine thread and vocoder worker do the rest."""
        if self._vstream is None:
            self._vstream = self.voc.stream(self.max_batch)
        self._lib.voc_set_max_workgroups(-1)     # the vocoder runs beside the frame loop: one workgroup per CU
        self.eng.reserve_text(self.max_tokens)   # before the scheduler opens the batch: a row per frame of every slot
        if self.text_hold:
            self.eng.hold_text()                 # a text slot without a row is held inside the frame: the others step on
        if self.prefix_cache:
            self.eng.prefix_cache(self.prefix_cache, self.prefix_cache_rows)
        self.sched = ConcurrentScheduler(self.eng, self.max_batch, self.max_queue, self._prepare, self._finish, self._push,
                                         self._close_stream, self._send_error, check_every=self.check_every,
                                         send_timeout=self.send_timeout, text_wait_ms=self.text_wait_ms,
                                         text_hold=self.text_hold, prefix_cache=bool(self.prefix_cache))
        self.sched.start()
        print(f"Batch synthesis server listening on {self.socket_path} (--concurrent: {self.max_batch} slots shared by every "
              f"request, up to {self.max_queue} queued utterances)")
        try:
            while self._running and self.sched.alive:
                try:
                    conn, _ = sock.accept()
                except socket.timeout:
                    continue
                except OSError:
                    break
                try:
                    conn.settimeout(10.0)            # a client that never finishes its request cannot hold the accept thread
                    msg = P.read_talker_request(conn)
                    if msg is None:
                        conn.close()
                        continue
                    conn.settimeout(None)
                except Exception as e:
                    print(f"Error: {e}")
                    self._send_error(conn)
                    conn.close()
                    continue
                self.sched.submit(conn, msg, time.time())
        finally:
            self.sched.stop()
            self._lib.voc_set_max_workgroups(0)
            sock.close()
            if os.path.exists(self.socket_path):
                os.unlink(self.socket_path)

    def close(self):
        self._running = False
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        self._stream_pool = None       # the push worker of streamed requests (the pipeline's worker when there is one)
        if self.pipeline:
            self._lib.voc_set_max_workgroups(0)
        self.voc.close()               # frees the streaming chunk walk first
        self._vstream = None
        self._istreams = {}
        self.eng.destroy()


class TextFeed:
    """The text of one "text_stream" request on its way into the frame loop: what the client has sent is read without
    blocking (poll), turned into token ids (text through the incremental tokeniser) and projected; take() hands the rows that
    are ready to the engine thread, which is the only caller.  project(ids, final) -> rows [n (+ 1: the tts_eos row)][hidden]."""

    def __init__(self, project, encoder, new_encoder, first_ids, n_tokens):
        self._project, self._encoder, self._new_encoder = project, encoder, new_encoder
        self._by_text = encoder is not None
        self._parser = P.TextRecordParser()
        self._rows = [project(first_ids)] if len(first_ids) else []
        self.last_rx = time.monotonic()                     # when the client's last bytes arrived (the request itself at first)
        self.n_tokens = int(n_tokens) + len(first_ids)     # text tokens so far (the final push's n_text)
        self.ended = False                                  # the end-of-text record has arrived
        self.final_pushed = False

    def _ids(self, ids, final=False):
        self.n_tokens += len(ids)
        if len(ids) or final:
            self._rows.append(self._project([int(t) for t in ids], final))

    def records(self, data):
        for kind, body in self._parser.feed(data):
            if kind == P.TEXT_IDS:
                if self._by_text:
                    raise ValueError("token ids after text: the held-back tail of the text could not be placed")
                self._ids(body)
            elif kind == P.TEXT_BYTES:
                if self._encoder is None:
                    if self._new_encoder is None:
                        raise RuntimeError("no tokenizer configured (--tokenizer DIR) for a text record")
                    self._encoder = self._new_encoder()      # ids first, text from here on: a fresh piece of text
                    self._by_text = True
                self._ids(self._encoder.feed(body))
            else:
                self._ids(self._encoder.finish() if self._encoder is not None else [], final=True)
                self.ended = True

    def poll(self, conn):
        """Reads what has arrived.  -> False once the client has closed its sending side before the end-of-text record."""
        while not self.ended:
            try:
                data = conn.recv(65536, socket.MSG_DONTWAIT)
            except (BlockingIOError, InterruptedError):
                return True
            if not data:
                return False
            self.last_rx = time.monotonic()
            self.records(data)
        return True

    def ready(self):
        """Whether take() has something for the engine: at least one row, or the end of the text."""
        return bool(self._rows) or (self.ended and not self.final_pushed)

    def take(self):
        """-> (rows [n][hidden] to push now, whether they end the text)."""
        rows, self._rows = self._rows, []
        final = self.ended and not self.final_pushed
        return (np.concatenate(rows) if rows else None), final


class _Request:
    """A request of --concurrent in flight: its connection and what has come back so far."""

    def __init__(self, conn, items, stream, t0):
        self.conn, self.stream, self.t0 = conn, bool(stream), t0
        self.n = len(items)
        self.left = self.n                      # utterances that have not ended
        self.codes = [None] * self.n            # per request index
        self.state = {"failed": False, "n": self.n, "frames": 0}   # the push worker's view (BatchSynthesisServer._push)
        self.gone = False                       # the client went away or the request failed: its slots are released
        self.feed = next((it[4] for it in items if len(it) > 4), None)   # TextFeed of a "text_stream" request
        self.prompts = None                     # codec prompts per request index (None: the request has none)
        if any(getattr(it, "prompt", None) is not None for it in items):
            self.prompts = [None] * self.n
            for it in items:
                self.prompts[it[0]] = getattr(it, "prompt", None)
        self.starved_since = None               # text_hold: since when its slot has been held (None: it is not)


class ConcurrentScheduler:
    """The engine and vocoder sides of `--concurrent` (module docstring).  `eng` has the FrameEngine surface open / admit /
    release / run / done / codes; the callables are the server's: prepare(msg) -> [(request index, prefix, n_text,
    SlotParams)] in queue order (raises on a malformed request), reply(conn, codes per utterance, t0) answers and closes an
    unstreamed request (a request that does not use the chunk walk: reply(conn, codes, t0, vocoder, arithmetic)), push(conn, state, resets, entries) and close_stream(conn, state, t0) stream records and end a streamed
    one, send_error(conn) writes -2.  The engine thread is the only caller of `eng`, the one worker thread the only caller of
    reply / push / close_stream.

    A client is gone once it has closed its connection (POLLHUP); a client that only shuts down its sending side after the
    request (shutdown(SHUT_WR)) still gets its reply.  Every write to a request's connection is bounded by send_timeout
    seconds (SO_SNDTIMEO): a client that stays connected but stops reading fails its own request -- the writer's error marks
    it failed, the engine then releases its slots -- instead of holding the one worker, and with it every other request.

    A "text_stream" request (an item with a fifth entry, its TextFeed) runs in a text slot: before every check the engine
    thread reads what its client has sent and pushes the rows (eng.push_text); a check that runs no frame because such a slot
    waits for its text (eng.text_state) polls the starving requests' connections for at most text_wait_ms, after which a
    request that has still sent nothing fails (-2) and its slot is released -- the stall is the whole batch's, so it is
    bounded the same way a stalled reader is.

    text_hold (the engine was told eng.hold_text() before this scheduler opens the batch): a text slot without a row is held
    inside the frame and the other slots step on, so a slow text client costs nobody else time.  A text-stream request is then
    admitted only once its feed has its first row (a slot without a frame cannot be held), waiting in the queue meanwhile
    while later requests pass it; a request whose slot has been held for text_wait_ms with no byte received from its client
    fails alone (-2, slot released); starved_checks counts only the checks that ran no frame (every live slot held), and
    held_steps sums the frame steps requests were held for.

    prefix_cache (the engine was told eng.prefix_cache(n, rows) before this scheduler opens the batch): the keys of an
    admission -- each item's `prefix_key` attribute (16 bytes; an item without one is admitted uncached) -- go to
    eng.admit(..., keys=[...]) in slot order; prefix_hits / prefix_misses count the flags it returns.  Without it admit is
    called as it always was, whatever the items carry.

    Codec prompts: an item's `prompt` attribute ([T][16] int32; absent or None: no prompt) goes to eng.admit(...,
    prompts=[...]) in slot order -- only when an utterance of the admission has one, so an engine without the argument
    serves everything else.  A streamed request's push worker finds the prompt of a slot it resets in state["prompts"][slot];
    an unstreamed request whose vocoder is not the chunk walk gets them as reply's sixth argument."""

    def __init__(self, eng, max_batch, max_queue, prepare, reply, push, close_stream, send_error, check_every=8,
                 send_timeout=30.0, text_wait_ms=200.0, text_hold=False, prefix_cache=False):
        from concurrent.futures import ThreadPoolExecutor
        self.eng, self.B, self.max_queue, self.check_every = eng, int(max_batch), int(max_queue), int(check_every)
        self._prepare, self._reply, self._push, self._close_stream, self._send_error = prepare, reply, push, close_stream, send_error
        self._cv = threading.Condition()
        self._queue = collections.deque()       # (request, (utt, prefix, n_text, params)) in admission order
        self._running = False
        self._pool = ThreadPoolExecutor(max_workers=1)
        self._thread = None
        self.alive = True                       # False once the engine thread has stopped on an error
        self.frame_steps = 0                    # frame steps the engine has run
        self.send_timeout = float(send_timeout)
        self.text_wait_ms = float(text_wait_ms)
        self.starved_checks = 0                 # checks that ran no frame because a text slot waited for its text
        self.text_hold = bool(text_hold)
        self.held_steps = 0                     # text_hold: frame steps text slots were held for, summed over requests
        self.prefix_cache = bool(prefix_cache)
        self.prefix_hits = self.prefix_misses = 0   # prefix_cache: admitted utterances that came from the cache / were prefilled

    # ---- accept side ----
    def submit(self, conn, msg, t0=None):
        """Check a request and queue its utterances, or answer -2 on its own connection and close it.  -> True if queued."""
        sec = int(self.send_timeout)
        conn.setsockopt(socket.SOL_SOCKET, socket.SO_SNDTIMEO,
                        struct.pack("ll", sec, int(round((self.send_timeout - sec) * 1e6))))
        try:
            items = self._prepare(msg)
            vocoder, arithmetic = request_vocoder(msg), request_vocoder_arithmetic(msg)
        except Exception as e:
            print(f"Error: {e}")
            return self._refuse(conn)
        with self._cv:
            if not self.alive or len(self._queue) + len(items) > self.max_queue:
                print(f"Error: queue full ({len(self._queue)} of {self.max_queue} utterances queued)" if self.alive else
                      "Error: the engine has stopped")
                return self._refuse(conn)
            req = _Request(conn, items, msg.get("stream"), time.time() if t0 is None else t0)
            req.state["vocoder"], req.state["vocoder_arithmetic"] = vocoder, arithmetic
            self._queue.extend((req, it) for it in items)
            self._cv.notify()
        return True

    def _refuse(self, conn):
        self._send_error(conn)
        conn.close()
        return False

    def start(self):
        self._running = True
        self._thread = threading.Thread(target=self._engine_main, name="q3-engine", daemon=True)
        self._thread.start()

    def stop(self):
        with self._cv:
            self._running = False
            self._cv.notify()
        if self._thread is not None:
            self._thread.join()
        self._pool.shutdown(wait=True)          # replies in flight go out before the server goes

    # ---- engine side ----
    @staticmethod
    def _client_gone(req):
        """The request failed on the writer's side, or its client closed the connection (hang-up; a half-close is not)."""
        if req.state["failed"]:
            return True
        try:
            p = select.poll()
            p.register(req.conn.fileno(), select.POLLIN)
            ev = p.poll(0)
        except (OSError, ValueError):
            return True
        return bool(ev and ev[0][1] & (select.POLLHUP | select.POLLERR | select.POLLNVAL))

    def _drop(self, req):
        """Engine side: a request that is gone or failed -- its queued utterances are skipped, its connection closes (after
        whatever the worker still has for it)."""
        if not req.gone:
            req.gone = True
            self._pool.submit(req.conn.close)

    def _fail(self, req, why):
        """Engine side: a request that cannot go on gets -2 now; its slots are released at this check."""
        if not req.gone:
            print(f"Error: {why}")
            req.state["failed"] = True
            self._pool.submit(self._send_error, req.conn)
            self._drop(req)

    def _feed_text(self, owner):
        """Engine side, before a check: read what the text-stream clients have sent and push the rows that are ready."""
        for b, o in enumerate(owner):
            req = o[0] if o is not None else None
            if req is None or req.feed is None or req.gone or req.feed.final_pushed:
                continue
            try:
                if not req.feed.poll(req.conn):
                    raise ValueError("the client closed its sending side before the end of its text")
                rows, final = req.feed.take()
                if rows is not None or final:
                    self.eng.push_text(b, rows if rows is not None else np.zeros((0, 1024), np.float32), final=final,
                                       n_text=req.feed.n_tokens)
                    req.feed.final_pushed = final
            except Exception as e:     # a malformed record, an unknown token, more rows than frames: this request only
                self._fail(req, f"text stream: {e}")

    def _wait_for_text(self, owner):
        """Engine side, after a check that ran no frame: if text slots starve, wait (at most text_wait_ms) until one of their
        clients has sent something, and fail those that are still silent after it.  -> True if the check was a starved one."""
        _, starved = self.eng.text_state()
        waiting = {id(owner[b][0]): owner[b][0] for b in range(self.B) if starved[b] and owner[b] is not None and not owner[b][0].gone}
        if not waiting:
            return False
        self.starved_checks += 1
        p = select.poll()
        for req in waiting.values():
            p.register(req.conn.fileno(), select.POLLIN)
        if not p.poll(self.text_wait_ms):
            for req in waiting.values():
                self._fail(req, f"text stream: no text for {self.text_wait_ms:.0f} ms while the frame loop waited for it")
        return True

    def _text_ready(self, req):
        """Engine side, text_hold: whether a queued text-stream request has its first row (so that its slot never waits
        without a frame).  A client that closed its sending side before any row fails here."""
        try:
            if not req.feed.poll(req.conn):
                raise ValueError("the client closed its sending side before the end of its text")
        except Exception as e:
            self._fail(req, f"text stream: {e}")
            return False
        return req.feed.ready()

    def _check_held(self, owner, ran, last_held):
        """Engine side, text_hold, after every check: count the held steps, fail the requests whose slot has been held for
        text_wait_ms without a byte from their client, and -- after a check that ran no frame because every live slot is
        held -- wait a moment for one of them to send something.  -> True if the check was such a starved one."""
        held = self.eng.held_steps()
        for b in range(self.B):
            if owner[b] is not None:
                self.held_steps += int(held[b]) - last_held[b]
                last_held[b] = int(held[b])
        _, starved = self.eng.text_state()
        now = time.monotonic()
        waiting = {}
        for b in range(self.B):
            req = owner[b][0] if owner[b] is not None else None
            if req is None or req.feed is None or req.gone:
                continue
            if not starved[b]:
                req.starved_since = None
                continue
            if req.starved_since is None:
                req.starved_since = now
            idle_ms = (now - max(req.starved_since, req.feed.last_rx)) * 1e3
            if idle_ms >= self.text_wait_ms:
                self._fail(req, f"text stream: no text for {self.text_wait_ms:.0f} ms while its slot was held")
            else:
                waiting[id(req)] = (req, self.text_wait_ms - idle_ms)
        if ran != 0 or not waiting:
            return ran == 0 and bool(starved.any())
        self.starved_checks += 1
        p = select.poll()
        for req, _ in waiting.values():
            p.register(req.conn.fileno(), select.POLLIN)
        p.poll(max(1.0, min([20.0] + [left for _, left in waiting.values()])))   # short: a new request must not wait for it
        return True

    def _engine_main(self):
        owner = [None] * self.B                 # (request, utt) of each slot
        try:
            self._engine_loop(owner)
        except Exception as e:
            print(f"Error: the engine thread stopped: {e}")
            with self._cv:
                self.alive = False
                pending = {id(r): r for r, _ in self._queue}
                self._queue.clear()
            pending.update({id(o[0]): o[0] for o in owner if o is not None})
            for req in pending.values():
                if not req.gone:
                    req.gone = True
                    self._pool.submit(self._refuse, req.conn)

    def _engine_loop(self, owner):
        eng, B = self.eng, self.B
        eng.open(B)
        pushed = [0] * B
        last_held = [0] * B                    # text_hold: eng.held_steps() of each slot at the last check
        pending_pushes = []
        while True:
            with self._cv:
                while self._running and not self._queue and all(o is None for o in owner):
                    self._cv.wait()            # nothing live, nothing queued: block (no spinning)
                if not self._running:
                    break
                free = [b for b in range(B) if owner[b] is None]
                take, later = [], []
                while self._queue and len(take) < len(free):
                    req, it = self._queue.popleft()
                    if req.gone:
                        continue
                    if self.text_hold and req.feed is not None and not self._client_gone(req) and not self._text_ready(req):
                        if not req.gone:
                            later.append((req, it))   # no row yet: it keeps its place, those behind it pass
                        continue
                    take.append((req, it))
                self._queue.extendleft(reversed(later))
            for req in {id(r): r for r, _ in take + later}.values():   # a client that left while its request waited
                if self._client_gone(req):
                    self._drop(req)
            take = [(r, it) for r, it in take if not r.gone]
            if not take and all(o is None for o in owner):
                waiting = [r for r, _ in later if not r.gone]
                if waiting:                    # only text requests without a row are queued: until one of them sends (or leaves)
                    p = select.poll()
                    for r in waiting:
                        p.register(r.conn.fileno(), select.POLLIN)
                    p.poll(20.0)               # (short: a request submitted meanwhile is looked at soon)
                continue                       # what was queued has left and nothing is live: back to waiting
            resets = collections.defaultdict(list)
            if take:
                slots = free[:len(take)]
                args = (slots, [it[1] for _, it in take], [it[2] for _, it in take], [it[3] for _, it in take])
                prompts = [getattr(it, "prompt", None) for _, it in take]
                kw = {"prompts": prompts} if any(p is not None for p in prompts) else {}
                if self.prefix_cache:
                    hit = eng.admit(*args, keys=[getattr(it, "prefix_key", None) for _, it in take], **kw)
                    self.prefix_hits += int(np.count_nonzero(hit))
                    self.prefix_misses += len(take) - int(np.count_nonzero(hit))
                else:
                    eng.admit(*args, **kw)
                for b, (req, it), prompt in zip(slots, take, prompts):
                    owner[b] = (req, it[0])
                    pushed[b] = 0
                    last_held[b] = 0
                    if req.stream:
                        resets[id(req)].append(b)
                        if prompt is not None and req.state.get("vocoder") == "incremental":
                            req.state.setdefault("prompts", {})[b] = prompt   # (taken by the push that resets slot b)
            text_live = any(o is not None and o[0].feed is not None for o in owner)
            if text_live:
                self._feed_text(owner)
            ran = eng.run(self.check_every)
            self.frame_steps += ran
            if self.text_hold:
                waited = text_live and self._check_held(owner, ran, last_held)
            else:
                waited = ran == 0 and text_live and self._wait_for_text(owner)
            done, per = eng.done()
            # clients that went away: their slots go idle now
            live = {id(o[0]): o[0] for o in owner if o is not None}
            for req in live.values():
                if self._client_gone(req):
                    self._drop(req)
            gone = [b for b in range(B) if owner[b] is not None and owner[b][0].gone]
            if gone:
                eng.release(gone)
                for b in gone:
                    owner[b] = None
            fin = [b for b in range(B) if owner[b] is not None and done[b]]
            streamed = [b for b in range(B) if owner[b] is not None and owner[b][0].stream]
            if not fin and not streamed:
                if ran == 0 and not gone and not take and not waited:
                    raise RuntimeError("the engine ran no frame and no utterance ended")
                continue
            codes, _ = eng.codes()
            entries = collections.defaultdict(list)
            for b in streamed:
                req, utt = owner[b]
                n, f = int(per[b]), b in fin
                if n > pushed[b] or f:
                    whole = np.ascontiguousarray(codes[:n, b, :], dtype=np.int32) if f else None
                    entries[id(req)].append((b, utt, np.ascontiguousarray(codes[pushed[b]:n, b, :]), f, whole))
                    pushed[b] = n
                    if f:
                        req.state["frames"] += n
            for f_ in pending_pushes:                # at most one check's pushes in flight
                f_.result()
            pending_pushes = []
            reqs = {id(owner[b][0]): owner[b][0] for b in streamed}
            for key, req in reqs.items():
                if entries[key] or resets[key]:
                    pending_pushes.append(self._pool.submit(self._push, req.conn, req.state, resets[key], entries[key]))
            for b in fin:
                req, utt = owner[b]
                owner[b] = None
                req.codes[utt] = np.ascontiguousarray(codes[:int(per[b]), b, :], dtype=np.int32)
                req.left -= 1
                if req.left == 0:
                    if req.stream:
                        self._pool.submit(self._close_stream, req.conn, req.state, req.t0)
                    elif req.state["vocoder"] == "walk":
                        self._pool.submit(self._reply, req.conn, req.codes, req.t0)
                    elif req.prompts is None:   # (reply's documented form is (conn, codes, t0); another vocoder adds its mode and arithmetic)
                        self._pool.submit(self._reply, req.conn, req.codes, req.t0, req.state["vocoder"], req.state["vocoder_arithmetic"])
                    else:
                        self._pool.submit(self._reply, req.conn, req.codes, req.t0, req.state["vocoder"], req.state["vocoder_arithmetic"],
                                          req.prompts)
        # shutting down: whatever is still in flight or queued gets -2
        with self._cv:
            rest = {id(r): r for r, _ in self._queue}
            self._queue.clear()
        rest.update({id(o[0]): o[0] for o in owner if o is not None})
        for req in rest.values():
            if not req.gone:
                req.gone = True
                self._pool.submit(self._refuse, req.conn)


VOCODER_MODES = ("walk", "incremental")


def request_vocoder(msg):
    """A request's "vocoder" key -> "walk" (the default: the reference's chunk walk) or "incremental" (the carry-state decode,
    include/qwen3tts_voc.h voc_incr_*); raises ValueError on any other value (the request is then answered with -2)."""
    v = msg.get("vocoder", "walk")
    if not isinstance(v, str) or v not in VOCODER_MODES:
        raise ValueError(f"vocoder must be one of {VOCODER_MODES} (got {v!r})")
    return v


VOCODER_ARITHMETICS = ("exact", "split")


def request_vocoder_arithmetic(msg):
    """A request's "vocoder_arithmetic" key -> "exact" (the default) or "split" (the incremental decode's split-fp16
    convolutions, voc_incr_set_arithmetic); raises ValueError on any other value, and on the key in a request that is not
    "vocoder": "incremental" (the request is then answered with -2)."""
    vocoder = request_vocoder(msg)
    if "vocoder_arithmetic" not in msg:
        return "exact"
    a = msg["vocoder_arithmetic"]
    if not isinstance(a, str) or a not in VOCODER_ARITHMETICS:
        raise ValueError(f"vocoder_arithmetic must be one of {VOCODER_ARITHMETICS} (got {a!r})")
    if vocoder != "incremental":
        raise ValueError('vocoder_arithmetic needs "vocoder": "incremental"')
    return a


PROMPT_KEYS = ("prompt_codes", "prompt_token_ids", "prompt_text", "voice")


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
        a = one(codes)
        return [a] * n_utts
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


_PARAM_KEYS = ("temperature", "top_k", "top_p", "cp_temperature", "cp_top_k", "seed")   # request keys = SlotParams fields


def request_slot_params(msg, defaults, max_tokens_cap):
    """--concurrent: a request's sampling keys and max_tokens over the server's defaults -> SlotParams (utt 0); raises
    ValueError on a value out of range or of the wrong type."""
    kw = {}
    for field in _PARAM_KEYS:
        key = field
        v = msg.get(key)
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{key} must be a number (got {v!r})")
        if field in ("top_k", "cp_top_k", "seed") and not (isinstance(v, int) or float(v).is_integer()):
            raise ValueError(f"{key} must be an integer (got {v!r})")
        kw[field] = int(v) if field in ("top_k", "cp_top_k", "seed") else float(v)
    mt = msg.get("max_tokens")
    if mt is not None and (isinstance(mt, bool) or not isinstance(mt, int)):
        raise ValueError(f"max_tokens must be an integer (got {mt!r})")
    kw["max_frames"] = min(int(mt), max_tokens_cap) if mt else defaults.max_frames
    p = dataclasses.replace(defaults, **kw)
    p.check(max_tokens_cap)
    return p


def pack_batch_request(texts=None, token_ids=None, language="russian", max_tokens=None, stream=False, temperature=None,
                       top_k=None, top_p=None, cp_temperature=None, cp_top_k=None, seed=None, vocoder=None,
                       vocoder_arithmetic=None, text_stream=False, prompt_codes=None, prompt_token_ids=None, prompt_text=None,
                       voice=None) -> bytes:
    """The request of the batched protocol; the sampling keys (honoured by --concurrent), the vocoder mode ("walk" /
    "incremental") and the incremental mode's arithmetic ("exact" / "split") are sent only when given.  text_stream: the
    request carries only the first piece of its one utterance's text; the rest follows as text records.  prompt_codes ([T][16], or
    one such per utterance), prompt_token_ids / prompt_text, voice: the codec prompt the utterances continue (--concurrent)."""
    import json
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
    for key, v in (("temperature", temperature), ("top_k", top_k), ("top_p", top_p), ("cp_temperature", cp_temperature),
                   ("cp_top_k", cp_top_k), ("seed", seed), ("vocoder", vocoder), ("vocoder_arithmetic", vocoder_arithmetic),
                   ("prompt_codes", prompt_codes), ("prompt_token_ids", prompt_token_ids), ("prompt_text", prompt_text),
                   ("voice", voice)):
        if v is not None:
            msg[key] = v
    raw = json.dumps(msg).encode()
    return struct.pack("<I", len(raw)) + raw


def pack_batch_reply(results) -> bytes:
    parts = [struct.pack("<i", len(results))]
    for codes, pcm in results:
        c = np.ascontiguousarray(codes, dtype="<i4").reshape(-1, 16)
        a = np.ascontiguousarray(pcm, dtype="<i2")
        parts += [struct.pack("<i", c.shape[0]), c.tobytes(), struct.pack("<i", a.shape[0]), a.tobytes()]
    return b"".join(parts)


def read_batch_reply(conn):
    """-> list of (codes [n][16] int32, pcm int16); raises on the error sentinel / a short read."""
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
        out.append((codes, pcm))
    return out


REC_AUDIO, REC_END = 1, 2


def pack_stream_audio(utt, pcm) -> bytes:
    a = np.ascontiguousarray(pcm, dtype="<i2").reshape(-1)
    return struct.pack("<iii", REC_AUDIO, int(utt), a.shape[0]) + a.tobytes()


def pack_stream_end(utt, codes) -> bytes:
    c = np.ascontiguousarray(codes, dtype="<i4").reshape(-1, 16)
    return struct.pack("<iii", REC_END, int(utt), c.shape[0]) + c.tobytes()


def read_stream_record(conn):
    """One record of a streamed reply -> ("audio", utt, pcm int16) / ("end", utt, codes [n][16] int32) / ("done",); raises on
    the error sentinel, an unknown record or a short read."""
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
    if kind not in (REC_AUDIO, REC_END):
        raise RuntimeError(f"unknown record {kind} in a streamed reply")
    utt, n = struct.unpack("<ii", exact(8))
    if n < 0:
        raise RuntimeError(f"record of {n} entries")
    if kind == REC_AUDIO:
        return ("audio", utt, np.frombuffer(exact(n * 2), dtype="<i2"))
    return ("end", utt, np.frombuffer(exact(n * 16 * 4), dtype="<i4").reshape(n, 16))


def synthesize_batch_stream(socket_path, texts=None, token_ids=None, language="russian", max_tokens=None, vocoder=None,
                            vocoder_arithmetic=None, **sampling):
    """Client side of the streamed request: yields its records as they arrive -- ("audio", utt, pcm) and ("end", utt, codes)
    -- until the request is done; raises on the error sentinel.  vocoder="incremental": the carry-state decode (audio from the
    first check on) instead of the chunk walk, vocoder_arithmetic="split": on its split-fp16 convolutions.  sampling: the optional
    keys of pack_batch_request."""
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.connect(socket_path)
    try:
        s.sendall(pack_batch_request(texts, token_ids, language, max_tokens, stream=True, vocoder=vocoder,
                                     vocoder_arithmetic=vocoder_arithmetic, **sampling))
        while True:
            rec = read_stream_record(s)
            if rec[0] == "done":
                return
            yield rec
    finally:
        s.close()


def synthesize_text_stream(socket_path, pieces, language="russian", max_tokens=None, vocoder=None, vocoder_arithmetic=None,
                           voice=None, prompt_codes=None, prompt_token_ids=None, prompt_text=None, **sampling):
    """Client side of a "text_stream" request (--concurrent servers): `pieces` is an iterable of the text's pieces as they
    become available -- str / bytes (UTF-8, cut anywhere; the server tokenises) or sequences of token ids.  The first piece
    goes out with the request (it must give at least one token), the others as text records from a sender thread that walks
    the iterable, then the end-of-text record.  Yields the records of synthesize_batch_stream, utterance 0.  voice, or
    prompt_codes with prompt_token_ids / prompt_text: the codec prompt the utterance continues (--text_voice servers)."""
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
        s.sendall(pack_batch_request([first] if as_text else None, None if as_text else [list(first)], language, max_tokens,
                                     stream=True, vocoder=vocoder, vocoder_arithmetic=vocoder_arithmetic, text_stream=True,
                                     prompt_codes=prompt_codes, prompt_token_ids=prompt_token_ids, prompt_text=prompt_text,
                                     voice=voice, **sampling))
        th.start()
        while True:
            rec = read_stream_record(s)
            if rec[0] == "done":
                return
            yield rec
    finally:
        s.close()
        if th.is_alive():
            th.join(timeout=5)


def synthesize_batch(socket_path, texts=None, token_ids=None, language="russian", max_tokens=None, **sampling):
    """Client side of the batched request.  sampling: the optional keys of pack_batch_request (vocoder and vocoder_arithmetic
    among them)."""
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.connect(socket_path)
    try:
        s.sendall(pack_batch_request(texts, token_ids, language, max_tokens, **sampling))
        return read_batch_reply(s)
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser(description="Qwen3-TTS batched synthesis server (MI355X)")
    ap.add_argument("--model", required=True, help="Q3TTSW1 container with talker, code predictor and text tables")
    ap.add_argument("--vocoder", required=True, help="container with the vocoder program")
    ap.add_argument("--socket", default="/tmp/qwen3_batch.sock")
    ap.add_argument("--tokenizer", default=None, help="directory with vocab.json + merges.txt")
    ap.add_argument("--max_batch", type=int, default=32)
    ap.add_argument("--n_ctx", type=int, default=512)
    ap.add_argument("--max_tokens", type=int, default=200)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--top_k", type=int, default=50)
    ap.add_argument("--cp_temperature", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--top_p", type=float, default=0.95)
    ap.add_argument("--cp_top_k", type=int, default=None, help="code predictor's top-k (default: --top_k)")
    ap.add_argument("--pipeline", action="store_true",
                    help="vocode request k on a worker thread while request k + 1 generates (one vocoder workgroup per CU)")
    ap.add_argument("--concurrent", action="store_true",
                    help="utterances of concurrent requests share one running frame loop (per-request sampling keys and seed)")
    ap.add_argument("--max_queue", type=int, default=None, help="--concurrent: utterances that may wait (default 16 x max_batch)")
    ap.add_argument("--check_every", type=int, default=8, help="--concurrent: frames between two admissions")
    ap.add_argument("--send_timeout", type=float, default=30.0,
                    help="--concurrent: seconds one write to a client may block before its request fails")
    ap.add_argument("--text_wait_ms", type=float, default=200.0,
                    help="--concurrent: milliseconds the frame loop waits for a text-stream client's text before its request fails")
    ap.add_argument("--text_hold", action="store_true",
                    help="--concurrent: a text-stream request without text for its next frame is held inside the frame while the "
                         "other requests go on (default: the whole frame loop waits for it)")
    ap.add_argument("--prefix_cache", type=int, default=0,
                    help="--concurrent: entries of the device prefix cache (0 = off): an utterance whose prefix is cached is "
                         "admitted without a prefill, with the same reply")
    ap.add_argument("--prefix_cache_rows", type=int, default=64, help="--prefix_cache: prefix rows an entry can hold")
    ap.add_argument("--voice", action="append", default=[], metavar="NAME=DIR",
                    help="--concurrent: a codec prompt requests may name with \"voice\": \"NAME\"; DIR as "
                         "encode_reference_audio --output_dir writes it (repeatable)")
    ap.add_argument("--voice_warm", type=int, default=0,
                    help="with --concurrent: cache the incremental vocoder's warm-up per codec prompt in N snapshot slots of the "
                         "vocoder (a known voice then costs one copy launch instead of decoding its prompt; default 0 = off)")
    ap.add_argument("--text_voice", action="store_true",
                    help="--concurrent: a text-stream request may carry a codec prompt (\"voice\" / \"prompt_codes\"): streamed "
                         "text in the prompt's voice")
    a = ap.parse_args()
    if any("=" not in v or not v.split("=", 1)[0] for v in a.voice):
        ap.error("--voice takes NAME=DIR")
    srv = BatchSynthesisServer(a.model, a.vocoder, a.socket, a.max_batch, a.n_ctx, a.max_tokens, a.temperature, a.top_k,
                               a.cp_temperature, a.tokenizer, a.seed, pipeline=a.pipeline, concurrent=a.concurrent,
                               max_queue=a.max_queue, top_p=a.top_p, cp_top_k=a.cp_top_k, check_every=a.check_every,
                               send_timeout=a.send_timeout, text_wait_ms=a.text_wait_ms, text_hold=a.text_hold,
                               prefix_cache=a.prefix_cache, prefix_cache_rows=a.prefix_cache_rows,
                               voices=dict(v.split("=", 1) for v in a.voice), text_voice=a.text_voice,
                               voice_warm=a.voice_warm)
    try:
        srv.serve()
    finally:
        srv.close()


if __name__ == "__main__":
    main()
