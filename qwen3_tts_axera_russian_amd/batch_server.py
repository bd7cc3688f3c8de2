#!/usr/bin/env python3
"""Batched synthesis server: B utterances per request through the on-device frame loop.

The reference closes the autoregressive loop in its client, two socket round trips per frame and one
utterance at a time (dual_npu/tts_client.py:144-215; `listen(1)`, llamacpp_talker_server.py:314).  This
server keeps that front-end (tokenizer, text projection, dual-stream prefix: llamacpp_talker_server.py:
115-161; EOS heuristics and sampling on the device) and runs the whole loop for all utterances of a request
on the GPU (include/qwen3tts_engine.h), then the vocoder's chunk walk (vocoder_server.py:73-121, :175) per
utterance.  The wire protocol and its clients: batch_wire; a request's keys and their -2 rules: batch_request;
`--concurrent`, its threads, text slots and `--text_hold`: batch_scheduler.

One process per GPU (HIP_VISIBLE_DEVICES), like the other servers.

Streamed reply: every check_every frames the new frames of every live slot go to the vocoder's streaming chunk walk (voc_stream_push, on one
worker thread with one vocoder workgroup per compute unit, as in --pipeline); a full 64-frame chunk is decoded as soon as its
frames exist, and all samples no later cross-fade can change go out at once.  An utterance's PCM records joined, and its codes,
are bit for bit what the unstreamed reply carries.

`--prefix_cache N` (with `--concurrent`; N entries of up to `--prefix_cache_rows` prefix rows each, default 0 = off): the
engine keeps the KV rows and the frame-0 state of admitted prefixes in a device pool (q3e_prefix_cache / q3e_admit_keyed), and
an utterance whose prefix is there is admitted by one copy launch instead of a prefill: a repeated text, the k takes of a
request that lists one text k times with a seed, and every text-stream request that begins with the same token (its 8-row
streaming prefix depends on the first token alone).  The key is the server's own (batch_request.prefix_key); a client never
supplies one.  The prefix rows are still built on the accept thread; the wire protocol is unchanged.

`--text_voice` (with `--concurrent`): a "text_stream" request may carry a codec prompt -- "voice", or "prompt_codes" with an
optional "prompt_token_ids" / "prompt_text" -- and its audio then continues the prompt while its text still arrives: streamed
text in a cloned voice.  The checks are the codec prompt's, and 8 + the prompt text's tokens + T + max_tokens must fit n_ctx.
The utterance runs in a text slot that continues a prompt (q3e_slot_params.reserved == 3): its prefix is rows 0..6 of the
streaming prefix, one `text + codec_pad` row per token of the prompt's text, then the first token + codec_bos
(build_prefix_stream(first, head)); the prompt's T frames follow as they do for any prompted utterance; and row i of the
streamed text rides on GENERATED frame i.  Its text length for the EOS heuristics counts the prompt's text, as the unstreamed
prompted request of the same texts does, and its prefix key is prefix_key(b"stream", prompt text ids + first token, codes).
The vocoder follows the streamed reply of a prompted request.  `--text_hold`, `--text_wait_ms` and `--prefix_cache` work as
they do for any text-stream request; the wire protocol has no new record.  Without the flag such a request is answered -2.

`--sampler_rules` (with `--concurrent`): the engine reserves a sampler-rules entry and an emitted-id set per slot
(q3e_rules_reserve, before the scheduler opens the batch), and a request may then set the rules its utterances are sampled
under -- "repetition_penalty", "repetition_window", "eos_boost", "eos_force", "min_tokens", "cp_top_p", or a "sampler" preset
(batch_request says which values, and that "upstream" is a recollection) -- through q3e_admit_ruled.  A request without these
keys, or with the default values spelled out, gets the reply it gets without the flag, bit for bit; the per-request output
names a rule set that is not the default.  Without the flag a request that carries any of the keys is answered -2; the wire
protocol has no new record.

`--logprobs` (with `--concurrent`): the engine reserves one float32 beside every id of the codes (q3e_scores_reserve, before
the scheduler opens the batch), and a request may then carry "logprobs": true: its reply holds, for every id it holds, the
model's log-probability at temperature 1 of that id (batch_request, batch_wire) -- what a client that asked for k takes ranks
them by.  The ids and the PCM are those of the request without the key, bit for bit, and a reply to a request without the key
is byte for byte the reply of a server without the flag.  The per-request line names the mean log-probability of each
utterance's code_0.  Without the flag the key is answered -2.

`--voice_warm N` (with `--concurrent`; default 0 = off): the incremental vocoder's warm-up per codec prompt is cached in N
snapshot slots of the vocoder handle (voice_warm.VoiceWarmCache, which says how).  A hit pushes no prompt frame: all hits of one
check go into one voc_incr_restore, and an unstreamed reply starts from the slot (synthesize_incremental(start_slot=)).  Several slots admitted together with the same new
voice: the first is the miss, the rest hit.  Every reply -- codes and PCM, streamed and not, both arithmetics as long as no
push is redone exactly -- is bit for bit the reply without the flag; requests without a prompt, or not "incremental", touch
nothing.  The counters voice_warm_hits / voice_warm_misses / voice_warm_evictions are on the server object, hits and misses in the
per-request line.  Only the vocoder worker touches the cache.

`--encoder ENC.q3w` (with `--concurrent`): a request may carry its codec prompt as AUDIO -- "prompt_audio" and the clip's raw PCM
behind the JSON (batch_wire, batch_request) -- and the server encodes it itself: one Encoder sized by `--prompt_audio_seconds`
(default 20), one caller at a time under its own lock, the PCM front-end and the speech-tokenizer encoder both on the GPU
(Encoder.encode_pcm).  The accept thread checks the descriptor (-2 before any payload byte is read), reads the payload, looks
the clip up in the id cache (`--prompt_audio_cache N`, default 16: an LRU keyed by a digest of format, channels, rate,
"max_frames" and the bytes; a hit runs no encode), encodes what is missing -- the clips of one request that share format,
channels and rate in one enc_encode_pcm call -- and hands the scheduler the request with "prompt_codes" equal to the ids: the
same checks, prefix key and reply, so `--prefix_cache`, `--voice_warm` and `--text_voice` work unchanged.  "register_voice":
"NAME" keeps the ids and the prompt's text for later "voice": "NAME" requests (at most `--max_voices` run-time names, default
64; a --voice name cannot be replaced); with "texts": [] the request only registers and is answered i32 0.  The counters
prompt_audio_hits / prompt_audio_misses / prompt_audio_evictions are on the server object, hits and misses in the per-request
line.  Without the flag such a request is answered -2.

`--speaker_encoder SPK.q3w` (with `--concurrent --encoder`): the other half of a cloned voice.  Any `--concurrent` server takes
"speaker_embedding" (batch_request: one more prefix row, tts_pad_embed + the embedding), alone -- "x-vector only", no transcript
needed -- or beside a codec prompt, and `--voice NAME=DIR` picks up DIR's ref_spk_embedding.npy; with this flag the server
computes the embedding itself from a "prompt_audio" clip: one SpeakerEncoder sized like the encoder, under the encoder's lock,
fed the clip's 24 kHz samples from the encoder's own front-end (Encoder.resample_pcm: the samples its codec prompt comes from).
"speaker": "with_prompt" adds the embedding to the clip's codec prompt, "only" takes the embedding alone, and the request then
IS the request with the embedding (and codes) inline: same checks, same prefix key (which digests the embedding), same reply.
The prompt-audio LRU keeps the embedding beside the ids (a repeated clip runs no embed), "register_voice" keeps it with the
voice.  The speaker encoder's dim must equal the model's hidden size.  That the checkpoint's speaker encoder is the pinned class
at this geometry, its mel parameters and the row's position are recollection; no similarity claim is made.

`--pipeline`: the vocoder of request k runs on a worker thread (and replies on k's connection) while the frame loop of request
k + 1 already runs -- the reference's client does the same per 64-frame block of ONE utterance (tts_client.py:188-197).  The
vocoder then launches one persistent workgroup per compute unit (voc_set_max_workgroups(-1)), which leaves the frame loop's
workgroups room beside it (244 -> 209 ms per 32 x 64-frame step); results are bit-identical.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import signal
import socket
import struct
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import hiplib
from . import protocol as P
from .batch_request import (PROMPT_KEYS, VOCODER_ARITHMETICS, VOCODER_MODES, PromptAudioCache, Utterance, VoiceTable,  # noqa: F401
                            load_voice, load_voice_speaker, prefix_key, prompt_audio_digest, request_has_prompt, request_has_speaker,
                            request_prompt_audio, request_logprobs, request_prompt_codes, request_slot_params, request_slot_rules,
                            request_speaker_embedding, request_speaker_mode, request_vocoder, request_vocoder_arithmetic)
from .batch_scheduler import ConcurrentScheduler, PushEntry, ReplyState, TextFeed, new_entries  # noqa: F401
from .batch_wire import (REC_AUDIO, REC_END, REC_SCORES, pack_batch_reply, pack_batch_request, pack_stream_audio,  # noqa: F401
                         pack_stream_end, pack_stream_scores, read_batch_reply, read_stream_record, synthesize_batch, synthesize_batch_stream,
                         synthesize_text_stream)
from .engine import FrameEngine, SlotParams
from .frontend import TextFrontEnd
from .vocoder import Vocoder
from .voice_warm import VoiceWarmCache
from .weights import ModelConfig, read_pack


class BatchSynthesisServer:
    sampler_rules = False      # --sampler_rules: requests may carry sampler rules (set by __init__)
    logprobs = False           # --logprobs: requests may ask for the log-probabilities of their ids (set by __init__)
    encoder = None             # --encoder: the Encoder audio prompts go through (set by __init__)
    runtime_voices = None      # the VoiceTable "register_voice" writes (set by __init__)
    speaker = None             # --speaker_encoder: the SpeakerEncoder audio prompts' embeddings come from (set by __init__)

    def __init__(self, model_path, vocoder_path, socket_path="/tmp/qwen3_batch.sock", max_batch=32, n_ctx=512,
                 max_tokens=200, temperature=0.0, top_k=50, cp_temperature=0.0, tokenizer=None, seed=0,
                 install_signal_handlers=True, max_request=None, pipeline=False, concurrent=False, max_queue=None, top_p=0.95,
                 cp_top_k=None, check_every=8, send_timeout=30.0, text_wait_ms=200.0, text_hold=False, prefix_cache=0,
                 prefix_cache_rows=64, voices=None, text_voice=False, voice_warm=0, sampler_rules=False, encoder=None,
                 prompt_audio_seconds=20.0, prompt_audio_cache=16, max_voices=64, logprobs=False, speaker_encoder=None):
        if concurrent and pipeline:
            raise ValueError("--concurrent runs its own vocoder worker: it does not combine with --pipeline")
        self.socket_path, self.max_batch, self.max_tokens, self.n_ctx = socket_path, max_batch, max_tokens, n_ctx
        cp_top_k = top_k if cp_top_k is None else cp_top_k
        # the settings a request of --concurrent inherits for every key it leaves out
        self.defaults = SlotParams(max_frames=max_tokens, temperature=float(temperature), top_k=int(top_k), top_p=float(top_p),
                                   cp_temperature=float(cp_temperature), cp_top_k=int(cp_top_k), seed=int(seed))
        self.defaults.check(max_tokens)
        self.concurrent, self.check_every = bool(concurrent), int(check_every)
        self.max_queue = int(max_queue) if max_queue else 16 * max_batch
        self.send_timeout, self.text_wait_ms = float(send_timeout), float(text_wait_ms)
        alone = not concurrent
        for bad, message in (
                (text_hold and alone, "--text_hold holds text slots of the shared frame loop: it needs --concurrent"),
                (int(prefix_cache) < 0 or int(prefix_cache_rows) <= 0,
                 "--prefix_cache takes a number of entries >= 0, --prefix_cache_rows a number of rows >= 1"),
                (prefix_cache and alone, "--prefix_cache serves the per-slot admissions of the shared frame loop: it needs --concurrent"),
                (voices and alone, "--voice names codec prompts of the shared frame loop's admissions: it needs --concurrent"),
                (text_voice and alone, "--text_voice lets text slots of the shared frame loop continue a codec prompt: it needs --concurrent"),
                (sampler_rules and alone, "--sampler_rules sets the sampler rules of the shared frame loop's slots: it needs --concurrent"),
                (logprobs and alone, "--logprobs records the log-probabilities of the shared frame loop's decisions: it needs --concurrent"),
                (encoder and alone, "--encoder encodes the audio prompts of the shared frame loop's admissions: it needs --concurrent"),
                (speaker_encoder and not encoder, "--speaker_encoder embeds the samples of the encoder's PCM front-end: it needs --encoder"),
                (not float(prompt_audio_seconds) > 0, "--prompt_audio_seconds takes a number > 0"),
                (int(voice_warm) < 0, "--voice_warm takes a number of snapshot slots >= 0"),
                (voice_warm and alone, "--voice_warm caches the vocoder warm-up of the shared frame loop's codec prompts: it needs --concurrent")):
            if bad:
                raise ValueError(message)
        self.text_hold, self.text_voice = bool(text_hold), bool(text_voice)
        self.sampler_rules = bool(sampler_rules)
        self.logprobs = bool(logprobs)
        self.prefix_cache, self.prefix_cache_rows = int(prefix_cache), int(prefix_cache_rows)
        self.voices = {name: load_voice(d) for name, d in dict(voices or {}).items()}   # name -> (codes [T][16], text or None)
        self.runtime_voices = VoiceTable(self.voices, max_voices)
        self._prompt_audio = PromptAudioCache(prompt_audio_cache)
        self._encoder_lock = threading.Lock()
        self._encoder_path, self._encoder_samples = encoder, int(round(float(prompt_audio_seconds) * 24000))
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
        for name, d in dict(voices or {}).items():          # a voice directory's speaker embedding, when it has one
            emb = load_voice_speaker(d, self._hidden)
            if emb is not None:
                self.runtime_voices.set_startup_speaker(name, emb)
        self.eng = FrameEngine(model_path, max_batch=max_batch, n_ctx=n_ctx, max_frames=max_tokens)
        self.eng.set_pad_embed(self.front.tts_pad_embed)
        self.eng.set_sampling(temperature, top_k, top_p, cp_temperature, cp_top_k, seed)
        self._lib = hiplib.load()
        self.voc = Vocoder(vocoder_path, 64, min(max_batch, 32))
        if encoder:
            from .encoder import Encoder
            self.encoder = Encoder(encoder, max_batch=min(max_batch, 4), max_samples=self._encoder_samples)
        if speaker_encoder:
            from .speaker import SpeakerEncoder
            self.speaker = SpeakerEncoder(speaker_encoder, max_batch=min(max_batch, 4), max_samples=self._encoder_samples)
            if self.speaker.dim != self._hidden or self.speaker.sample_rate != 24000:
                dim, rate = self.speaker.dim, self.speaker.sample_rate
                self.speaker.close()
                raise ValueError(f"--speaker_encoder gives {dim} values at {rate} Hz, the model takes {self._hidden} at 24000 Hz")
        # --voice_warm N: N snapshot slots on the vocoder handle, and the LRU over them (the vocoder worker's, like the handle)
        self._voice_warm = VoiceWarmCache(int(voice_warm))
        if self._voice_warm.n_slots:
            self.voc.snapshots(self._voice_warm.n_slots)
        self.pipeline = bool(pipeline)
        self._pool = self._stream_pool = None   # (_stream_pool: the push worker of streamed requests when there is no pipeline's)
        self._vstream = None           # streaming chunk walk: one stream per slot of the frame loop
        self._istreams = {}            # carry-state incremental decode: one object per arithmetic, made by the worker on first use
        if self.pipeline:
            self._pool = ThreadPoolExecutor(max_workers=1)       # ONE worker: the vocoder handle has one caller, replies keep their order
            self._lib.voc_set_max_workgroups(-1)
        self._running = True
        if install_signal_handlers:
            signal.signal(signal.SIGINT, self._signal_handler)
            signal.signal(signal.SIGTERM, self._signal_handler)

    _hidden = property(lambda self: len(self.front.tts_pad_embed))   # the model's hidden size: what a speaker embedding must have

    def _signal_handler(self, signum, frame):
        self._running = False

    def _token_ids(self, msg):
        if msg.get("token_ids") is not None:
            return [[int(x) for x in ids] for ids in msg["token_ids"]]
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer configured (--tokenizer DIR) and the request has no token_ids")
        return [self.tokenizer.encode(t, add_special_tokens=False) for t in msg.get("texts", [])]

    def _queue(self, token_ids, max_tokens, speakers=None):
        """A request's prefixes -> (prefixes, n_text, max_tokens, order): order[k] = request index of the queue's k-th utterance.
        speakers (one float32 [hidden] or None per utterance): the speaker row of its prefix."""
        B = len(token_ids)
        if B == 0:
            raise ValueError("a request needs at least one utterance")
        if B > self.max_request:
            raise ValueError(f"a request may carry at most {self.max_request} utterances (got {B})")
        max_tokens = min(int(max_tokens or self.max_tokens), self.max_tokens)
        speakers = speakers or [None] * B
        prefixes = [self.front.build_prefix(ids, speaker=spk) for ids, spk in zip(token_ids, speakers)]
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
        that mode carries.  prompts (one [T][16] array or None per utterance): the codec prompts, as batch_request says."""
        if vocoder == "incremental":
            out = []
            for c, pr in zip(cs, prompts or [None] * len(cs)):
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
        if state.vocoder != "incremental":
            for b in resets:
                self._vstream.reset(b)
            return self._vstream.push([e.slot for e in entries], [e.frames for e in entries],
                                      [e.finished for e in entries]) if entries else []
        arithmetic = state.arithmetic
        if arithmetic not in self._istreams:
            self._istreams[arithmetic] = self.voc.incremental(self.max_batch, arithmetic)
        istream = self._istreams[arithmetic]
        ch = self.voc.chunk_tokens
        drop = state.drop                      # samples of a slot's prompt that are still to be dropped from what it hands out
        for b in resets:
            drop.pop(b, None)
        # a slot that continues a prompt: the prompt's frames first, in pieces of at most chunk_tokens frames, none of their
        # samples going out -- or, with --voice_warm, the state those pushes leave, copied from the voice's snapshot
        prompts = {b: state.prompts.pop(b, None) for b in resets}
        drop.update(self._voice_warm.start(istream, arithmetic, resets, prompts, ch, self.voc.incremental_samples))
        parts, j = [[] for _ in entries], 0
        while entries and (j == 0 or any(len(e.frames) > j * ch for e in entries)):
            sel = [(k, e) for k, e in enumerate(entries) if j == 0 or len(e.frames) > j * ch]
            pcm = istream.push([e.slot for _, e in sel], [e.frames[j * ch:(j + 1) * ch] for _, e in sel],
                               [e.finished and len(e.frames) <= (j + 1) * ch for _, e in sel])
            for (k, _), a in zip(sel, pcm):
                parts[k].append(a.copy())
            j += 1
        out = [np.concatenate(p) for p in parts]
        for k, e in enumerate(entries):
            left = drop.get(e.slot, 0)
            if left > 0:
                drop[e.slot] = left - min(left, len(out[k]))
                out[k] = out[k][left:]
        return out

    def _push(self, conn, state, resets, entries):
        """Worker side of a streamed request (state: its ReplyState, entries: PushEntry): start the refilled slots' streams, push
        the new frames, send the PCM that became final and the end records."""
        if state.failed:
            return
        try:
            pcm = self._stream_pcm(state, resets, entries)
            out = []
            for entry, a in zip(entries, pcm):
                if len(a):
                    out.append(pack_stream_audio(entry.utt, a))
                if entry.finished:
                    if state.logprobs:                    # (the engine thread wrote them before it submitted this push)
                        out.append(pack_stream_scores(entry.utt, state.utt_scores[entry.utt]))
                    out.append(pack_stream_end(entry.utt, entry.codes))
            if out:
                conn.sendall(b"".join(out))
        except Exception as e:
            state.failed = True
            print(f"Error: {e}")
            self._send_error(conn)

    def _close_stream(self, conn, state, t0):
        """Worker side: the last record of a streamed request, then its connection closes."""
        try:
            if not state.failed:
                conn.sendall(P.pack_sentinel(P.SENTINEL_DONE))
                print(f"  {state.n} utterances, {state.frames} frames streamed in {time.time() - t0:.3f}s{self._prefix_note()}"
                      f"{self._logprob_note(state)}")
        except OSError:
            pass
        finally:
            conn.close()

    def synthesize_stream(self, conn, token_ids, max_tokens=None, t0=None, vocoder="walk", arithmetic="exact"):
        """A streamed request: the frame loop runs here (generate_queue), the vocoder's pushes and every write to `conn` on the
        worker thread, at most one push in flight.  -> the worker's future of the request's last record (it closes conn)."""
        t0 = time.time() if t0 is None else t0
        state = ReplyState(len(token_ids), vocoder, arithmetic)
        if self._pool is None and self._stream_pool is None:
            self._stream_pool = ThreadPoolExecutor(max_workers=1)
        pool = self._pool if self._pool is not None else self._stream_pool
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
                resets = [b for b, o in enumerate(owner) if o is not None and slot_utt[b] != o]
                for b in resets:
                    slot_utt[b], pushed[b] = owner[b], 0
                entries = new_entries(codes, per, [(b, order[o]) for b, o in enumerate(owner) if o is not None], pushed, ended)
                state.frames += sum(len(e.codes) for e in entries if e.finished)
                if not (resets or entries):
                    return
                if fut is not None:
                    fut.result()                         # one push in flight
                if state.failed:
                    raise RuntimeError("streamed request failed on the vocoder side")
                fut = pool.submit(self._push, conn, state, resets, entries)

            self.eng.generate_queue([prefixes[i] for i in order], [n_text[i] for i in order], max_tokens, on_frames=on_frames)
        except Exception as e:
            if fut is not None:
                fut.result()
            if not state.failed:
                print(f"Error: {e}")
                state.failed = True
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
        """--concurrent, accept side: a request -> its Utterances in queue order, each with its prefix key (and its codec
        prompt, if it has one); raises on anything malformed, before any of it is queued."""
        request_vocoder_arithmetic(msg)      # (checks "vocoder" too)
        base = request_slot_params(msg, self.defaults, self.max_tokens)
        rules = request_slot_rules(msg, self.sampler_rules)
        request_logprobs(msg, self.logprobs)
        if rules is not None and not rules.is_default():
            print(f"  sampler rules: {rules}")
        prompted = request_has_prompt(msg)
        if msg.get("text_stream"):
            if prompted or request_has_speaker(msg):
                self._check_text_voice(msg)
            return [dataclasses.replace(self._prepare_text_stream(msg, base), rules=rules)]
        ids = self._token_ids(msg)
        prompts = [None] * len(ids)
        speakers = self._request_speakers(msg, len(ids))
        if prompted:     # a codec prompt: its text (if any) in front of every utterance's, its frames behind every prefix
            prompts, head = self._request_prompts(msg, len(ids))
            ids = [head + u for u in ids]
        prefixes, n_text, max_tokens, order = self._queue(ids, base.max_frames, speakers)
        for i in order if prompted else ():
            rows = prefixes[i].shape[0] + len(prompts[i])
            if rows + max_tokens > self.n_ctx or rows > max(self.max_batch, 2048):
                raise ValueError("prefix + codec prompt + max_tokens exceed n_ctx (or the rows of one prefill pass)")
        return [Utterance(i, prefixes[i], n_text[i], dataclasses.replace(base, max_frames=max_tokens, utt=i),
                          prefix_key=prefix_key(b"prompt", ids[i], prompts[i], speakers[i]) if prompted and len(prompts[i]) else
                          prefix_key(b"full", ids[i], speaker=speakers[i]), prompt=prompts[i], rules=rules) for i in order]

    def _check_text_voice(self, msg):
        if msg.get("text_stream") and not self.text_voice:
            if not request_has_prompt(msg):
                raise ValueError('a speaker embedding does not combine with "text_stream"')
            raise ValueError('a codec prompt does not combine with "text_stream"')

    def _request_speakers(self, msg, n_utts):
        """A request's speaker embeddings -> one float32 [hidden] (or None) per utterance: "speaker_embedding", else the
        embedding kept with its "voice" unless "speaker" is "off".  By now a "prompt_audio" request's "speaker" has become
        "speaker_embedding" (_resolve_prompt_audio): "only" / "with_prompt" still standing here have no clip to come from."""
        mode = request_speaker_mode(msg)
        if mode != "off":
            raise ValueError(f'"speaker": "{mode}" needs "prompt_audio" (and a server started with --speaker_encoder)')
        if msg.get("speaker_embedding") is not None:
            return request_speaker_embedding(msg["speaker_embedding"], n_utts, self._hidden)
        name = msg.get("voice")
        if isinstance(name, str) and msg.get("speaker") != "off" and self.runtime_voices is not None:
            emb = self.runtime_voices.speaker(name)
            if emb is not None:
                return [emb] * n_utts
        return [None] * n_utts

    def _request_prompts(self, msg, n_utts):
        """A request's codec prompt -> (one [T][16] int32 array per utterance, the prompt text's token ids): from "prompt_codes"
        and "prompt_token_ids" / "prompt_text", or from the "voice" that names them; raises ValueError on anything malformed."""
        self._check_text_voice(msg)
        codes, text, head = msg.get("prompt_codes"), msg.get("prompt_text"), msg.get("prompt_token_ids")
        if msg.get("voice") is not None:
            if codes is not None or text is not None or head is not None:
                raise ValueError('"voice" stands for "prompt_codes" and the prompt text: give one or the other')
            name = msg["voice"]
            entry = self.voices.get(name) if isinstance(name, str) else None
            if entry is None and isinstance(name, str) and self.runtime_voices is not None:
                entry = self.runtime_voices.get(name)           # (registered at run time: "register_voice")
            if entry is None:
                raise ValueError(f"unknown voice {name!r}")
            codes, text = entry
            if isinstance(text, list):                          # (registered with "prompt_token_ids")
                head, text = text, None
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
        """A "text_stream" request -> its one Utterance (0, streaming prefix, 0, SlotParams of a text slot, TextFeed), whose
        prefix key covers the first token alone; with a codec prompt as the module docstring says under `--text_voice`."""
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
        (spk,) = self._request_speakers(msg, 1)
        own = 8 if spk is None else 9                  # rows of the streaming prefix (one more with a speaker row)
        if request_has_prompt(msg):
            (prompt,), head = self._request_prompts(msg, 1)
            rows = own + len(head) + len(prompt)
            if rows + base.max_frames > self.n_ctx or rows > max(self.max_batch, 2048):
                raise ValueError("prefix + codec prompt + max_tokens exceed n_ctx (or the rows of one prefill pass)")
        if own + base.max_frames > self.n_ctx:
            raise ValueError("prefix + max_tokens exceed n_ctx")
        feed = TextFeed(lambda ids, final=False: text_stream_rows(self.front, ids, final), encoder,
                        None if self.tokenizer is None else self.tokenizer.incremental, first[1:], 1 + len(head))
        params = dataclasses.replace(base, utt=0, text_stream=True, text_after_prompt=prompt is not None)
        return Utterance(0, self.front.build_prefix_stream(first[0], head, speaker=spk), 0, params, feed,
                         prefix_key(b"stream", head + first[:1], prompt, spk), prompt)

    def _prefix_note(self):
        """The prefix cache's and the voice warm-ups' counters so far, for the per-request line ("" without the flags)."""
        note = ""
        if self.prefix_cache and self.sched is not None:
            note = f" (prefix cache: {self.sched.prefix_hits} hits, {self.sched.prefix_misses} misses so far)"
        if self.encoder is not None:
            note += f" (prompt audio: {self._prompt_audio.hits} hits, {self._prompt_audio.misses} misses so far)"
        return note + self._voice_warm.note()

    prompt_audio_hits = property(lambda self: self._prompt_audio.hits)
    prompt_audio_misses = property(lambda self: self._prompt_audio.misses)
    prompt_audio_evictions = property(lambda self: self._prompt_audio.evictions)

    def _resolve_prompt_audio(self, conn, msg):
        """Accept side, --concurrent: a request with "prompt_audio" / "register_voice" becomes the request with "prompt_codes"
        equal to the encoder's ids -- the descriptors checked from the JSON alone, then the payload read from conn, the clips
        looked up in the id cache and the missing ones encoded (one library call per format / channels / rate).  -> True when
        the request only registered a voice and has been answered; raises on anything malformed (the caller answers -2)."""
        spec, name = msg.get("prompt_audio"), msg.get("register_voice")
        if self.encoder is None:
            raise ValueError('"prompt_audio" needs a server started with --encoder')
        if spec is None:
            raise ValueError('"register_voice" needs "prompt_audio"')
        if msg.get("prompt_codes") is not None or msg.get("voice") is not None:
            raise ValueError('"prompt_audio" takes the place of "prompt_codes" / "voice": give one')
        mode = request_speaker_mode(msg)           # where the speaker embedding comes from: "off" (none), the clip alone, or both
        if mode != "off":
            if self.speaker is None:
                raise ValueError('"speaker" needs a server started with --speaker_encoder')
            if msg.get("speaker_embedding") is not None:
                raise ValueError('"speaker" takes the embedding from the clip: it does not combine with "speaker_embedding"')
            if mode == "only" and name is not None:
                raise ValueError('"speaker": "only" keeps no codec prompt: it does not combine with "register_voice"')
        utts = msg["token_ids"] if msg.get("token_ids") is not None else msg.get("texts", [])
        if not isinstance(utts, list):
            raise ValueError("texts / token_ids is a list")
        if name is not None:
            if isinstance(spec, list):
                raise ValueError('"register_voice" takes a single "prompt_audio" object')
            self.runtime_voices.check_register(name)
        elif not utts:
            raise ValueError("a request needs at least one utterance")
        descs, shared = request_prompt_audio(spec, len(utts), self._encoder_samples)
        if mode != "off":
            for d in descs:
                if d.samples_24k < self.speaker.min_samples:
                    raise ValueError(f'"prompt_audio": {d.samples_24k} samples at 24 kHz, the speaker encoder needs {self.speaker.min_samples}')
        want_ids, want_spk = mode != "only", mode != "off"
        payloads = [P.recv_payload(conn, d.nbytes) for d in descs]
        keys = [prompt_audio_digest(d, raw) for d, raw in zip(descs, payloads)]
        ids, embs, missing, missing_spk = [None] * len(descs), [None] * len(descs), {}, {}
        for k, (d, key) in enumerate(zip(descs, keys)):
            first = next((j for j in range(k) if keys[j] == key), None)
            if first is not None:                  # (a clip the request repeats: encoded and embedded once, below)
                continue
            ids[k], embs[k] = self._prompt_audio.lookup(key, want_ids, want_spk)
            if want_ids and ids[k] is None:
                missing.setdefault((d.format, d.channels, d.rate), []).append(k)
            if want_spk and embs[k] is None:
                missing_spk.setdefault((d.format, d.channels, d.rate), []).append(k)
        for (fmt, channels, rate), ks in missing.items():
            with self._encoder_lock:
                got = self.encoder.encode_pcm([descs[k].array(payloads[k]) for k in ks], rate, channels)
            for k, c in zip(ks, got):
                ids[k] = np.ascontiguousarray(c[:descs[k].max_frames], np.int64)
                self._prompt_audio.put(keys[k], ids[k])
        for (fmt, channels, rate), ks in missing_spk.items():
            with self._encoder_lock:               # the front-end's own 24 kHz samples, then the speaker encoder
                samples = self.encoder.resample_pcm([descs[k].array(payloads[k]) for k in ks], rate, channels)
                got = self.speaker.embed(samples)
            for k, e in zip(ks, got):
                embs[k] = np.ascontiguousarray(e, np.float32)
                self._prompt_audio.put(keys[k], speaker=embs[k])
        for k in range(len(descs)):
            j = keys.index(keys[k])
            ids[k], embs[k] = ids[j], embs[j]
        del msg["prompt_audio"]
        msg.pop("register_voice", None)
        msg.pop("speaker", None)
        if want_ids:
            msg["prompt_codes"] = ids[0].tolist() if shared else [c.tolist() for c in ids]
        if want_spk:
            msg["speaker_embedding"] = embs[0].tolist() if shared else [e.tolist() for e in embs]
        if name is not None:
            text = msg.get("prompt_token_ids") if msg.get("prompt_token_ids") is not None else msg.get("prompt_text")
            self._request_prompts(dict(msg, text_stream=False), 1)      # (the checks a later "voice" request would fail)
            self.runtime_voices.register(name, msg["prompt_codes"], text, speaker=embs[0] if want_spk else None)
            print(f"  voice {name!r} registered: {len(ids[0])} frames")
            if not utts:
                conn.sendall(struct.pack("<i", 0))
                conn.close()
                return True
        return False

    voice_warm_hits = property(lambda self: self._voice_warm.hits)
    voice_warm_misses = property(lambda self: self._voice_warm.misses)
    voice_warm_evictions = property(lambda self: self._voice_warm.evictions)

    @staticmethod
    def _logprob_note(state):
        """The per-request line of a "logprobs" request: the mean log-probability of code_0 over each utterance's frames."""
        if not state.logprobs or state.utt_scores is None:
            return ""
        means = [float(np.mean(s[:, 0])) if s is not None and len(s) else float("nan") for s in state.utt_scores]
        return ", mean logprob " + " ".join(f"{m:.3f}" for m in means)

    def _finish(self, conn, cs, t0, state):
        """Worker side of an unstreamed reply (--pipeline, --concurrent): vocode as `state` says, reply on conn, close it."""
        try:
            res = self.vocode(cs, state.vocoder, state.arithmetic, state.utt_prompts)
            conn.sendall(pack_batch_reply(res, state.utt_scores if state.logprobs else None))
            print(f"  {len(res)} utterances, {sum(len(c) for c, _ in res)} frames in {time.time() - t0:.3f}s{self._prefix_note()}"
                  f"{self._logprob_note(state)}")
        except Exception as e:
            print(f"Error: {e}")
            self._send_error(conn)
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
                if request_has_speaker(msg):
                    raise ValueError("a speaker embedding needs a --concurrent server")
                request_slot_rules(msg, False)
                request_logprobs(msg, False)
                if msg.get("stream"):
                    # streamed reply: the worker writes every record and closes the connection
                    ids = self._token_ids(msg)
                    handed_over = True
                    self.synthesize_stream(conn, ids, msg.get("max_tokens"), t0, vocoder, arithmetic)
                    continue
                if self._pool is not None:
                    # pipelined: this request's vocoder runs on the worker while the loop accepts and generates the next one
                    cs = self.generate(self._token_ids(msg), msg.get("max_tokens"))
                    self._pool.submit(self._finish, conn, cs, t0, ReplyState(len(cs), vocoder, arithmetic))
                    handed_over = True
                    continue
                res = self.synthesize(self._token_ids(msg), msg.get("max_tokens"), vocoder, arithmetic)
                conn.sendall(pack_batch_reply(res))
                print(f"  {len(res)} utterances, {sum(len(c) for c, _ in res)} frames in {time.time() - t0:.3f}s")
            except Exception as e:  # like the reference's servers: report, send the error sentinel, keep serving
                print(f"Error: {e}")
                self._send_error(conn)
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
        if self.sampler_rules:
            self.eng.rules()                     # the rules entry and the emitted-id set of every slot: arguments of the frame
        if self.logprobs:
            self.eng.scores_reserve()            # one f32 beside every id of the codes: an argument of the frame's sampling launches
        self.sched = ConcurrentScheduler(self.eng, self.max_batch, self.max_queue, self._prepare, self._finish, self._push,
                                         self._close_stream, self._send_error, check_every=self.check_every,
                                         send_timeout=self.send_timeout, text_wait_ms=self.text_wait_ms,
                                         text_hold=self.text_hold, prefix_cache=bool(self.prefix_cache), logprobs=self.logprobs)
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
                    if msg.get("prompt_audio") is not None or msg.get("register_voice") is not None:
                        if self._resolve_prompt_audio(conn, msg):     # (reads the payload behind the JSON)
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
        if self.speaker is not None:
            self.speaker.close()
            self.speaker = None
        if self.encoder is not None:
            self.encoder.close()
            self.encoder = None
        self.voc.close()               # frees the streaming chunk walk first
        self._vstream, self._istreams = None, {}
        self.eng.destroy()


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
    ap.add_argument("--sampler_rules", action="store_true",
                    help="--concurrent: requests may set their sampler rules (repetition_penalty, repetition_window, eos_boost, "
                         "eos_force, min_tokens, cp_top_p, sampler: reference / upstream)")
    ap.add_argument("--logprobs", action="store_true",
                    help="--concurrent: requests may ask for the log-probability of every id of their reply (\"logprobs\": true)")
    ap.add_argument("--voice", action="append", default=[], metavar="NAME=DIR",
                    help="--concurrent: a codec prompt requests may name with \"voice\": \"NAME\"; DIR as "
                         "encode_reference_audio --output_dir writes it (repeatable)")
    ap.add_argument("--voice_warm", type=int, default=0,
                    help="with --concurrent: cache the incremental vocoder's warm-up per codec prompt in N snapshot slots of the "
                         "vocoder (a known voice then costs one copy launch instead of decoding its prompt; default 0 = off)")
    ap.add_argument("--encoder", default=None,
                    help="--concurrent: speech-tokenizer encoder container; requests may then carry their codec prompt as audio "
                         "(\"prompt_audio\" + the raw PCM behind the JSON), encoded on the GPU")
    ap.add_argument("--prompt_audio_seconds", type=float, default=20.0, help="--encoder: the longest audio prompt, in seconds")
    ap.add_argument("--prompt_audio_cache", type=int, default=16,
                    help="--encoder: entries of the LRU of encoded audio prompts (a repeated clip runs no encode)")
    ap.add_argument("--speaker_encoder", default=None,
                    help="--concurrent --encoder: speaker-encoder container; a \"prompt_audio\" request may then carry \"speaker\": "
                         "\"with_prompt\" / \"only\" and gets the clip's x-vector as one more prefix row")
    ap.add_argument("--max_voices", type=int, default=64, help="--encoder: voices \"register_voice\" may keep at run time")
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
                               voice_warm=a.voice_warm, sampler_rules=a.sampler_rules, encoder=a.encoder,
                               prompt_audio_seconds=a.prompt_audio_seconds, prompt_audio_cache=a.prompt_audio_cache,
                               max_voices=a.max_voices, logprobs=a.logprobs, speaker_encoder=a.speaker_encoder)
    try:
        srv.serve()
    finally:
        srv.close()


if __name__ == "__main__":
    main()
