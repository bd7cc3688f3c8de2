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

Every check_every frames the new frames of every live slot go to the vocoder's streaming chunk walk (voc_stream_push, on one
worker thread with one vocoder workgroup per compute unit, as in --pipeline); a full 64-frame chunk is decoded as soon as its
frames exist, and all samples no later cross-fade can change go out at once.  An utterance's PCM records joined, and its codes,
are bit for bit what the unstreamed reply carries.

`--pipeline`: the vocoder of request k runs on a worker thread (and replies on k's connection) while the frame loop of request
k + 1 already runs -- the reference's client does the same per 64-frame block of ONE utterance (tts_client.py:188-197).  The
vocoder then launches one persistent workgroup per compute unit (voc_set_max_workgroups(-1)), which leaves the frame loop's
workgroups room beside it (244 -> 209 ms per 32 x 64-frame step); results are bit-identical.
"""
from __future__ import annotations

import argparse
import os
import signal
import socket
import struct
import time

import numpy as np

from . import hiplib
from . import protocol as P
from .engine import FrameEngine
from .frontend import TextFrontEnd
from .weights import ModelConfig, read_pack


class BatchSynthesisServer:
    def __init__(self, model_path, vocoder_path, socket_path="/tmp/qwen3_batch.sock", max_batch=32, n_ctx=512,
                 max_tokens=200, temperature=0.0, top_k=50, cp_temperature=0.0, tokenizer=None, seed=0,
                 install_signal_handlers=True, max_request=None, pipeline=False):
        self.socket_path, self.max_batch, self.max_tokens = socket_path, max_batch, max_tokens
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
        self.eng.set_sampling(temperature, top_k, 0.95, cp_temperature, top_k, seed)
        self.n_ctx = n_ctx
        self._lib = hiplib.load()
        self.voc = self._lib.voc_load(str(vocoder_path).encode(), 64, min(max_batch, 32))
        if not self.voc:
            raise RuntimeError(f"voc_load failed: {vocoder_path}")
        self.pipeline = bool(pipeline)
        self._pool = None
        self._stream_pool = None       # the push worker of streamed requests (the pipeline's worker when there is one)
        self._vstream = None           # streaming chunk walk: one stream per slot of the frame loop
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

    def vocode(self, cs):
        """The vocoder of a request: every utterance's chunk walk in ONE batched call (voc_synthesize_batch: chunks of all
        utterances decoded together, overlap-crossfade assembled on the device; per utterance = VocoderServer.synthesize +
        int16) -> list of (codes, pcm int16)."""
        B = len(cs)
        live = [b for b in range(B) if cs[b].shape[0] > 0]
        pcm = {b: np.zeros(0, np.int16) for b in range(B)}
        if live:
            n = np.array([cs[b].shape[0] for b in live], np.int32)
            cat = np.ascontiguousarray(np.concatenate([cs[b] for b in live], axis=0), dtype=np.int64)
            cap = int(self._lib.voc_synthesize_batch_max_samples(self.voc, hiplib.iptr(n), len(n)))
            buf = np.empty(cap, np.int16)
            off = np.zeros(len(n) + 1, np.int64)
            if self._lib.voc_synthesize_batch(self.voc, cat.ctypes.data_as(hiplib.i64p), hiplib.iptr(n), len(n),
                                              buf.ctypes.data_as(hiplib.i16p), cap, off.ctypes.data_as(hiplib.i64p)) != 0:
                raise RuntimeError("voc_synthesize_batch failed")
            for k, b in enumerate(live):
                pcm[b] = buf[off[k]:off[k + 1]].copy()
        return [(cs[b], pcm[b]) for b in range(B)]

    def synthesize(self, token_ids, max_tokens=None):
        """-> list of (codes int32 [n_frames][16], pcm int16) per utterance."""
        return self.vocode(self.generate(token_ids, max_tokens))

    def _push(self, conn, state, resets, entries):
        """Worker side of a streamed request: start the refilled slots' streams, push every live slot's new frames to the
        streaming chunk walk, send the PCM that became final and the end records.  entries: (slot, utt, new frames,
        finished, all codes of the utterance when finished)."""
        if state["failed"]:
            return
        try:
            lib, vs = self._lib, self._vstream
            for b in resets:
                if lib.voc_stream_reset(vs, b) != 0:
                    raise RuntimeError("voc_stream_reset failed")
            if entries:
                streams = np.array([e[0] for e in entries], np.int32)
                n_new = np.array([e[2].shape[0] for e in entries], np.int32)
                fin = np.array([int(e[3]) for e in entries], np.int32)
                cat = np.ascontiguousarray(np.concatenate([e[2] for e in entries], axis=0), dtype=np.int64).reshape(-1, 16)
                args = (vs, len(entries), hiplib.iptr(streams))
                cap = int(lib.voc_stream_push_max_samples(*args, hiplib.iptr(n_new), hiplib.iptr(fin)))
                if cap < 0:
                    raise RuntimeError("voc_stream_push: invalid push")
                buf = np.empty(max(cap, 1), np.int16)
                off = np.zeros(len(entries) + 1, np.int64)
                if lib.voc_stream_push(*args, cat.ctypes.data_as(hiplib.i64p), hiplib.iptr(n_new), hiplib.iptr(fin),
                                       buf.ctypes.data_as(hiplib.i16p), cap, off.ctypes.data_as(hiplib.i64p)) != 0:
                    raise RuntimeError("voc_stream_push failed")
                out = []
                for k, (_, utt, _, finished, codes) in enumerate(entries):
                    if off[k + 1] > off[k]:
                        out.append(pack_stream_audio(utt, buf[off[k]:off[k + 1]]))
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
                print(f"  {state['n']} utterances, {state['frames']} frames streamed in {time.time() - t0:.3f}s")
        except OSError:
            pass
        finally:
            conn.close()

    def synthesize_stream(self, conn, token_ids, max_tokens=None, t0=None):
        """A streamed request: the frame loop runs here (generate_queue), the vocoder's pushes and every write to `conn` on the
        worker thread, at most one push in flight.  -> the worker's future of the request's last record (it closes conn)."""
        t0 = time.time() if t0 is None else t0
        state = {"failed": False, "n": len(token_ids), "frames": 0}
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
                self._vstream = self._lib.voc_stream_create(self.voc, self.max_batch)
                if not self._vstream:
                    raise RuntimeError("voc_stream_create failed")
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

    def _finish(self, conn, cs, t0):
        """Worker side of the pipelined mode: vocode, reply on the request's own connection, close it."""
        try:
            res = self.vocode(cs)
            conn.sendall(pack_batch_reply(res))
            print(f"  {len(res)} utterances, {sum(len(c) for c, _ in res)} frames in {time.time() - t0:.3f}s")
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
        sock.listen(1)
        sock.settimeout(1.0)
        os.chmod(self.socket_path, 0o666)
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
                if msg.get("stream"):
                    # streamed reply: the worker writes every record and closes the connection
                    ids = self._token_ids(msg)
                    handed_over = True
                    self.synthesize_stream(conn, ids, msg.get("max_tokens"), t0)
                    continue
                if self._pool is not None:
                    # pipelined: this request's vocoder runs on the worker while the loop accepts and generates the next one
                    cs = self.generate(self._token_ids(msg), msg.get("max_tokens"))
                    self._pool.submit(self._finish, conn, cs, t0)
                    handed_over = True
                    continue
                res = self.synthesize(self._token_ids(msg), msg.get("max_tokens"))
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

    def close(self):
        self._running = False
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        self._stream_pool = None       # the push worker of streamed requests (the pipeline's worker when there is one)
        self._vstream = None           # streaming chunk walk: one stream per slot of the frame loop
        if self.pipeline:
            self._lib.voc_set_max_workgroups(0)
        if self.voc:
            self._lib.voc_free(self.voc)
            self.voc = None
        self.eng.destroy()


def pack_batch_request(texts=None, token_ids=None, language="russian", max_tokens=None, stream=False) -> bytes:
    import json
    msg = {"language": language}
    if stream:
        msg["stream"] = True
    if token_ids is not None:
        msg["token_ids"] = [[int(t) for t in ids] for ids in token_ids]
    else:
        msg["texts"] = list(texts)
    if max_tokens:
        msg["max_tokens"] = int(max_tokens)
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


def synthesize_batch_stream(socket_path, texts=None, token_ids=None, language="russian", max_tokens=None):
    """Client side of the streamed request: yields its records as they arrive -- ("audio", utt, pcm) and ("end", utt, codes)
    -- until the request is done; raises on the error sentinel."""
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.connect(socket_path)
    try:
        s.sendall(pack_batch_request(texts, token_ids, language, max_tokens, stream=True))
        while True:
            rec = read_stream_record(s)
            if rec[0] == "done":
                return
            yield rec
    finally:
        s.close()


def synthesize_batch(socket_path, texts=None, token_ids=None, language="russian", max_tokens=None):
    """Client side of the batched request."""
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.connect(socket_path)
    try:
        s.sendall(pack_batch_request(texts, token_ids, language, max_tokens))
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
    ap.add_argument("--pipeline", action="store_true",
                    help="vocode request k on a worker thread while request k + 1 generates (one vocoder workgroup per CU)")
    a = ap.parse_args()
    srv = BatchSynthesisServer(a.model, a.vocoder, a.socket, a.max_batch, a.n_ctx, a.max_tokens, a.temperature, a.top_k,
                               a.cp_temperature, a.tokenizer, a.seed, pipeline=a.pipeline)
    try:
        srv.serve()
    finally:
        srv.close()


if __name__ == "__main__":
    main()
