"""The scheduler of batch_server --concurrent: utterances of different requests share ONE running frame loop.

An accept thread reads and checks every request (a malformed one, or one that would take the queue past max_queue
utterances, gets -2 at once) and queues its utterances; the engine thread -- the only caller of the engine -- opens max_batch slots once (q3e_open) and every check_every
frames admits queued utterances into free slots (FIFO across requests; within a request longest first), each with
its own frame budget (the request's max_tokens), sampling settings and seed (q3e_admit), runs the loop, polls which slots
ended, and releases the slots of a client that went away; one vocoder worker -- the only caller of the vocoder -- streams the
new frames of streamed requests (one voc_stream per slot, reset on admission) and answers an unstreamed request with one
voc_synthesize_batch over its utterances once its last one ended.

Determinism contract: a request's reply, codes and PCM, depends only on the request, its seed and the server's configuration -- not on what else is in flight nor on which slots it gets.  The loop always steps max_batch rows (a
row's f32 sums depend on the row count of the pass), every utterance is prefilled in a pass of its own (the ragged prefill's
tiles depend on the rows of the pass), and utterance u of a request with seed s draws from the stream mix(s, u), keyed by
(stream, frame, group) and not by the slot (include/qwen3tts_engine.h).  With `--prefix_cache N` a reply is, bit for bit, the
reply without it.

Streamed text (batch_wire has the records): the utterance runs in a text slot of the frame loop (include/qwen3tts_engine.h,
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
"""
from __future__ import annotations

import collections
import dataclasses
import select
import socket
import struct
import threading
import time
import typing

import numpy as np

from . import protocol as P
from .batch_request import request_logprobs, request_vocoder, request_vocoder_arithmetic


@dataclasses.dataclass
class ReplyState:
    """What the engine side and the vocoder worker share about one request's reply."""
    n: int                          # utterances of the request
    vocoder: str = "walk"
    arithmetic: str = "exact"
    failed: bool = False            # the worker sets it (the engine thread too, when it fails the request); the engine thread reads it
    frames: int = 0                 # frames of the utterances that have ended: the engine thread writes it
    prompts: dict = dataclasses.field(default_factory=dict)   # by slot: set by the engine thread on admission, popped by the reset's push
    drop: dict = dataclasses.field(default_factory=dict)      # by slot: samples of a prompt still to drop; the worker's alone
    utt_prompts: list = None        # codec prompts per request index (None: none), for the unstreamed reply
    logprobs: bool = False          # the request asked for the log-probabilities of its ids
    utt_scores: list = None         # with logprobs: float32 [frames][16] per request index, written by the engine thread as each
                                    # utterance ends, before the push that ends it (or its reply) is submitted to the worker


class PushEntry(typing.NamedTuple):
    """What one slot hands to a push: its new frames, and all codes of its utterance once it has finished."""
    slot: int
    utt: int
    frames: np.ndarray
    finished: bool
    codes: np.ndarray


def new_entries(codes, per, slots, pushed, finished):
    """What is new since the last check in `slots`, (slot, utt) pairs: an entry for every slot that has frames beyond
    pushed[slot] or is in `finished`; pushed is brought up to date.  codes [frames][B][16], per[slot] = frames so far."""
    entries = []
    for b, utt in slots:
        n, fin = int(per[b]), b in finished
        if n > pushed[b] or fin:
            whole = np.ascontiguousarray(codes[:n, b, :], dtype=np.int32) if fin else None
            entries.append(PushEntry(b, utt, np.ascontiguousarray(codes[pushed[b]:n, b, :]), fin, whole))
            pushed[b] = n
    return entries


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

    def __init__(self, conn, items, stream, t0, vocoder, arithmetic, logprobs=False):
        self.conn, self.stream, self.t0 = conn, bool(stream), t0
        self.n = self.left = len(items)         # (left: utterances that have not ended)
        self.codes = [None] * self.n            # per request index
        prompts = {it.utt: it.prompt for it in items}
        self.state = ReplyState(self.n, vocoder, arithmetic, logprobs=bool(logprobs))
        if logprobs:
            self.state.utt_scores = [None] * self.n
        if any(p is not None for p in prompts.values()):
            self.state.utt_prompts = [prompts.get(i) for i in range(self.n)]
        self.gone = False                       # the client went away or the request failed: its slots are released
        self.feed = next((it.feed for it in items if it.feed is not None), None)   # TextFeed of a "text_stream" request
        self.starved_since = None               # text_hold: since when its slot has been held (None: it is not)


class ConcurrentScheduler:
    """The engine and vocoder sides of `--concurrent` (module docstring).  `eng` has the FrameEngine surface open / admit /
    release / run / done / codes; the callables are the server's: prepare(msg) -> [batch_request.Utterance] in queue order
    (raises on a malformed request), reply(conn, codes per utterance, t0, state) answers and closes an unstreamed request,
    push(conn, state, resets, entries) and close_stream(conn, state, t0) stream records and end a streamed one (state: the
    request's ReplyState, entries: PushEntry), send_error(conn) writes -2.

    A client is gone once it has closed its connection (POLLHUP); a client that only shuts down its sending side after the
    request (shutdown(SHUT_WR)) still gets its reply.  Every write to a request's connection is bounded by send_timeout
    seconds (SO_SNDTIMEO): a client that stays connected but stops reading fails its own request -- the writer's error marks
    it failed, the engine then releases its slots -- instead of holding the one worker, and with it every other request.

    A "text_stream" request is an utterance with a TextFeed (eng.push_text, eng.text_state); with text_hold the engine was
    told eng.hold_text(), with prefix_cache eng.prefix_cache(n, rows), before this scheduler opens the batch.  eng.admit is
    called positionally as it always was; keys=[each utterance's prefix_key; None: admitted uncached] is added only with
    prefix_cache (prefix_hits / prefix_misses count the flags it returns), prompts=[each utterance's prompt or None] only when
    an utterance of the admission has one, so an engine without either argument serves everything else.  A streamed request's
    push worker finds the prompt of a slot it resets in state.prompts[slot], an unstreamed reply in state.utt_prompts.

    logprobs: the engine was told eng.scores_reserve() before this scheduler opens the batch, and a request may carry
    "logprobs": true (without it the key is refused).  eng.scores() is then read, beside eng.codes(), at the checks where an
    utterance of such a request ends: its log-probabilities go into state.utt_scores[utt], where the unstreamed reply, the
    push that ends a streamed utterance and the per-request line find them."""

    def __init__(self, eng, max_batch, max_queue, prepare, reply, push, close_stream, send_error, check_every=8,
                 send_timeout=30.0, text_wait_ms=200.0, text_hold=False, prefix_cache=False, logprobs=False):
        from concurrent.futures import ThreadPoolExecutor
        self.eng, self.B, self.max_queue, self.check_every = eng, int(max_batch), int(max_queue), int(check_every)
        self._prepare, self._reply, self._push, self._close_stream, self._send_error = prepare, reply, push, close_stream, send_error
        self._cv = threading.Condition()
        self._queue = collections.deque()       # (request, Utterance) in admission order
        self._running, self._thread = False, None
        self._pool = ThreadPoolExecutor(max_workers=1)
        self.alive = True                       # False once the engine thread has stopped on an error
        self.frame_steps = 0                    # frame steps the engine has run
        self.send_timeout, self.text_wait_ms = float(send_timeout), float(text_wait_ms)
        self.text_hold, self.prefix_cache = bool(text_hold), bool(prefix_cache)
        self.logprobs = bool(logprobs)
        self.starved_checks = 0                 # checks that ran no frame because a text slot waited for its text
        self.held_steps = 0                     # text_hold: frame steps text slots were held for, summed over requests
        self.prefix_hits = self.prefix_misses = 0   # prefix_cache: admitted utterances that came from the cache / were prefilled
        self._owner = [None] * self.B           # (request, utt) of each slot; this and the next three are the engine thread's
        self._pushed = [0] * self.B             # frames of each slot that have gone to a push
        self._last_held = [0] * self.B          # text_hold: eng.held_steps() of each slot at the last check
        self._pending_pushes = []

    # ---- accept side ----
    def submit(self, conn, msg, t0=None):
        """Check a request and queue its utterances, or answer -2 on its own connection and close it.  -> True if queued."""
        sec = int(self.send_timeout)
        conn.setsockopt(socket.SOL_SOCKET, socket.SO_SNDTIMEO,
                        struct.pack("ll", sec, int(round((self.send_timeout - sec) * 1e6))))
        try:
            items = self._prepare(msg)
            vocoder, arithmetic = request_vocoder(msg), request_vocoder_arithmetic(msg)
            logprobs = request_logprobs(msg, self.logprobs)
        except Exception as e:
            print(f"Error: {e}")
            return self._refuse(conn)
        with self._cv:
            if not self.alive or len(self._queue) + len(items) > self.max_queue:
                print(f"Error: queue full ({len(self._queue)} of {self.max_queue} utterances queued)" if self.alive else
                      "Error: the engine has stopped")
                return self._refuse(conn)
            req = _Request(conn, items, msg.get("stream"), time.time() if t0 is None else t0, vocoder, arithmetic, logprobs)
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
        if req.state.failed:
            return True
        try:
            ev = ConcurrentScheduler._poll([req], 0)
        except (OSError, ValueError):
            return True
        return bool(ev and ev[0][1] & (select.POLLHUP | select.POLLERR | select.POLLNVAL))

    @staticmethod
    def _poll(reqs, ms):
        """Wait until a client of `reqs` has sent something (or left), for at most ms milliseconds."""
        p = select.poll()
        for req in reqs:
            p.register(req.conn.fileno(), select.POLLIN)
        return p.poll(ms)

    def _drop(self, req):
        """Engine side: a request that is gone or failed; its connection closes after whatever the worker still has for it."""
        if not req.gone:
            req.gone = True
            self._pool.submit(req.conn.close)

    def _fail(self, req, why):
        """Engine side: a request that cannot go on gets -2 now; its slots are released at this check."""
        if not req.gone:
            print(f"Error: {why}")
            req.state.failed = True
            self._pool.submit(self._send_error, req.conn)
            self._drop(req)

    def _refuse_all(self):
        """The engine thread ends (shutting down, or on an error): whatever is still in flight or queued gets -2."""
        with self._cv:
            rest = {id(r): r for r, _ in self._queue}
            self._queue.clear()
        rest.update({id(o[0]): o[0] for o in self._owner if o is not None})
        for req in rest.values():
            if not req.gone:
                req.gone = True
                self._pool.submit(self._refuse, req.conn)

    def _feed_text(self):
        """Engine side, before a check: read what the text-stream clients have sent and push the rows that are ready."""
        for b, o in enumerate(self._owner):
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

    def _wait_for_text(self):
        """Engine side, after a check that ran no frame: the starved-batch rule.  -> True if the check was a starved one."""
        _, starved = self.eng.text_state()
        waiting = {id(o[0]): o[0] for b, o in enumerate(self._owner) if starved[b] and o is not None and not o[0].gone}
        if not waiting:
            return False
        self.starved_checks += 1
        if not self._poll(waiting.values(), self.text_wait_ms):
            for req in waiting.values():
                self._fail(req, f"text stream: no text for {self.text_wait_ms:.0f} ms while the frame loop waited for it")
        return True

    def _text_ready(self, req):
        """Engine side, text_hold: whether a queued text-stream request has its first row; a client that half-closed fails."""
        try:
            if not req.feed.poll(req.conn):
                raise ValueError("the client closed its sending side before the end of its text")
        except Exception as e:
            self._fail(req, f"text stream: {e}")
            return False
        return req.feed.ready()

    def _check_held(self, ran):
        """Engine side, text_hold, after every check: count the held steps, apply the held-slot rule, and -- after a check that
        ran no frame because every live slot is held -- wait a moment for a client to send.  -> True if it was such a check."""
        owner, last_held = self._owner, self._last_held
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
        # short: a new request must not wait for it
        self._poll([req for req, _ in waiting.values()], max(1.0, min([20.0] + [left for _, left in waiting.values()])))
        return True

    def _engine_main(self):
        try:
            self._engine_loop()
        except Exception as e:
            print(f"Error: the engine thread stopped: {e}")
            with self._cv:
                self.alive = False
        self._refuse_all()

    def _engine_loop(self):
        """One check per turn: take, admit, feed text, run, release, dispatch -- until the scheduler stops."""
        self.eng.open(self.B)
        while True:
            taken = self._take()
            if taken is None:
                return
            free, take, later = taken
            if not take and all(o is None for o in self._owner):
                waiting = [r for r, _ in later if not r.gone]
                if waiting:                    # only text requests without a row are queued: until one of them sends (or leaves)
                    self._poll(waiting, 20.0)  # (short: a request submitted meanwhile is looked at soon)
                continue                       # what was queued has left and nothing is live: back to waiting
            resets = self._admit(free, take)
            text_live = any(o is not None and o[0].feed is not None for o in self._owner)
            if text_live:
                self._feed_text()
            ran, waited = self._run(text_live)
            done, per = self.eng.done()
            gone = self._release_gone()
            self._dispatch(done, per, resets, stalled=ran == 0 and not gone and not take and not waited)

    def _take(self):
        """Step 1: block while nothing is live or queued, then take queued utterances for the free slots.  -> (free slots,
        the (request, utterance) pairs to admit, those left waiting for a first row), or None once the scheduler stops."""
        owner = self._owner
        with self._cv:
            while self._running and not self._queue and all(o is None for o in owner):
                self._cv.wait()            # nothing live, nothing queued: block (no spinning)
            if not self._running:
                return None
            free = [b for b in range(self.B) if owner[b] is None]
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
        return free, [(r, it) for r, it in take if not r.gone], later

    def _admit(self, free, take):
        """Step 2: admit the taken utterances.  -> the slots a streamed request's next push resets, by id(request)."""
        resets = collections.defaultdict(list)
        if not take:
            return resets
        slots = free[:len(take)]
        args = (slots, [it.prefix for _, it in take], [it.n_text for _, it in take], [it.params for _, it in take])
        kw = {"prompts": [it.prompt for _, it in take]} if any(it.prompt is not None for _, it in take) else {}
        if any(it.rules is not None for _, it in take):     # (a server with --sampler_rules: eng.rules() was called)
            kw["rules"] = [it.rules for _, it in take]
        if self.prefix_cache:
            hit = self.eng.admit(*args, keys=[it.prefix_key for _, it in take], **kw)
            self.prefix_hits += int(np.count_nonzero(hit))
            self.prefix_misses += len(take) - int(np.count_nonzero(hit))
        else:
            self.eng.admit(*args, **kw)
        for b, (req, it) in zip(slots, take):
            self._owner[b] = (req, it.utt)
            self._pushed[b] = 0
            self._last_held[b] = 0
            if req.stream:
                resets[id(req)].append(b)
                if it.prompt is not None and req.state.vocoder == "incremental":
                    req.state.prompts[b] = it.prompt   # (taken by the push that resets slot b)
        return resets

    def _run(self, text_live):
        """Step 4: run check_every frames, then see to starved or held text slots.  -> (frames run, whether it waited)."""
        ran = self.eng.run(self.check_every)
        self.frame_steps += ran
        if self.text_hold:
            return ran, text_live and self._check_held(ran)
        return ran, ran == 0 and text_live and self._wait_for_text()

    def _release_gone(self):
        """Step 5: clients that went away: their slots go idle now.  -> the released slots."""
        owner = self._owner
        for req in {id(o[0]): o[0] for o in owner if o is not None}.values():
            if self._client_gone(req):
                self._drop(req)
        gone = [b for b in range(self.B) if owner[b] is not None and owner[b][0].gone]
        if gone:
            self.eng.release(gone)
            for b in gone:
                owner[b] = None
        return gone

    def _dispatch(self, done, per, resets, stalled):
        """Step 6: the streamed requests' new frames go to the worker; a request whose last utterance ended gets its reply."""
        owner = self._owner
        fin = [b for b in range(self.B) if owner[b] is not None and done[b]]
        streamed = {}                                # id(request) -> (request, its (slot, utt) pairs)
        for b in range(self.B):
            if owner[b] is not None and owner[b][0].stream:
                streamed.setdefault(id(owner[b][0]), (owner[b][0], []))[1].append((b, owner[b][1]))
        if not fin and not streamed:
            if stalled:
                raise RuntimeError("the engine ran no frame and no utterance ended")
            return
        codes, _ = self.eng.codes()
        # the log-probabilities, when an utterance that asked for them ends at this check
        scores = self.eng.scores()[0] if any(owner[b][0].state.logprobs for b in fin) else None
        for b in fin:
            req, utt = owner[b]
            if req.state.logprobs:
                req.state.utt_scores[utt] = np.ascontiguousarray(scores[:int(per[b]), b, :], dtype=np.float32)
        pushes = []
        for key, (req, slots) in streamed.items():
            entries = new_entries(codes, per, slots, self._pushed, fin)
            req.state.frames += sum(len(e.codes) for e in entries if e.finished)
            if entries or resets[key]:
                pushes.append((req, resets[key], entries))
        for f in self._pending_pushes:               # at most one check's pushes in flight
            f.result()
        self._pending_pushes = [self._pool.submit(self._push, req.conn, req.state, r, e) for req, r, e in pushes]
        for b in fin:
            req, utt = owner[b]
            owner[b] = None
            req.codes[utt] = np.ascontiguousarray(codes[:int(per[b]), b, :], dtype=np.int32)
            req.left -= 1
            if req.left == 0 and req.stream:
                self._pool.submit(self._close_stream, req.conn, req.state, req.t0)
            elif req.left == 0:
                self._pool.submit(self._reply, req.conn, req.codes, req.t0, req.state)
