"""batch_server --concurrent without a GPU: the scheduler (ConcurrentScheduler) against a fake engine with the FrameEngine
surface open / admit / release / run / done / codes, and the request's sampling keys.  CPU only."""
import json
import socket
import struct
import threading
import time

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from qwen3_tts_axera_russian_amd.engine import SlotParams

CAP = 50   # the server's --max_tokens
DEFAULTS = SlotParams(max_frames=CAP, temperature=0.0, top_k=50, top_p=0.95, cp_temperature=0.0, cp_top_k=50, seed=0)


class FakeEngine:
    """Slot b's utterance emits one frame per step, codes[f][b] = tag * 1000 + f (tag = the utterance's first token id), and
    ends after min(budget, natural length = its number of text tokens) frames."""

    def __init__(self, step_s=0.0):
        self.step_s = step_s
        self.admitted = []       # (tag, slot, SlotParams) in admission order
        self.released = []       # (slot, frames it had emitted)
        self.opened = []

    def open(self, B):
        self.opened.append(B)
        self.B = B
        self.tag = [None] * B
        self.lim = [0] * B
        self.frames = [0] * B
        self.ended = [True] * B

    def admit(self, slots, prefixes, n_text, params):
        assert len(slots) == len(prefixes) == len(n_text) == len(params) > 0
        for b, p, nt, sp in zip(slots, prefixes, n_text, params):
            assert self.ended[b], "admitted into a live slot"
            self.tag[b] = int(p[0, 0])
            self.lim[b] = min(sp.max_frames, nt)
            self.frames[b] = 0
            self.ended[b] = False
            self.admitted.append((self.tag[b], b, sp))

    def release(self, slots):
        for b in slots:
            self.released.append((b, self.frames[b]))
            self.ended[b] = True

    def run(self, n):
        steps = 0
        while steps < n and not all(self.ended):
            for b in range(self.B):
                if not self.ended[b]:
                    self.frames[b] += 1
                    self.ended[b] = self.frames[b] >= self.lim[b]
            steps += 1
            if self.step_s:
                time.sleep(self.step_s)
        return steps

    def done(self):
        return np.array(self.ended), np.array(self.frames, np.int32)

    def codes(self):
        nf = max(self.frames)
        out = np.full((nf, self.B, 16), -1, np.int32)
        for b in range(self.B):
            if self.tag[b] is not None:
                for f in range(self.frames[b]):
                    out[f, b, :] = self.tag[b] * 1000 + f
        return out, np.array(self.frames, np.int32)


def fake_prepare(msg):
    """The server's _prepare without a front end: the prefix carries the utterance's tag (its first token id)."""
    ids = msg["token_ids"]
    if not ids:
        raise ValueError("a request needs at least one utterance")
    base = bs.request_slot_params(msg, DEFAULTS, CAP)
    import dataclasses
    return [bs.Utterance(i, np.full((2, 4), t[0], np.float32), len(t), dataclasses.replace(base, utt=i)) for i, t in enumerate(ids)]


def fake_reply(conn, cs, t0, state):
    try:
        conn.sendall(bs.pack_batch_reply([(c, c[:, 0].astype(np.int16)) for c in cs]))
    finally:
        conn.close()


def fake_push(conn, state, resets, entries):
    out = []
    for _, utt, new, fin, whole in entries:
        if new.shape[0]:
            out.append(bs.pack_stream_audio(utt, new[:, 0].astype(np.int16)))
        if fin:
            out.append(bs.pack_stream_end(utt, whole))
    try:
        if out:
            conn.sendall(b"".join(out))
    except OSError:
        state.failed = True


def fake_close_stream(conn, state, t0):
    try:
        if not state.failed:
            conn.sendall(P.pack_sentinel(P.SENTINEL_DONE))
    except OSError:
        pass
    finally:
        conn.close()


def send_error(conn):
    try:
        conn.sendall(P.pack_sentinel(P.SENTINEL_ERROR))
    except OSError:
        pass


def make(eng, max_batch=2, max_queue=64, check_every=2):
    return bs.ConcurrentScheduler(eng, max_batch, max_queue, fake_prepare, fake_reply, fake_push, fake_close_stream,
                                  send_error, check_every=check_every)


def submit(sched, **req):
    """-> the client's end of a socket pair whose server end carries the request."""
    srv, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    cli.settimeout(20)
    raw = bs.pack_batch_request(**req)
    msg = json.loads(raw[4:].decode())
    sched.submit(srv, msg)
    return cli


def read_stream(cli):
    recs = []
    while True:
        rec = bs.read_stream_record(cli)
        if rec[0] == "done":
            return recs
        recs.append(rec)


def test_fifo_admission_routing_and_budgets():
    """Utterances of interleaved requests are admitted FIFO (request by request, each in its own order); every reply reaches its
    own connection with its utterances in request order; a request's max_tokens is each of its slots' budget."""
    eng = FakeEngine()
    sched = make(eng, max_batch=2)
    a = submit(sched, token_ids=[[11, 0, 0, 0, 0, 0], [12, 0, 0], [13] + [0] * 9], max_tokens=4)
    b = submit(sched, token_ids=[[21] * 7, [22] * 2], max_tokens=30)
    c = submit(sched, token_ids=[[31] * 5], stream=True)
    d = submit(sched, token_ids=[[41] * 3, [42] * 8])
    sched.start()
    try:
        ra, rb, rd = bs.read_batch_reply(a), bs.read_batch_reply(b), bs.read_batch_reply(d)
        rc = read_stream(c)
    finally:
        sched.stop()
    assert eng.opened == [2]
    assert [t for t, _, _ in eng.admitted] == [11, 12, 13, 21, 22, 31, 41, 42]
    budgets = {t: sp.max_frames for t, _, sp in eng.admitted}
    assert [budgets[t] for t in (11, 12, 13)] == [4, 4, 4]
    assert [budgets[t] for t in (21, 22)] == [30, 30]
    assert budgets[31] == budgets[41] == CAP
    utts = {t: sp.utt for t, _, sp in eng.admitted}
    assert [utts[t] for t in (11, 12, 13, 21, 22, 41, 42)] == [0, 1, 2, 0, 1, 0, 1]
    for res, tags, lens in ((ra, (11, 12, 13), (4, 3, 4)), (rb, (21, 22), (7, 2)), (rd, (41, 42), (3, 8))):
        assert len(res) == len(tags)
        for (codes, pcm), t, n in zip(res, tags, lens):
            np.testing.assert_array_equal(codes[:, 0], t * 1000 + np.arange(n))
            np.testing.assert_array_equal(pcm, (t * 1000 + np.arange(n)).astype(np.int16))
    # the streamed request: audio records joined + the end record carry its utterance, nothing of another request
    audio = np.concatenate([r[2] for r in rc if r[0] == "audio"])
    ends = [r for r in rc if r[0] == "end"]
    assert len(ends) == 1 and ends[0][1] == 0
    np.testing.assert_array_equal(ends[0][2][:, 0], 31000 + np.arange(5))
    np.testing.assert_array_equal(audio, (31000 + np.arange(5)).astype(np.int16))
    assert sched.frame_steps < sum((4, 3, 4, 7, 2, 5, 3, 8))     # slots were shared


def test_closed_connection_releases_its_slots_and_others_go_on():
    eng = FakeEngine(step_s=0.002)
    sched = make(eng, max_batch=2, check_every=1)
    long_ = submit(sched, token_ids=[[71] * 60])                      # 50 frames (the cap) at 2 ms each
    other = submit(sched, token_ids=[[81] * 6, [82] * 6, [83] * 6])
    sched.start()
    try:
        t = time.time()
        while not any(tag == 71 for tag, _, _ in eng.admitted):
            assert time.time() - t < 10
            time.sleep(0.001)
        long_.close()
        res = bs.read_batch_reply(other)
        t = time.time()
        while not eng.released:
            assert time.time() - t < 10
            time.sleep(0.005)
    finally:
        sched.stop()
    slot71 = [b for tag, b, _ in eng.admitted if tag == 71][0]
    assert eng.released[0][0] == slot71 and eng.released[0][1] < CAP    # released before its budget ran out
    assert [int(c[0, 0]) for c, _ in res] == [81000, 82000, 83000]


def test_full_queue_answers_minus_two_and_the_server_keeps_serving():
    eng = FakeEngine()
    sched = make(eng, max_batch=2, max_queue=4)
    first = submit(sched, token_ids=[[51] * 3, [52] * 3, [53] * 3])
    over = submit(sched, token_ids=[[61] * 3, [62] * 3])              # 3 + 2 > 4
    assert struct.unpack("<i", over.recv(4))[0] == P.SENTINEL_ERROR
    assert over.recv(1) == b""                                       # and its connection is closed
    sched.start()
    try:
        assert len(bs.read_batch_reply(first)) == 3
        after = submit(sched, token_ids=[[91] * 2])
        res = bs.read_batch_reply(after)
    finally:
        sched.stop()
    assert int(res[0][0][0, 0]) == 91000
    assert 61 not in [t for t, _, _ in eng.admitted]


def test_engine_thread_blocks_when_idle():
    """Nothing live and nothing queued: the engine thread waits on the queue instead of stepping the loop."""
    eng = FakeEngine()
    calls = []
    run = eng.run
    eng.run = lambda n: calls.append(n) or run(n)
    sched = make(eng)
    sched.start()
    try:
        time.sleep(0.2)
        assert calls == []
        r = bs.read_batch_reply(submit(sched, token_ids=[[17] * 3]))
        assert int(r[0][0][0, 0]) == 17000
        n = len(calls)
        time.sleep(0.2)
        assert len(calls) == n
    finally:
        sched.stop()


def test_request_keys_round_trip():
    raw = bs.pack_batch_request(token_ids=[[1, 2]], max_tokens=20, temperature=0.7, top_k=5, top_p=0.9, cp_temperature=0.25,
                                cp_top_k=7, seed=2 ** 64 - 1)
    (n,) = struct.unpack("<I", raw[:4])
    msg = json.loads(raw[4:4 + n].decode())
    p = bs.request_slot_params(msg, DEFAULTS, CAP)
    assert p == SlotParams(max_frames=20, temperature=0.7, top_k=5, top_p=0.9, cp_temperature=0.25, cp_top_k=7,
                           seed=2 ** 64 - 1, utt=0)
    # a missing key takes the server's value; max_tokens beyond the server's cap is clamped to it, as before
    msg = json.loads(bs.pack_batch_request(token_ids=[[1]], max_tokens=500)[4:].decode())
    assert not {"temperature", "top_k", "top_p", "cp_temperature", "cp_top_k", "seed"} & set(msg)
    assert bs.request_slot_params(msg, DEFAULTS, CAP) == DEFAULTS


@pytest.mark.parametrize("bad", [{"temperature": -0.1}, {"temperature": float("nan")}, {"cp_temperature": float("inf")},
                                 {"top_p": 0.0}, {"top_p": 1.5}, {"seed": -1}, {"seed": 2 ** 64}, {"seed": 1.5},
                                 {"top_k": "many"}, {"temperature": True}, {"max_tokens": -3}, {"max_tokens": 2.5}])
def test_out_of_range_keys_are_refused_before_anything_is_queued(bad):
    with pytest.raises(ValueError):
        bs.request_slot_params(dict({"token_ids": [[1]]}, **bad), DEFAULTS, CAP)
    eng = FakeEngine()
    sched = make(eng)
    srv, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    cli.settimeout(5)
    assert sched.submit(srv, dict({"token_ids": [[1, 2], [3]]}, **bad)) is False
    assert len(sched._queue) == 0
    assert struct.unpack("<i", cli.recv(4))[0] == P.SENTINEL_ERROR
    sched.stop()


def test_slot_params_check():
    with pytest.raises(ValueError):
        SlotParams(max_frames=0).check(10)
    with pytest.raises(ValueError):
        SlotParams(max_frames=11).check(10)
    SlotParams(max_frames=10, temperature=0.5, top_p=1.0, seed=2 ** 64 - 1).check(10)


def _wait_until(cond, what, limit=10.0):
    t = time.time()
    while not cond():
        assert time.time() - t < limit, what
        time.sleep(0.002)


def test_a_queued_client_that_leaves_while_nothing_is_live_does_not_stop_the_server():
    eng = FakeEngine()
    sched = make(eng)
    quitter = submit(sched, token_ids=[[14] * 5])
    quitter.close()                                              # gone before the engine thread looks at the queue
    sched.start()
    try:
        time.sleep(0.1)
        assert sched.alive
        res = bs.read_batch_reply(submit(sched, token_ids=[[15] * 4]))
        assert sched.alive
    finally:
        sched.stop()
    assert int(res[0][0][0, 0]) == 15000
    assert [t for t, _, _ in eng.admitted] == [15]


def test_a_client_that_gives_up_in_the_queue_behind_a_live_request():
    eng = FakeEngine(step_s=0.002)
    sched = make(eng, max_batch=1, check_every=2)
    a = submit(sched, token_ids=[[24] * 40])                     # 40 frames in the only slot
    sched.start()
    try:
        _wait_until(lambda: eng.admitted, "request A was not admitted")
        waiting = submit(sched, token_ids=[[25] * 5])             # queued behind A ...
        waiting.close()                                          # ... and gives up
        assert int(bs.read_batch_reply(a)[0][0][0, 0]) == 24000
        time.sleep(0.1)
        assert sched.alive
        res = bs.read_batch_reply(submit(sched, token_ids=[[26] * 3]))
    finally:
        sched.stop()
    assert int(res[0][0][0, 0]) == 26000
    assert [t for t, _, _ in eng.admitted] == [24, 26]


def test_a_half_closed_client_still_gets_its_reply():
    eng = FakeEngine(step_s=0.001)
    sched = make(eng, check_every=1)
    cli = submit(sched, token_ids=[[33] * 20])
    cli.shutdown(socket.SHUT_WR)                                 # done sending; still reading
    sched.start()
    try:
        res = bs.read_batch_reply(cli)
    finally:
        sched.stop()
    np.testing.assert_array_equal(res[0][0][:, 0], 33000 + np.arange(20))
    assert eng.released == []


def test_a_client_that_stops_reading_fails_alone():
    """A streamed client that stays connected but never reads: the write to it times out, its request fails and its slot is
    released; the other request is answered meanwhile."""
    def big_push(conn, state, resets, entries):
        if state.failed:
            return
        try:
            conn.sendall(b"\0" * (8 << 20))                     # far more than the socket buffer
        except OSError:
            state.failed = True

    eng = FakeEngine(step_s=0.002)
    sched = bs.ConcurrentScheduler(eng, 2, 64, fake_prepare, fake_reply, big_push, fake_close_stream, send_error,
                                   check_every=2, send_timeout=0.2)
    stuck = submit(sched, token_ids=[[44] * 60], stream=True)     # never read
    other = submit(sched, token_ids=[[45] * 30])
    sched.start()
    try:
        res = bs.read_batch_reply(other)
        _wait_until(lambda: eng.released, "the stuck request's slot was not released")
    finally:
        sched.stop()
        stuck.close()
    assert int(res[0][0][0, 0]) == 45000
    slot44 = [b for t, b, _ in eng.admitted if t == 44][0]
    assert eng.released[0][0] == slot44 and eng.released[0][1] < CAP
