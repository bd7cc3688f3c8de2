"""batch_server --concurrent --logprobs without a GPU: the "logprobs" key and what refuses it, both reply shapes packed and
read back, the scheduler handing eng.scores() to the replies -- against a stand-in engine in the style of
tests/test_concurrent_scheduler.py -- and the bytes of a reply to a request without the key, which are what they always were.
CPU only."""
import io
import json
import socket
import struct

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from tests.test_concurrent_scheduler import (CAP, FakeEngine, fake_close_stream, fake_prepare, fake_push, fake_reply, read_stream,
                                             send_error)
from tests.test_text_stream_scheduler import _bare_server


def _msg(**req):
    return json.loads(bs.pack_batch_request(**req)[4:].decode())


class Pipe:
    """bytes as a connection that recv()s them"""

    def __init__(self, raw):
        self._b = io.BytesIO(raw)

    def recv(self, n, *flags):
        return self._b.read(n)

    def left(self):
        return len(self._b.read())


# ---- the key ----------------------------------------------------------------------------------------------------------------
def test_the_request_carries_the_key_only_when_asked():
    assert "logprobs" not in _msg(token_ids=[[1, 2]])
    assert _msg(token_ids=[[1, 2]], logprobs=True)["logprobs"] is True
    # a request without the key is the bytes it always was
    assert bs.pack_batch_request(token_ids=[[1, 2]], max_tokens=7, seed=3) == bs.pack_batch_request(token_ids=[[1, 2]], max_tokens=7, seed=3,
                                                                                                  logprobs=None)


def test_request_logprobs():
    assert bs.request_logprobs({}, False) is False and bs.request_logprobs({}, True) is False
    assert bs.request_logprobs({"logprobs": None}, False) is False
    assert bs.request_logprobs({"logprobs": True}, True) is True
    assert bs.request_logprobs({"logprobs": False}, True) is False
    for v in (True, False):
        with pytest.raises(ValueError, match="--logprobs"):
            bs.request_logprobs({"logprobs": v}, False)
    for v in (1, 0, "true", "yes", 1.0, [True], {"on": True}):
        for enabled in (False, True):
            with pytest.raises(ValueError, match="true or false"):
                bs.request_logprobs({"logprobs": v}, enabled)


def test_prepare_refuses_the_key_without_the_flag_and_a_wrong_type():
    srv = _bare_server()
    ids = [[5, 6, 7], [9]]
    plain = srv._prepare(_msg(token_ids=ids, seed=3))
    with pytest.raises(ValueError, match="--logprobs"):
        srv._prepare(_msg(token_ids=ids, seed=3, logprobs=True))
    srv.logprobs = True
    for v in (1, "true", 0.5, [True]):
        with pytest.raises(ValueError, match="true or false"):
            srv._prepare(dict(_msg(token_ids=ids, seed=3), logprobs=v))
    # with the flag the key changes nothing of what is queued
    for v in (True, False):
        for a, b in zip(srv._prepare(_msg(token_ids=ids, seed=3, logprobs=v)), plain):
            np.testing.assert_array_equal(a.prefix, b.prefix)
            assert (a.utt, a.n_text, a.params, a.prefix_key) == (b.utt, b.n_text, b.params, b.prefix_key)


def test_the_flag_needs_concurrent():
    with pytest.raises(ValueError, match="--concurrent"):
        bs.BatchSynthesisServer("none.q3w", "none.q3w", logprobs=True, install_signal_handlers=False)


def test_the_per_request_line_names_the_mean_of_column_0():
    note = bs.BatchSynthesisServer._logprob_note
    assert note(bs.ReplyState(2)) == ""
    st = bs.ReplyState(2, logprobs=True, utt_scores=[np.full((4, 16), -2.0, np.float32) * np.arange(1, 17, dtype=np.float32),
                                                      np.array([[-1.0] * 16, [-4.0] * 16], np.float32)])
    assert note(st) == ", mean logprob -2.000 -2.500"
    st.utt_scores[1] = None                              # an utterance that never ended (the request failed on the way)
    assert note(st) == ", mean logprob -2.000 nan"


# ---- the wire ---------------------------------------------------------------------------------------------------------------
RNG = np.random.default_rng(51)
RESULTS = [(RNG.integers(0, 2048, (n, 16)).astype(np.int32), RNG.integers(-3000, 3000, 37 * n).astype(np.int16)) for n in (5, 0, 12)]
SCORES = [(-8.0 * RNG.random((n, 16))).astype(np.float32) for n in (5, 0, 12)]
SCORES[0][1, 3], SCORES[0][2, 0], SCORES[2][0, 15] = -np.inf, np.nan, 0.0


def parent_pack_batch_reply(results):
    """The reply as every server before --logprobs packed it, spelled out: i32 n, then per utterance i32 n_frames,
    i32[n_frames * 16], i32 n_samples, i16[n_samples], little-endian."""
    raw = struct.pack("<i", len(results))
    for codes, pcm in results:
        c = np.asarray(codes).astype("<i4").reshape(-1, 16)
        a = np.asarray(pcm).astype("<i2").reshape(-1)
        raw += struct.pack("<i", c.shape[0]) + c.tobytes() + struct.pack("<i", a.shape[0]) + a.tobytes()
    return raw


def test_unstreamed_reply_round_trip():
    raw = bs.pack_batch_reply(RESULTS, SCORES)
    pipe = Pipe(raw)
    got = bs.read_batch_reply(pipe, logprobs=True)
    assert pipe.left() == 0 and len(got) == 3
    for (c, a, s), (rc, ra), rs in zip(got, RESULTS, SCORES):
        np.testing.assert_array_equal(c, rc)
        np.testing.assert_array_equal(a, ra)
        assert s.dtype == np.float32 and s.shape == rs.shape and s.tobytes() == rs.tobytes()     # NaN and -inf as they were
    # each utterance's block, then i32 n_frames and f32[n_frames * 16]
    want = struct.pack("<i", 3)
    for (c, a), s in zip(RESULTS, SCORES):
        want += parent_pack_batch_reply([(c, a)])[4:] + struct.pack("<i", len(s)) + s.astype("<f4").tobytes()
    assert raw == want
    with pytest.raises(ValueError, match="frames"):
        bs.pack_batch_reply(RESULTS, [SCORES[0], SCORES[1], SCORES[2][:-1]])


def test_streamed_record_round_trip():
    assert bs.REC_SCORES == 3
    raw = bs.pack_stream_scores(2, SCORES[2]) + bs.pack_stream_end(2, RESULTS[2][0]) + bs.pack_stream_scores(1, SCORES[1]) + \
        P.pack_sentinel(P.SENTINEL_DONE)
    assert raw[:12] == struct.pack("<iii", 3, 2, 12) and raw[12:12 + 12 * 16 * 4] == SCORES[2].astype("<f4").tobytes()
    pipe = Pipe(raw)
    kind, utt, s = bs.read_stream_record(pipe)
    assert (kind, utt) == ("scores", 2) and s.dtype == np.float32 and s.tobytes() == SCORES[2].tobytes()
    kind, utt, c = bs.read_stream_record(pipe)
    assert (kind, utt) == ("end", 2)
    np.testing.assert_array_equal(c, RESULTS[2][0])
    kind, utt, s = bs.read_stream_record(pipe)
    assert (kind, utt, s.shape) == ("scores", 1, (0, 16))
    assert bs.read_stream_record(pipe) == ("done",) and pipe.left() == 0
    with pytest.raises(RuntimeError, match="unknown record"):
        bs.read_stream_record(Pipe(struct.pack("<iii", 4, 0, 0)))


def test_replies_without_the_key_are_the_parents_bytes():
    assert bs.pack_batch_reply(RESULTS) == parent_pack_batch_reply(RESULTS)
    assert bs.pack_batch_reply(RESULTS, None) == parent_pack_batch_reply(RESULTS)
    assert bs.pack_batch_reply([]) == struct.pack("<i", 0)
    for got, (c, a) in zip(bs.read_batch_reply(Pipe(parent_pack_batch_reply(RESULTS))), RESULTS):
        assert len(got) == 2
        np.testing.assert_array_equal(got[0], c)
        np.testing.assert_array_equal(got[1], a)
    assert bs.pack_stream_end(1, RESULTS[0][0]) == struct.pack("<iii", 2, 1, 5) + RESULTS[0][0].astype("<i4").tobytes()
    assert bs.pack_stream_audio(0, RESULTS[0][1]) == struct.pack("<iii", 1, 0, 185) + RESULTS[0][1].astype("<i2").tobytes()


# ---- the scheduler ------------------------------------------------------------------------------------------------------------
class ScoreFakeEngine(FakeEngine):
    """FakeEngine with scores(): the score of codes[f][b][g] is -(tag + f / 100 + g / 10000)."""

    def __init__(self):
        super().__init__()
        self.score_reads = 0

    def scores(self):
        self.score_reads += 1
        codes, per = self.codes()
        out = np.zeros(codes.shape, np.float32)
        for b in range(self.B):
            if self.tag[b] is not None:
                for f in range(self.frames[b]):
                    out[f, b, :] = -(self.tag[b] + f / 100.0 + np.arange(16) / 10000.0)
        return out, per


def want_scores(tag, n):
    return np.array([[-(tag + f / 100.0 + g / 10000.0) for g in range(16)] for f in range(n)], np.float32).reshape(n, 16)


def score_reply(conn, cs, t0, state):
    """fake_reply with the server's rule: the scores of a "logprobs" request behind every utterance's block."""
    try:
        conn.sendall(bs.pack_batch_reply([(c, c[:, 0].astype(np.int16)) for c in cs], state.utt_scores if state.logprobs else None))
    finally:
        conn.close()


def score_push(conn, state, resets, entries):
    """fake_push with the server's rule: record 3 right before the end record of a "logprobs" request's utterance."""
    out = []
    for e in entries:
        if e.frames.shape[0]:
            out.append(bs.pack_stream_audio(e.utt, e.frames[:, 0].astype(np.int16)))
        if e.finished:
            if state.logprobs:
                out.append(bs.pack_stream_scores(e.utt, state.utt_scores[e.utt]))
            out.append(bs.pack_stream_end(e.utt, e.codes))
    if out:
        conn.sendall(b"".join(out))


def make(eng, logprobs, reply=score_reply, push=score_push):
    return bs.ConcurrentScheduler(eng, 2, 64, fake_prepare, reply, push, fake_close_stream, send_error, check_every=2,
                                  logprobs=logprobs)


def _submit(sched, **req):
    s, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    cli.settimeout(20)
    return sched.submit(s, _msg(**req)), cli


def _raw(cli):
    out = b""
    while True:
        b = cli.recv(65536)
        if not b:
            return out
        out += b


def test_the_scheduler_refuses_the_key_without_the_flag_for_that_request_alone():
    eng = ScoreFakeEngine()
    sched = make(eng, logprobs=False)
    ok, good = _submit(sched, token_ids=[[1] * 3])
    assert ok is True
    for bad in (dict(logprobs=True), dict(logprobs=True, stream=True)):
        ok, cli = _submit(sched, token_ids=[[2] * 3], **bad)
        assert ok is False and struct.unpack("<i", cli.recv(4))[0] == P.SENTINEL_ERROR
    assert len(sched._queue) == 1
    sched.start()
    try:
        (c, a), = bs.read_batch_reply(good)
    finally:
        sched.stop()
    assert c.shape == (3, 16) and eng.score_reads == 0
    # with the flag, a value that is not a boolean
    sched = make(ScoreFakeEngine(), logprobs=True)
    s, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    cli.settimeout(5)
    assert sched.submit(s, dict(_msg(token_ids=[[2] * 3]), logprobs="true")) is False
    assert struct.unpack("<i", cli.recv(4))[0] == P.SENTINEL_ERROR and len(sched._queue) == 0
    sched.stop()


def test_scores_reach_both_reply_shapes_and_nobody_else():
    eng = ScoreFakeEngine()
    sched = make(eng, logprobs=True)
    _, plain = _submit(sched, token_ids=[[1] * 3, [2] * 5])
    _, scored = _submit(sched, token_ids=[[3] * 4, [4] * 2], logprobs=True)
    _, streamed = _submit(sched, token_ids=[[5] * 5, [6] * 3], logprobs=True, stream=True)
    _, plain_stream = _submit(sched, token_ids=[[7] * 3], stream=True)
    _, off = _submit(sched, token_ids=[[8] * 2], logprobs=False)
    sched.start()
    try:
        raw_plain = _raw(plain)
        got = bs.read_batch_reply(scored, logprobs=True)
        recs = read_stream(streamed)
        raw_stream = _raw(plain_stream)
        raw_off = _raw(off)
    finally:
        sched.stop()
    # the requests without the key (or with false): the parent's bytes
    cs = [np.array([[1000 * t + f] * 16 for f in range(n)], np.int32) for t, n in ((1, 3), (2, 5))]
    assert raw_plain == parent_pack_batch_reply([(c, c[:, 0].astype(np.int16)) for c in cs])
    c8 = np.array([[8000 + f] * 16 for f in range(2)], np.int32)
    assert raw_off == parent_pack_batch_reply([(c8, c8[:, 0].astype(np.int16))])
    c7 = np.array([[7000 + f] * 16 for f in range(3)], np.int32)
    kinds, pcm = [], []
    pipe = Pipe(raw_stream)
    while True:
        rec = bs.read_stream_record(pipe)
        kinds.append(rec[0])
        if rec[0] == "done":
            break
        if rec[0] == "audio":
            pcm.append(rec[2])
        else:
            np.testing.assert_array_equal(rec[2], c7)
    assert "scores" not in kinds and kinds[-2:] == ["end", "done"] and pipe.left() == 0
    np.testing.assert_array_equal(np.concatenate(pcm), c7[:, 0].astype(np.int16))
    # unstreamed with the key
    assert [len(r) for r in got] == [3, 3]
    for (c, a, s), (tag, n) in zip(got, ((3, 4), (4, 2))):
        assert c.shape == (n, 16) and int(c[0, 0]) == tag * 1000
        assert s.tobytes() == want_scores(tag, n).tobytes()
    # streamed with the key: record 3 once per utterance, directly before its end record
    order = [(r[0], r[1]) for r in recs if r[0] != "audio"]
    assert sorted(order) == [("end", 0), ("end", 1), ("scores", 0), ("scores", 1)]
    for i, (kind, utt) in enumerate(r[:2] for r in recs):
        if kind == "scores":
            assert recs[i + 1][:2] == ("end", utt)
    by = {(r[0], r[1]): r[2] for r in recs if r[0] != "audio"}
    for utt, (tag, n) in enumerate(((5, 5), (6, 3))):
        assert by[("end", utt)].shape == (n, 16)
        assert by[("scores", utt)].tobytes() == want_scores(tag, n).tobytes()
    assert eng.score_reads >= 1


def test_an_engine_without_scores_serves_requests_without_the_key():
    """eng.scores() is read only at a check where an utterance that asked for it ends."""
    eng = FakeEngine()                       # no scores() at all
    sched = make(eng, logprobs=True, reply=fake_reply, push=fake_push)
    _, a = _submit(sched, token_ids=[[1] * 3])
    _, b = _submit(sched, token_ids=[[2] * 4], stream=True)
    sched.start()
    try:
        (c, _), = bs.read_batch_reply(a)
        recs = read_stream(b)
    finally:
        sched.stop()
    assert c.shape == (3, 16) and [r[0] for r in recs if r[0] != "audio"] == ["end"] and CAP >= 4
