"""batch_server --concurrent with a "text_stream" request, without a GPU: the scheduler against a stand-in engine (the one of
tests/test_concurrent_scheduler.py plus text slots that never run ahead of their rows).  CPU only."""
import dataclasses
import json
import socket
import struct
import time

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import frontend as fe
from qwen3_tts_axera_russian_amd import protocol as P
from qwen3_tts_axera_russian_amd.weights import ModelConfig
from tests.test_concurrent_scheduler import (CAP, DEFAULTS, FakeEngine, fake_close_stream, fake_prepare, fake_push, fake_reply,
                                             read_stream, send_error)

EOS_ROW, PAD = -1, -5


class TextFakeEngine(FakeEngine):
    """FakeEngine with text slots: frame f of a text slot records the first value of its row f (PAD past the rows); a slot
    whose text is open steps only while it has a row for the frame, and that stalls every slot; once its text is final it ends
    two frames after its last row."""

    def open(self, B):
        super().open(B)
        self.text = [None] * B       # per text slot: {"rows": [...], "final": bool}
        self.pushes = []             # (slot, values, final, n_text, frames the slot had emitted)

    def admit(self, slots, prefixes, n_text, params):
        super().admit(slots, prefixes, n_text, params)
        for b, sp in zip(slots, params):
            self.text[b] = {"rows": [], "final": False} if sp.text_stream else None
            if sp.text_stream:
                self.lim[b], self.ended[b] = sp.max_frames, False

    def release(self, slots):
        super().release(slots)
        for b in slots:
            self.text[b] = None

    def push_text(self, slot, rows, final=False, n_text=0):
        t = self.text[slot]
        if t is None or t["final"] or self.ended[slot]:
            raise ValueError("not a live text slot")
        vals = [int(r[0]) for r in np.asarray(rows).reshape(-1, 1024 if np.asarray(rows).size else 1)] if np.asarray(rows).size else []
        if len(t["rows"]) + len(vals) > CAP:
            raise ValueError("rows beyond the reservation")
        self.pushes.append((slot, vals, bool(final), int(n_text), self.frames[slot]))
        t["rows"] += vals
        if final:
            t["final"] = True
            self.lim[slot] = min(self.lim[slot], len(t["rows"]) + 2)

    def _room(self):
        live = [b for b in range(self.B) if not self.ended[b] and self.text[b] is not None and not self.text[b]["final"]]
        return min([len(self.text[b]["rows"]) - self.frames[b] for b in live], default=10 ** 9)

    def text_state(self):
        rows = np.array([len(t["rows"]) if t else 0 for t in self.text], np.int32)
        starved = np.array([bool(t) and not t["final"] and not self.ended[b] and len(t["rows"]) <= self.frames[b]
                            for b, t in enumerate(self.text)])
        return rows, starved

    def run(self, n):
        return super().run(max(0, min(n, self._room())))

    def codes(self):
        out, frames = super().codes()
        for b, t in enumerate(self.text):
            if t is not None:
                for f in range(self.frames[b]):
                    out[f, b, :] = t["rows"][f] if f < len(t["rows"]) else PAD
        return out, frames


def project(ids, final=False):
    """Stand-in projection: a row's first value is its token id; the tts_eos row carries EOS_ROW."""
    vals = [int(t) for t in ids] + ([EOS_ROW] if final else [])
    return np.repeat(np.array(vals, np.float32)[:, None], 1024, axis=1).reshape(-1, 1024)


def text_prepare(msg):
    if not msg.get("text_stream"):
        return fake_prepare(msg)
    first = msg["token_ids"][0]
    base = bs.request_slot_params(msg, DEFAULTS, CAP)
    feed = bs.TextFeed(project, None, None, first[1:], 1)
    return [bs.Utterance(0, np.full((8, 4), first[0], np.float32), 0, dataclasses.replace(base, utt=0, text_stream=True), feed)]


def make(eng, prepare=text_prepare, text_wait_ms=2000.0, max_batch=2, check_every=2):
    return bs.ConcurrentScheduler(eng, max_batch, 64, prepare, fake_reply, fake_push, fake_close_stream, send_error,
                                  check_every=check_every, text_wait_ms=text_wait_ms)


def submit(sched, **req):
    srv, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    cli.settimeout(20)
    raw = bs.pack_batch_request(**req)
    ok = sched.submit(srv, json.loads(raw[4:].decode()))
    return cli, ok


def _end_codes(recs):
    ends = [r for r in recs if r[0] == "end"]
    assert len(ends) == 1 and ends[0][1] == 0
    audio = np.concatenate([r[2] for r in recs if r[0] == "audio"])
    np.testing.assert_array_equal(audio, ends[0][2][:, 0].astype(np.int16))     # the streamed records carry the same frames
    return [int(x) for x in ends[0][2][:, 0]]


def test_rows_reach_the_engine_in_order_and_before_the_frame_that_needs_them():
    eng = TextFakeEngine(step_s=0.001)
    sched = make(eng)
    cli, ok = submit(sched, token_ids=[[100, 101, 102]], stream=True, text_stream=True, max_tokens=30)
    assert ok
    sched.start()
    try:
        for ids in ([103], [104, 105, 106], [], [107]):
            time.sleep(0.01)
            cli.sendall(P.pack_text_record(P.TEXT_IDS, ids))
        half = P.pack_text_record(P.TEXT_IDS, [108, 109]) + P.pack_text_record(P.TEXT_END)
        cli.sendall(half[:9])                                # a record split across two writes
        time.sleep(0.01)
        cli.sendall(half[9:])
        codes = _end_codes(read_stream(cli))
    finally:
        sched.stop()
    text = [101, 102, 103, 104, 105, 106, 107, 108, 109, EOS_ROW]
    assert codes == text + [PAD, PAD]                        # row i at frame i, the tts_eos row last, pad afterwards
    pushed = [v for _, vals, _, _, _ in eng.pushes for v in vals]
    assert pushed == text                                    # in order, nothing twice
    seen = 0
    for _, vals, final, n_text, frames in eng.pushes:
        assert frames <= seen                                # no frame had run past the rows pushed before
        seen += len(vals)
    assert [p[2] for p in eng.pushes] == [False] * (len(eng.pushes) - 1) + [True]
    assert eng.pushes[-1][3] == 10                           # the text's 10 tokens, told with the final push
    assert eng.admitted[0][2].text_stream and eng.admitted[0][2].max_frames == 30


def test_a_starved_check_waits_and_resumes():
    eng = TextFakeEngine()
    sched = make(eng, text_wait_ms=5000.0)
    cli, _ = submit(sched, token_ids=[[200, 201]], stream=True, text_stream=True)
    other, _ = submit(sched, token_ids=[[31] * 6])           # an ordinary request beside it stalls with it and resumes
    sched.start()
    try:
        t = time.time()
        while sched.starved_checks == 0:
            assert time.time() - t < 10
            time.sleep(0.002)
        assert sched.alive
        steps = sched.frame_steps
        time.sleep(0.05)
        assert sched.frame_steps == steps == 1               # one row, one frame; the loop waits, it does not spin or stop
        cli.sendall(P.pack_text_record(P.TEXT_IDS, [202, 203]) + P.pack_text_record(P.TEXT_END))
        codes = _end_codes(read_stream(cli))
        res = bs.read_batch_reply(other)
    finally:
        sched.stop()
    assert codes == [201, 202, 203, EOS_ROW, PAD, PAD]
    np.testing.assert_array_equal(res[0][0][:, 0], 31000 + np.arange(6))
    assert sched.alive and eng.released == []


def test_a_silent_client_fails_alone_after_text_wait_ms():
    eng = TextFakeEngine()
    sched = make(eng, text_wait_ms=100.0)
    silent, _ = submit(sched, token_ids=[[300, 301, 302]], stream=True, text_stream=True)
    other, _ = submit(sched, token_ids=[[41] * 9])
    t0 = time.time()
    sched.start()
    try:
        res = bs.read_batch_reply(other)                     # answered in full although it had to wait with the silent one
        took = time.time() - t0
        with pytest.raises(RuntimeError, match="server error"):
            read_stream(silent)                              # -2 on its own connection
        assert silent.recv(1) == b""                         # ... which is then closed
    finally:
        sched.stop()
    np.testing.assert_array_equal(res[0][0][:, 0], 41000 + np.arange(9))
    slot = [b for tag, b, _ in eng.admitted if tag == 300][0]
    assert eng.released == [(slot, 2)]                       # two rows, two frames, then released
    assert 0.1 <= took < 5.0 and sched.alive
    assert sched.starved_checks >= 1


def test_a_client_that_half_closes_before_the_end_of_its_text_fails():
    eng = TextFakeEngine()
    sched = make(eng)
    cli, _ = submit(sched, token_ids=[[400, 401]], stream=True, text_stream=True)
    cli.sendall(P.pack_text_record(P.TEXT_IDS, [402]))
    cli.shutdown(socket.SHUT_WR)
    sched.start()
    try:
        with pytest.raises(RuntimeError, match="server error"):
            read_stream(cli)
    finally:
        sched.stop()
    assert [b for b, _ in eng.released] == [0] and sched.alive


def _bare_server(tokenizer=None):
    """BatchSynthesisServer._prepare without an engine: the real request checks over a small host front end."""
    r = np.random.default_rng(3)
    cfg = ModelConfig(text_vocab=64, tts_pad=61, tts_bos=62, tts_eos=63, im_start=60, assistant=59, newline=58)
    front = fe.TextFrontEnd(cfg, r.standard_normal((64, 8)).astype(np.float32), r.standard_normal((8, 8)).astype(np.float32),
                            np.zeros(8, np.float32), r.standard_normal((16, 8)).astype(np.float32), np.zeros(16, np.float32),
                            r.standard_normal((3072, 16)).astype(np.float32))
    srv = object.__new__(bs.BatchSynthesisServer)
    srv.front, srv.tokenizer, srv.cfg = front, tokenizer, cfg
    srv.max_tokens, srv.max_batch, srv.max_request, srv.n_ctx, srv.defaults = CAP, 2, 16, 96, DEFAULTS
    srv.text_voice = False
    return srv


GOOD = dict(token_ids=[[5, 6, 7]], stream=True, text_stream=True)


@pytest.mark.parametrize("bad", [dict(GOOD, stream=False), dict(GOOD, token_ids=[[5, 6], [7]]), dict(GOOD, token_ids=[[]]),
                                 dict(GOOD, token_ids=[]), dict(texts=["no tokenizer here"], stream=True, text_stream=True),
                                 dict(GOOD, max_tokens=95), dict(GOOD, vocoder="fast")])
def test_a_malformed_text_stream_request_gets_minus_two(bad):
    srv = _bare_server()
    eng = TextFakeEngine()
    sched = make(eng, prepare=srv._prepare)
    s, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    cli.settimeout(5)
    srv.n_ctx = 100 if "max_tokens" in bad else 96          # (8 prefix rows + 95 frames do not fit 100 positions)
    if "max_tokens" in bad:
        srv.max_tokens, srv.defaults = 95, dataclasses.replace(DEFAULTS, max_frames=95)
    raw = bs.pack_batch_request(**{k: v for k, v in bad.items() if k != "stream"}, stream=bad["stream"])
    assert sched.submit(s, json.loads(raw[4:].decode())) is False
    assert len(sched._queue) == 0
    assert struct.unpack("<i", cli.recv(4))[0] == P.SENTINEL_ERROR
    sched.stop()


def test_a_well_formed_request_is_prepared_with_the_streaming_prefix():
    srv = _bare_server()
    (it,) = srv._prepare(json.loads(bs.pack_batch_request(**GOOD)[4:].decode()))
    utt, prefix, n_text, params, feed = it.utt, it.prefix, it.n_text, it.params, it.feed
    assert utt == 0 and n_text == 0 and params.text_stream and params.utt == 0
    np.testing.assert_array_equal(prefix, srv.front.build_prefix_stream(5))
    rows, final = feed.take()
    np.testing.assert_array_equal(rows, fe.text_stream_rows(srv.front, [6, 7]))
    assert not final and feed.n_tokens == 3
    feed.records(P.pack_text_record(P.TEXT_IDS, [8]) + P.pack_text_record(P.TEXT_END))
    rows, final = feed.take()
    np.testing.assert_array_equal(rows, fe.text_stream_rows(srv.front, [8], final=True))
    assert final and feed.n_tokens == 4 and feed.ended


def test_text_records_go_through_the_incremental_tokeniser():
    class Words:      # stand-in for ByteLevelBPE.incremental(): one id per complete word, the open word held back
        def __init__(self):
            self.buf = b""

        def feed(self, piece):
            self.buf += piece if isinstance(piece, bytes) else piece.encode()
            *done, self.buf = self.buf.split(b" ")
            return [len(w) for w in done if w]

        def finish(self):
            w, self.buf = self.buf, b""
            return [len(w)] if w else []

    enc = Words()
    first = enc.feed("ab cde f")
    feed = bs.TextFeed(project, enc, Words, first[1:], 1)
    assert first == [2, 3]
    feed.records(P.pack_text_record(P.TEXT_BYTES, b"gh") + P.pack_text_record(P.TEXT_BYTES, b" ijkl m"))
    rows, final = feed.take()
    assert [int(r[0]) for r in rows] == [3, 3, 4] and not final          # "cde" (from the request), "fgh", "ijkl"
    feed.records(P.pack_text_record(P.TEXT_END))
    rows, final = feed.take()
    assert [int(r[0]) for r in rows] == [1, EOS_ROW] and final and feed.n_tokens == 5
    with pytest.raises(ValueError):
        feed.records(P.pack_text_record(P.TEXT_IDS, [1]))                  # nothing after the end of the text
    mixed = bs.TextFeed(project, Words(), Words, [], 1)
    with pytest.raises(ValueError):
        mixed.records(P.pack_text_record(P.TEXT_IDS, [9]))                 # ids after text: refused
