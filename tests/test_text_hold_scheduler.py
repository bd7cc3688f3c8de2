"""batch_server --concurrent --text_hold without a GPU: the scheduler against the stand-in engine of
tests/test_text_stream_scheduler.py with the engine's hold bookkeeping (include/qwen3tts_engine.h, q3e_text_hold): a text
slot without a row for its next frame is held while the others step; a text slot without a frame and without a row stalls
every slot.  CPU only."""
import time

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from tests.test_concurrent_scheduler import fake_close_stream, fake_push, fake_reply, read_stream, send_error
from tests.test_text_stream_scheduler import EOS_ROW, PAD, TextFakeEngine, _end_codes, submit, text_prepare


class HoldFakeEngine(TextFakeEngine):
    """TextFakeEngine in hold mode: per step a live text slot before its final push with 1 <= frames, frames >= rows and
    frames < budget is held (it emits nothing, held[b] counts it); run(n) takes min(n, the most steps a live slot can use)
    steps, and none while a live text slot has neither a frame nor a row."""

    def open(self, B):
        super().open(B)
        self.held = [0] * B
        self.age0_stalls = 0         # run() calls that took no step because a text slot had no frame and no row
        self.steps_beside_held = 0   # steps in which one slot was held and another one emitted a frame

    def admit(self, slots, prefixes, n_text, params):
        super().admit(slots, prefixes, n_text, params)
        for b in slots:
            self.held[b] = 0

    def _waits(self, b):
        return not self.ended[b] and self.text[b] is not None and not self.text[b]["final"]

    def _is_held(self, b):
        return self._waits(b) and 1 <= self.frames[b] < self.lim[b] and self.frames[b] >= len(self.text[b]["rows"])

    def held_steps(self):
        return np.array(self.held, np.int64)

    def run(self, n):
        live = [b for b in range(self.B) if not self.ended[b]]
        if any(self._waits(b) and self.frames[b] == 0 and not self.text[b]["rows"] for b in live):
            self.age0_stalls += 1
            return 0
        room = max([(min(len(self.text[b]["rows"]), self.lim[b]) if self._waits(b) else self.lim[b]) - self.frames[b]
                    for b in live], default=0)
        steps = 0
        while steps < min(n, room):
            held = [b for b in live if self._is_held(b)]
            moved = [b for b in live if not self.ended[b] and b not in held]
            for b in held:
                self.held[b] += 1
            for b in moved:
                self.frames[b] += 1
                self.ended[b] = self.frames[b] >= self.lim[b]
            self.steps_beside_held += bool(held and moved)
            steps += 1
            if self.step_s:
                time.sleep(self.step_s)
        return steps


def make(eng, text_wait_ms=5000.0, max_batch=2, check_every=2):
    return bs.ConcurrentScheduler(eng, max_batch, 64, text_prepare, fake_reply, fake_push, fake_close_stream, send_error,
                                  check_every=check_every, text_wait_ms=text_wait_ms, text_hold=True)


def _until(cond, what):
    t = time.time()
    while not cond():
        assert time.time() - t < 10, what
        time.sleep(0.002)


def test_admission_waits_for_the_first_row_and_later_requests_pass():
    eng = HoldFakeEngine()
    sched = make(eng)
    cli, ok = submit(sched, token_ids=[[100]], stream=True, text_stream=True)      # one token: the prefix, no row yet
    assert ok
    other, _ = submit(sched, token_ids=[[31] * 6])
    sched.start()
    try:
        res = bs.read_batch_reply(other)                     # submitted later, admitted first, answered in full
        assert [tag for tag, _, _ in eng.admitted] == [31] and sched.alive
        cli.sendall(P.pack_text_record(P.TEXT_IDS, [101]))   # the first row: now it is admitted
        _until(lambda: len(eng.admitted) == 2, "the text request was not admitted with its first row")
        cli.sendall(P.pack_text_record(P.TEXT_IDS, [102]) + P.pack_text_record(P.TEXT_END))
        codes = _end_codes(read_stream(cli))
    finally:
        sched.stop()
    np.testing.assert_array_equal(res[0][0][:, 0], 31000 + np.arange(6))
    assert codes == [101, 102, EOS_ROW, PAD, PAD]
    assert [tag for tag, _, _ in eng.admitted] == [31, 100]
    assert eng.age0_stalls == 0                              # the engine never saw a text slot without a frame and a row
    assert eng.pushes[0][4] == 0 and eng.pushes[0][1] == [101]


def test_the_end_record_alone_admits_a_one_token_text():
    eng = HoldFakeEngine()
    sched = make(eng)
    cli, _ = submit(sched, token_ids=[[150]], stream=True, text_stream=True)
    cli.sendall(P.pack_text_record(P.TEXT_END))
    sched.start()
    try:
        codes = _end_codes(read_stream(cli))
    finally:
        sched.stop()
    assert codes == [EOS_ROW, PAD, PAD] and eng.age0_stalls == 0


def test_frames_of_another_request_keep_coming_while_a_text_slot_is_held():
    eng = HoldFakeEngine()
    sched = make(eng)
    cli, _ = submit(sched, token_ids=[[200, 201]], stream=True, text_stream=True)   # one row, then silence
    other, _ = submit(sched, token_ids=[[31] * 30])
    sched.start()
    try:
        res = bs.read_batch_reply(other)                     # all 30 frames although the text client sends nothing
        slot = [b for tag, b, _ in eng.admitted if tag == 200][0]
        assert eng.frames[slot] == 1 and eng.held[slot] >= 29 and eng.steps_beside_held >= 29
        _until(lambda: sched.starved_checks > 0, "alone and held, the text slot's checks run no frame")
        steps = sched.frame_steps
        cli.sendall(P.pack_text_record(P.TEXT_IDS, [202, 203]) + P.pack_text_record(P.TEXT_END))
        codes = _end_codes(read_stream(cli))
    finally:
        sched.stop()
    np.testing.assert_array_equal(res[0][0][:, 0], 31000 + np.arange(30))
    assert codes == [201, 202, 203, EOS_ROW, PAD, PAD]
    assert steps == 30                                       # no step was run for the held slot alone
    assert sched.held_steps == eng.held[slot] == 29 and sched.alive and eng.released == []


def test_a_silent_client_fails_alone_after_text_wait_ms():
    eng = HoldFakeEngine(step_s=0.001)
    sched = make(eng, text_wait_ms=100.0)
    silent, _ = submit(sched, token_ids=[[300, 301, 302]], stream=True, text_stream=True)
    other, _ = submit(sched, token_ids=[[41] * 9])
    alone_eng = HoldFakeEngine()
    alone = make(alone_eng)
    ref_cli, _ = submit(alone, token_ids=[[41] * 9])
    alone.start()
    try:
        ref = bs.read_batch_reply(ref_cli)
    finally:
        alone.stop()
    sched.start()
    try:
        res = bs.read_batch_reply(other)
        with pytest.raises(RuntimeError, match="server error"):
            read_stream(silent)                              # -2 on its own connection
        assert silent.recv(1) == b""                         # ... which is then closed
    finally:
        sched.stop()
    np.testing.assert_array_equal(res[0][0], ref[0][0])      # the codes it gets alone
    np.testing.assert_array_equal(res[0][0][:, 0], 41000 + np.arange(9))
    slot = [b for tag, b, _ in eng.admitted if tag == 300][0]
    assert eng.released == [(slot, 2)]                       # two rows, two frames, held, then released
    assert sched.alive and sched.held_steps == eng.held[slot] > 0


def test_a_hang_up_while_queued_without_a_row_is_dropped():
    eng = HoldFakeEngine()
    sched = make(eng)
    cli, _ = submit(sched, token_ids=[[500]], stream=True, text_stream=True)
    cli.close()
    other, _ = submit(sched, token_ids=[[51] * 4])
    sched.start()
    try:
        res = bs.read_batch_reply(other)
        _until(lambda: len(sched._queue) == 0, "the request of a client that left stayed queued")
    finally:
        sched.stop()
    np.testing.assert_array_equal(res[0][0][:, 0], 51000 + np.arange(4))
    assert [tag for tag, _, _ in eng.admitted] == [51] and sched.alive
