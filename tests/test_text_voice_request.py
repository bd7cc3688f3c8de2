"""batch_server --concurrent --text_voice, without a GPU: what _prepare queues for a "text_stream" request that carries a
codec prompt, what it refuses, and the scheduler driving a stand-in engine through such a request -- on _bare_server and
the fake engines of the scheduler tests.  CPU only."""
import json
import socket
import struct

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from qwen3_tts_axera_russian_amd.engine import SlotParams
from tests.test_concurrent_scheduler import CAP, fake_close_stream, fake_push, fake_reply, read_stream, send_error
from tests.test_text_stream_scheduler import PAD, TextFakeEngine, _bare_server, _end_codes

RNG = np.random.default_rng(43)
PROMPT = RNG.integers(0, 2048, size=(7, 16)).astype(np.int32)
HEAD = [11, 12, 13]
N_CTX = 96                                                   # _bare_server's


def _msg(**req):
    return json.loads(bs.pack_batch_request(**req)[4:].decode())


def _server(text_voice=True, voices=None):
    srv = _bare_server()
    srv.voices = voices or {}
    srv.text_voice = text_voice
    return srv


GOOD = dict(token_ids=[[5, 6, 7]], stream=True, text_stream=True, prompt_codes=PROMPT, prompt_token_ids=HEAD, seed=3)


def test_the_new_field_needs_a_text_slot():
    SlotParams(max_frames=4, text_stream=True, text_after_prompt=True).check(8)
    assert not SlotParams(max_frames=4).text_after_prompt
    with pytest.raises(ValueError, match="text_stream"):
        SlotParams(max_frames=4, text_after_prompt=True).check(8)


def test_prepare_queues_one_prompted_text_slot():
    srv = _server()
    items = srv._prepare(_msg(**GOOD))
    assert len(items) == 1
    (it,) = items
    assert it.feed is not None and it.utt == 0 and it.n_text == 0
    np.testing.assert_array_equal(it.prefix, srv.front.build_prefix_stream(5, HEAD))       # the prefix of 8 + len(head) rows
    assert it.prefix.shape[0] == 8 + len(HEAD)
    assert it.params.text_stream and it.params.text_after_prompt and it.params.utt == 0 and it.params.seed == 3
    assert it.params.max_frames == CAP
    it.params.check(CAP)
    assert it.prompt.dtype == np.int32
    np.testing.assert_array_equal(it.prompt, PROMPT)
    assert it.prefix_key == bs.prefix_key(b"stream", HEAD + [5], PROMPT)
    feed = it.feed
    assert isinstance(feed, bs.TextFeed) and feed.n_tokens == len(HEAD) + 3            # what the unstreamed request passes
    unstreamed = _server()._prepare(_msg(token_ids=[[5, 6, 7]], prompt_codes=PROMPT, prompt_token_ids=HEAD))
    assert unstreamed[0].n_text == feed.n_tokens
    rows, final = feed.take()
    assert rows.shape == (2, it.prefix.shape[1]) and not final                             # tokens 6 and 7 ride on frames 0 and 1
    feed.records(P.pack_text_record(P.TEXT_IDS, [8]) + P.pack_text_record(P.TEXT_END))
    rows, final = feed.take()
    assert rows.shape[0] == 2 and final and feed.n_tokens == len(HEAD) + 4
    # keys of another kind, of another head or of another prompt are other keys
    assert it.prefix_key not in (bs.prefix_key(b"stream", [5]), bs.prefix_key(b"prompt", HEAD + [5], PROMPT),
                                 bs.prefix_key(b"stream", HEAD[:-1] + [5], PROMPT), bs.prefix_key(b"stream", HEAD + [5], PROMPT[:-1]))
    # without a prompt text the prefix is the 8 rows of any text stream, the key still covers the codes
    (it,) = srv._prepare(_msg(**{k: v for k, v in GOOD.items() if k != "prompt_token_ids"}))
    np.testing.assert_array_equal(it.prefix, srv.front.build_prefix_stream(5))
    assert it.prefix_key == bs.prefix_key(b"stream", [5], PROMPT) and it.feed.n_tokens == 3 and it.params.text_after_prompt
    # an empty prompt is no prompt (the engine takes the bit without frames)
    (it,) = srv._prepare(_msg(**dict(GOOD, prompt_codes=[])))
    assert it.prompt is None and it.params.text_after_prompt and it.prefix.shape[0] == 8 + len(HEAD)
    # a request without any prompt key is the text-stream request it always was
    (it,) = srv._prepare(_msg(token_ids=[[5, 6, 7]], stream=True, text_stream=True))
    assert it.prompt is None and not it.params.text_after_prompt and it.prefix_key == bs.prefix_key(b"stream", [5])
    np.testing.assert_array_equal(it.prefix, srv.front.build_prefix_stream(5))


def test_a_voice_stands_for_its_codes(tmp_path):
    d = tmp_path / "anna"
    d.mkdir()
    np.save(d / "ref_codec_tokens.npy", PROMPT.astype(np.int64))
    srv = _server(voices={"anna": bs.load_voice(str(d))})
    (a,) = srv._prepare(_msg(token_ids=[[5, 6]], stream=True, text_stream=True, voice="anna"))
    (b,) = srv._prepare(_msg(token_ids=[[5, 6]], stream=True, text_stream=True, prompt_codes=PROMPT))
    np.testing.assert_array_equal(a.prefix, b.prefix)
    np.testing.assert_array_equal(a.prompt, b.prompt)
    assert a.prefix_key == b.prefix_key and a.params == b.params


def test_the_longest_prompt_that_fits_is_queued():
    srv = _server()
    T = N_CTX - 8 - len(HEAD) - CAP
    (it,) = srv._prepare(_msg(**dict(GOOD, prompt_codes=np.zeros((T, 16), np.int32))))
    assert it.prompt.shape == (T, 16) and it.prefix.shape[0] == 8 + len(HEAD)


BAD = [
    dict(voice="nobody"),
    dict(voice="anna"),                                                                # with the inline keys of GOOD
    dict(prompt_codes=None),                                                           # a prompt text without a prompt
    dict(prompt_token_ids=[1, "2"]),
    dict(prompt_token_ids=None, prompt_text="no tokenizer here"),
    dict(prompt_codes=[[1] * 15]),
    dict(prompt_codes=[[0] * 15 + [2048]]),
    dict(prompt_codes=[[-1] + [0] * 15]),
    dict(prompt_codes="abc"),
    dict(prompt_codes=[PROMPT.tolist()] * 2),                                          # 2 prompts for the one utterance
    dict(prompt_codes=np.zeros((N_CTX - 8 - len(HEAD) - CAP + 1, 16), np.int32)),      # one frame more than n_ctx takes
    dict(stream=False),
    dict(token_ids=[[5, 6], [7]]),
    dict(token_ids=[[]]),
]


class VoiceFakeEngine(TextFakeEngine):
    """TextFakeEngine whose admit takes prompts like FrameEngine.admit and whose rows may be of any width: frame f of a text
    slot records 100 + f while it has a row for it."""

    def open(self, B):
        super().open(B)
        self.calls = []          # (slots, params, prompts or "absent") per admit call
        self.rows = {}           # slot -> the rows pushed, as they came

    def admit(self, slots, prefixes, n_text, params, prompts="absent"):
        super().admit(slots, prefixes, n_text, params)
        self.calls.append((list(slots), list(params), prompts, [np.array(p) for p in prefixes]))
        for b in slots:
            self.rows[b] = []

    def push_text(self, slot, rows, final=False, n_text=0):
        rows = np.asarray(rows, np.float32)
        real = list(rows.reshape(-1, rows.shape[-1])) if rows.size else []
        k = len(self.rows[slot])
        stand_in = np.repeat(np.arange(100 + k, 100 + k + len(real), dtype=np.float32)[:, None], 1024, axis=1)
        super().push_text(slot, stand_in, final, n_text)
        self.rows[slot] += real


def make(eng, prepare, max_batch=2):
    return bs.ConcurrentScheduler(eng, max_batch, 64, prepare, fake_reply, fake_push, fake_close_stream, send_error, check_every=2,
                                  text_wait_ms=5000.0)


def _submit(sched, msg):
    s, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    cli.settimeout(20)
    return cli, sched.submit(s, msg)


def _raw_msg(bad):
    raw = ("prompt_codes", "prompt_token_ids")               # as a client that does not use pack_batch_request may send them
    merged = dict(GOOD, **bad)
    msg = _msg(**{k: v for k, v in merged.items() if k not in raw})
    msg.update({k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in merged.items() if k in raw and v is not None})
    return msg


@pytest.mark.parametrize("bad", BAD)
def test_a_malformed_request_is_refused_before_anything_is_queued(bad):
    srv = _server(voices={"anna": (PROMPT.tolist(), None)})
    eng = VoiceFakeEngine()
    sched = make(eng, srv._prepare)
    cli, ok = _submit(sched, _raw_msg(bad))
    assert ok is False
    assert len(sched._queue) == 0 and not hasattr(eng, "calls")
    assert struct.unpack("<i", cli.recv(4))[0] == P.SENTINEL_ERROR
    sched.stop()


def test_without_text_voice_it_is_refused_as_before():
    for srv in (_server(text_voice=False), _bare_server()):          # the flag off, and a server that never heard of it
        srv.voices = {"anna": (PROMPT.tolist(), None)}
        for req in (GOOD, dict(token_ids=[[5, 6]], stream=True, text_stream=True, voice="anna")):
            with pytest.raises(ValueError, match='a codec prompt does not combine with "text_stream"'):
                srv._prepare(_raw_msg(req) if req is GOOD else _msg(**req))
            with pytest.raises(ValueError, match='a codec prompt does not combine with "text_stream"'):
                srv._request_prompts(_msg(**req), 1)
    eng = VoiceFakeEngine()
    sched = make(eng, _server(text_voice=False)._prepare)
    cli, ok = _submit(sched, _raw_msg({}))
    assert ok is False and len(sched._queue) == 0
    assert struct.unpack("<i", cli.recv(4))[0] == P.SENTINEL_ERROR
    sched.stop()


def test_the_scheduler_admits_it_with_both_bits_feeds_rows_and_finishes():
    srv = _server()
    eng = VoiceFakeEngine()
    sched = make(eng, srv._prepare)
    cli, ok = _submit(sched, _raw_msg(dict(max_tokens=30)))
    assert ok
    other, ok = _submit(sched, _msg(token_ids=[[31] * 6]))           # an ordinary request beside it (a plain prefix)
    assert ok
    sched.start()
    try:
        cli.sendall(P.pack_text_record(P.TEXT_IDS, [8, 9]))
        cli.sendall(P.pack_text_record(P.TEXT_IDS, [10]) + P.pack_text_record(P.TEXT_END))
        codes = _end_codes(read_stream(cli))
        res = bs.read_batch_reply(other)
    finally:
        sched.stop()
    # rows: tokens 6, 7, 8, 9, 10 and the tts_eos row, one per generated frame from frame 0; then the fake's two pad frames
    assert codes == [100, 101, 102, 103, 104, 105, PAD, PAD]
    assert res[0][0].shape[0] == 6
    slots, params, prompts, prefixes = next(c for c in eng.calls if any(p.text_stream for p in c[1]))
    at = [i for i, p in enumerate(params) if p.text_stream][0]
    p = params[at]
    assert p.text_after_prompt and p.max_frames == 30
    assert (1 if p.text_stream else 0) | (2 if p.text_after_prompt else 0) == 3          # q3e_slot_params.reserved
    assert prompts != "absent" and len(prompts) == len(slots)
    np.testing.assert_array_equal(prompts[at], PROMPT)
    assert all(q is None for i, q in enumerate(prompts) if i != at)
    np.testing.assert_array_equal(prefixes[at], srv.front.build_prefix_stream(5, HEAD))
    from qwen3_tts_axera_russian_amd.frontend import text_stream_rows
    np.testing.assert_array_equal(np.stack(eng.rows[slots[at]]), text_stream_rows(srv.front, [6, 7, 8, 9, 10], final=True))
    assert [x[2] for x in eng.pushes][-1] is True and eng.pushes[-1][3] == len(HEAD) + 6   # n_text_total: head + the text
    assert sched.alive and eng.released == []
