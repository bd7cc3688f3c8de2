"""batch_server --concurrent with codec prompts, without a GPU: the request keys ("prompt_codes", "prompt_token_ids",
"voice"), the key of a prompted prefix, what _prepare queues and refuses, and how ConcurrentScheduler hands the prompts to
the engine -- against a stand-in engine in the style of tests/test_concurrent_scheduler.py.  CPU only."""
import json
import socket
import struct

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from tests.test_concurrent_scheduler import (CAP, FakeEngine, fake_close_stream, fake_push, fake_reply, send_error)
from tests.test_text_stream_scheduler import _bare_server

RNG = np.random.default_rng(41)
PROMPT = RNG.integers(0, 2048, size=(7, 16)).astype(np.int32)
OTHER = RNG.integers(0, 2048, size=(3, 16)).astype(np.int32)


def _msg(**req):
    return json.loads(bs.pack_batch_request(**req)[4:].decode())


def _server(voices=None):
    srv = _bare_server()
    srv.voices = voices or {}
    return srv


def test_the_key_of_a_prompted_prefix_covers_ids_and_codes():
    ids = [5, 6, 7]
    k = bs.prefix_key(b"prompt", ids, PROMPT)
    assert isinstance(k, bytes) and len(k) == 16
    assert k == bs.prefix_key(b"prompt", np.array(ids, np.int64), PROMPT.astype(np.int64).tolist())
    assert bs.prefix_key(b"prompt", [5, 6, 8], PROMPT) != k and bs.prefix_key(b"prompt", [5, 6], PROMPT) != k
    seen = {k}
    for f in range(PROMPT.shape[0]):                     # any single id of the prompt
        for g in range(16):
            q = PROMPT.copy()
            q[f, g] = (q[f, g] + 1) % 2048
            kk = bs.prefix_key(b"prompt", ids, q)
            assert kk not in seen
            seen.add(kk)
    assert bs.prefix_key(b"prompt", ids, PROMPT[:-1]) not in seen
    # nothing of kind b"full" (nor b"stream"): not the ids alone, not the ids followed by the codes as if they were ids
    flat = ids + [int(x) for x in PROMPT.reshape(-1)]
    for kind in (b"full", b"stream"):
        assert bs.prefix_key(kind, ids) not in seen and bs.prefix_key(kind, flat) not in seen
        assert bs.prefix_key(kind, [len(ids)] + flat) not in seen
    # where the text ends and the codes begin is part of the key
    assert bs.prefix_key(b"prompt", ids + [int(PROMPT[0, 0])], PROMPT) != k
    # the keys the server has always derived are what they were
    import hashlib
    assert bs.prefix_key(b"full", ids) == hashlib.sha256(b"full\0" + np.asarray(ids, "<i4").tobytes()).digest()[:16]


def test_prepare_queues_the_prompt_beside_the_tuple():
    srv = _server()
    ids = [[5, 6, 7], [9], [5, 6, 7]]
    items = srv._prepare(_msg(token_ids=ids, seed=3, prompt_codes=PROMPT, prompt_token_ids=[11, 12]))
    assert [it.feed for it in items] == [None, None, None]                         # no text feed: the plain utterance
    for it in items:
        full = [11, 12] + ids[it.utt]
        np.testing.assert_array_equal(it.prefix, srv.front.build_prefix(full))         # the prompt's text in front
        assert it.n_text == len(full)                                                  # n_text counts both
        assert it.params.utt == it.utt and it.params.max_frames == CAP and it.params.seed == 3
        assert it.prompt.dtype == np.int32 and it.prompt.shape == (7, 16)
        np.testing.assert_array_equal(it.prompt, PROMPT)
        assert it.prefix_key == bs.prefix_key(b"prompt", full, PROMPT)
    # one prompt per utterance; an empty one is no prompt, and its key is the plain one
    items = srv._prepare(_msg(token_ids=ids, prompt_codes=[PROMPT.tolist(), [], OTHER.tolist()]))
    by_utt = {it.utt: it for it in items}
    np.testing.assert_array_equal(by_utt[0].prompt, PROMPT)
    np.testing.assert_array_equal(by_utt[2].prompt, OTHER)
    assert by_utt[1].prompt is None and by_utt[1].prefix_key == bs.prefix_key(b"full", ids[1])
    assert by_utt[0].prefix_key != by_utt[2].prefix_key
    # without the keys nothing changes
    plain = srv._prepare(_msg(token_ids=ids, seed=3))
    assert all(it.prompt is None and it.prefix_key == bs.prefix_key(b"full", ids[it.utt]) for it in plain)


def test_a_voice_stands_for_its_codes_and_text(tmp_path):
    d = tmp_path / "anna"
    d.mkdir()
    np.save(d / "ref_codec_tokens.npy", PROMPT.astype(np.int64))     # what encode_reference_audio --output_dir writes
    srv = _server({"anna": bs.load_voice(str(d))})
    ids = [[5, 6, 7], [9]]
    by_voice = srv._prepare(_msg(token_ids=ids, voice="anna"))
    inline = srv._prepare(_msg(token_ids=ids, prompt_codes=PROMPT))
    for a, b in zip(by_voice, inline):
        np.testing.assert_array_equal(a.prefix, b.prefix)
        np.testing.assert_array_equal(a.prompt, b.prompt)
        assert (a.utt, a.n_text, a.params, a.feed) == (b.utt, b.n_text, b.params, b.feed) and a.prefix_key == b.prefix_key
    (d / "ref_text.txt").write_text("spoken in the clip")
    codes, text = bs.load_voice(str(d))
    assert text == "spoken in the clip" and codes == PROMPT.tolist()
    srv = _server({"anna": (codes, text)})
    with pytest.raises(RuntimeError, match="tokenizer"):          # the text needs the tokeniser this bare server lacks
        srv._prepare(_msg(token_ids=ids, voice="anna"))

    class Words:                                                  # (stands where the byte-level BPE stands)
        @staticmethod
        def encode(text, add_special_tokens=False):
            return [len(w) for w in text.split()]
    srv.tokenizer = Words()
    by_voice = srv._prepare(_msg(token_ids=ids, voice="anna"))
    inline = srv._prepare(_msg(token_ids=ids, prompt_codes=PROMPT, prompt_token_ids=[6, 2, 3, 4]))
    for a, b in zip(by_voice, inline):
        np.testing.assert_array_equal(a.prefix, b.prefix)
        assert a.n_text == b.n_text == 4 + len(ids[a.utt]) and a.prefix_key == b.prefix_key


BAD = [
    dict(prompt_codes=PROMPT, stream=True, text_stream=True, token_ids=[[5, 6]]),     # with "text_stream"
    dict(voice="nobody"),
    dict(voice="anna", prompt_codes=PROMPT),                                           # one or the other
    dict(prompt_token_ids=[1, 2]),                                                     # a prompt text without a prompt
    dict(prompt_codes=PROMPT, prompt_token_ids=[1, "2"]),
    dict(prompt_codes=PROMPT, prompt_text="no tokenizer here"),
    dict(prompt_codes=[[1] * 15]),                                                     # a frame of 15 ids
    dict(prompt_codes=[[1.5] * 16]),
    dict(prompt_codes=[[True] * 16]),
    dict(prompt_codes=[[0] * 15 + [2048]]),
    dict(prompt_codes=[[2048] + [0] * 15]),
    dict(prompt_codes=[[-1] + [0] * 15]),
    dict(prompt_codes="abc"),
    dict(prompt_codes=[PROMPT.tolist()] * 3),                                          # 3 prompts for 2 utterances
    dict(prompt_codes=np.zeros((96 - 12 - CAP + 1, 16), np.int32)),                    # one frame more than n_ctx takes
]


@pytest.mark.parametrize("bad", BAD)
def test_a_malformed_prompt_is_refused_before_anything_is_queued(bad):
    srv = _server({"anna": (PROMPT.tolist(), None)})
    eng = PromptFakeEngine()
    sched = make(eng, srv._prepare)
    s, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    cli.settimeout(5)
    raw = ("prompt_codes", "prompt_token_ids")           # as a client that does not use pack_batch_request may send them
    msg = _msg(**dict(dict(token_ids=[[5, 6, 7], [9]]), **{k: v for k, v in bad.items() if k not in raw}))
    msg.update({k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in bad.items() if k in raw})
    assert sched.submit(s, msg) is False
    assert len(sched._queue) == 0 and eng.calls == []
    assert struct.unpack("<i", cli.recv(4))[0] == P.SENTINEL_ERROR
    sched.stop()


def test_the_longest_prompt_that_fits_is_queued():
    srv = _server()
    T = 96 - 12 - CAP                                    # n_ctx 96, 9 + 3 prefix rows, max_tokens CAP
    (it,) = srv._prepare(_msg(token_ids=[[5, 6, 7]], prompt_codes=np.zeros((T, 16), np.int32)))
    assert it.prefix.shape[0] == 12 and it.prompt.shape == (T, 16)


class PromptFakeEngine(FakeEngine):
    """FakeEngine whose admit takes prompts like FrameEngine.admit."""

    def __init__(self):
        super().__init__()
        self.calls = []          # (slots, tags, prompts or "absent") per admit call

    def admit(self, slots, prefixes, n_text, params, prompts="absent"):
        super().admit(slots, prefixes, n_text, params)
        self.calls.append((list(slots), [int(p[0, 0]) for p in prefixes], prompts))


def tagged_prepare(msg):
    """fake_prepare's tuples (the tag rides in the prefix) with the request's prompts beside them."""
    import dataclasses
    from tests.test_concurrent_scheduler import DEFAULTS
    base = bs.request_slot_params(msg, DEFAULTS, CAP)
    ids = msg["token_ids"]
    prompts = bs.request_prompt_codes(msg["prompt_codes"], len(ids)) if msg.get("prompt_codes") is not None else [None] * len(ids)
    return [bs.Utterance(i, np.full((2, 4), t[0], np.float32), len(t), dataclasses.replace(base, utt=i), prompt=prompts[i])
            for i, t in enumerate(ids)]


def make(eng, prepare, max_batch=2):
    return bs.ConcurrentScheduler(eng, max_batch, 64, prepare, fake_reply, fake_push, fake_close_stream, send_error, check_every=2)


def test_prompts_reach_admit_in_queue_order():
    eng = PromptFakeEngine()
    sched = make(eng, tagged_prepare, max_batch=2)
    clients = []
    for req in (dict(token_ids=[[1] * 4, [2] * 4], prompt_codes=[PROMPT.tolist(), []]),
                dict(token_ids=[[3] * 4]),
                dict(token_ids=[[4] * 4], prompt_codes=OTHER)):
        s, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
        cli.settimeout(20)
        assert sched.submit(s, _msg(**req)) is True
        clients.append(cli)
    sched.start()
    try:
        replies = [bs.read_batch_reply(c) for c in clients]
    finally:
        sched.stop()
    assert [len(r) for r in replies] == [2, 1, 1]
    assert [int(r[0][0][0, 0]) // 1000 for r in replies] == [1, 3, 4]                # every reply is its own request's
    tags = [t for _, ts, _ in eng.calls for t in ts]
    assert tags == [1, 2, 3, 4]                                                     # FIFO across requests
    got = {}
    for slots, ts, prompts in eng.calls:
        if prompts == "absent":                          # an admission without any prompt is called as it always was
            got.update({t: "absent" for t in ts})
            continue
        assert len(prompts) == len(slots)
        got.update(dict(zip(ts, prompts)))
    np.testing.assert_array_equal(got[1], PROMPT)
    np.testing.assert_array_equal(got[4], OTHER)
    assert got[2] is None                                # beside a prompted utterance: None
    assert got[3] is None or got[3] == "absent"
