"""batch_server --concurrent --prefix_cache without a GPU: the keys the server derives (prefix_key, _prepare,
_prepare_text_stream) and how ConcurrentScheduler hands them to the engine, against a stand-in engine in the style of
tests/test_concurrent_scheduler.py.  CPU only."""
import dataclasses
import json

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from tests.test_concurrent_scheduler import (FakeEngine, fake_close_stream, fake_prepare, fake_push, fake_reply, read_stream,
                                             send_error, submit)
from tests.test_text_stream_scheduler import _bare_server


class KeyedFakeEngine(FakeEngine):
    """FakeEngine whose admit takes keys like FrameEngine.admit: a key is a hit once an earlier utterance (of this call or
    an earlier one) has brought it."""

    def __init__(self):
        super().__init__()
        self.calls = []          # (slots, tags, keys) per admit call
        self.seen = set()

    def admit(self, slots, prefixes, n_text, params, keys=None):
        super().admit(slots, prefixes, n_text, params)
        self.calls.append((list(slots), [int(p[0, 0]) for p in prefixes], None if keys is None else list(keys)))
        if keys is None:
            return None
        hit = []
        for k in keys:
            hit.append(k is not None and k in self.seen)
            if k is not None:
                self.seen.add(k)
        return np.array(hit, bool)


def keyed_prepare(msg):
    """fake_prepare with the server's keys: the tag (first token id) rides in the prefix, the key covers all ids."""
    return [dataclasses.replace(it, prefix_key=bs.prefix_key(b"full", msg["token_ids"][it.utt])) for it in fake_prepare(msg)]


def make(eng, prepare, prefix_cache, max_batch=2):
    return bs.ConcurrentScheduler(eng, max_batch, 64, prepare, fake_reply, fake_push, fake_close_stream, send_error,
                                  check_every=2, prefix_cache=prefix_cache)


def test_keys_are_a_function_of_the_kind_and_the_token_ids():
    k = bs.prefix_key(b"full", [5, 6, 7])
    assert isinstance(k, bytes) and len(k) == 16 and k != bytes(16)
    assert bs.prefix_key(b"full", [5, 6, 7]) == k == bs.prefix_key(b"full", np.array([5, 6, 7], np.int64))
    assert bs.prefix_key(b"stream", [5, 6, 7]) != k
    assert bs.prefix_key(b"full", [5, 6]) != k and bs.prefix_key(b"full", [5, 6, 8]) != k and bs.prefix_key(b"full", [7, 6, 5]) != k
    assert bs.prefix_key(b"full", [5]) != bs.prefix_key(b"stream", [5])
    assert bs.prefix_key(b"full", [1, 0]) != bs.prefix_key(b"full", [1])          # no token is padding


def test_prepare_attaches_the_key_of_each_utterance():
    srv = _bare_server()
    ids = [[5, 6, 7], [9], [5, 6, 7]]
    items = srv._prepare(json.loads(bs.pack_batch_request(token_ids=ids, seed=3)[4:].decode()))
    assert [it.feed for it in items] == [None, None, None]                         # the plain utterances the scheduler always took
    assert [it.prefix_key for it in items] == [bs.prefix_key(b"full", ids[it.utt]) for it in items]
    by_utt = {it.utt: it for it in items}
    assert by_utt[0].prefix_key == by_utt[2].prefix_key != by_utt[1].prefix_key   # two takes of one text share the prefill
    assert (by_utt[0].params.utt, by_utt[2].params.utt) == (0, 2)                          # ... and keep their own draw streams
    # a client cannot supply a key
    forged = dict(json.loads(bs.pack_batch_request(token_ids=ids)[4:].decode()), prefix_key="00" * 16, keys=["00" * 16] * 3)
    assert [it.prefix_key for it in srv._prepare(forged)] == [it.prefix_key for it in items]


def test_a_text_stream_key_depends_on_the_first_token_alone():
    srv = _bare_server()

    def key(first_piece):
        (item,) = srv._prepare(json.loads(bs.pack_batch_request(token_ids=[first_piece], stream=True, text_stream=True)[4:].decode()))
        assert item.feed is not None and item.params.text_stream
        return item.prefix_key

    assert key([5, 6, 7]) == key([5]) == key([5, 9, 9, 9]) == bs.prefix_key(b"stream", [5])
    assert key([6, 6, 7]) != key([5, 6, 7])
    (full,) = srv._prepare(json.loads(bs.pack_batch_request(token_ids=[[5]])[4:].decode()))
    assert full.prefix_key != key([5])                                             # another prefix for the same token


def test_keys_reach_admit_in_slot_order_and_the_counters_add_up():
    eng = KeyedFakeEngine()
    sched = make(eng, keyed_prepare, prefix_cache=True, max_batch=3)
    reqs = [[[11, 1, 1], [12, 2], [11, 1, 1]],          # the third repeats the first: a hit in the same admission
            [[12, 2], [13, 3, 3, 3]],                   # the first repeats an utterance of the request before
            [[11, 1, 1]]]
    clients = [submit(sched, token_ids=ids) for ids in reqs[:2]] + [submit(sched, token_ids=reqs[2], stream=True)]
    sched.start()
    try:
        replies = [bs.read_batch_reply(c) for c in clients[:2]]
        read_stream(clients[2])
    finally:
        sched.stop()
    assert [len(r) for r in replies] == [3, 2]
    want = {ids[0]: bs.prefix_key(b"full", ids) for req in reqs for ids in req}
    admitted = 0
    for slots, tags, keys in eng.calls:
        assert slots == sorted(slots) and len(keys) == len(slots)
        assert keys == [want[t] for t in tags]           # key u belongs to the utterance that goes into slots[u]
        admitted += len(slots)
    assert admitted == 6
    assert [t for _, tags, _ in eng.calls for t in tags] == [11, 12, 11, 12, 13, 11]   # FIFO, as without the cache
    assert (sched.prefix_hits, sched.prefix_misses) == (3, 3)
    assert sched.prefix_hits + sched.prefix_misses == admitted


def test_an_item_without_a_key_is_admitted_uncached():
    eng = KeyedFakeEngine()
    sched = make(eng, fake_prepare, prefix_cache=True)                              # plain utterances: no prefix key
    cli = submit(sched, token_ids=[[21, 1], [21, 1]])
    sched.start()
    try:
        assert len(bs.read_batch_reply(cli)) == 2
    finally:
        sched.stop()
    assert [keys for _, _, keys in eng.calls] == [[None, None]]
    assert (sched.prefix_hits, sched.prefix_misses) == (0, 2)


@pytest.mark.parametrize("prepare", [fake_prepare, keyed_prepare])
def test_without_the_option_admit_is_called_as_before(prepare):
    eng = FakeEngine()                                   # admit(slots, prefixes, n_text, params): any further argument is a TypeError
    sched = make(eng, prepare, prefix_cache=False)
    cli = submit(sched, token_ids=[[31, 1, 1], [31, 1, 1], [32]])
    sched.start()
    try:
        res = bs.read_batch_reply(cli)
    finally:
        sched.stop()
    assert sched.alive and len(res) == 3
    assert [t for t, _, _ in eng.admitted] == [31, 31, 32]
    assert (sched.prefix_hits, sched.prefix_misses) == (0, 0)
    default = bs.ConcurrentScheduler(eng, 2, 64, prepare, fake_reply, fake_push, fake_close_stream, send_error)
    assert default.prefix_cache is False
    default._pool.shutdown()


def test_the_server_refuses_the_option_without_concurrent():
    with pytest.raises(ValueError, match="--concurrent"):
        bs.BatchSynthesisServer("none.q3w", "none.q3w", prefix_cache=4)
    with pytest.raises(ValueError, match="prefix_cache"):
        bs.BatchSynthesisServer("none.q3w", "none.q3w", concurrent=True, prefix_cache=-1)
