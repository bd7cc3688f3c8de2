"""batch_server --concurrent --prefix_cache end to end over the socket, on the tiny packs of tests/test_gpu_concurrent.py:
repeated requests are served from the prefix cache, and every reply -- codes and PCM -- is bit for bit the reply of a server
started without the option."""
import os
import threading
import time

import numpy as np
import pytest

from tests.test_gpu_concurrent import LONG, SAMPLE_KEYS, _call, packs  # noqa: F401 -- (packs: the fixture)
from tests.test_gpu_text_stream import _text_call

pytestmark = pytest.mark.gpu

REPEATED = dict(token_ids=[LONG[:12]], max_tokens=30, seed=5, **SAMPLE_KEYS)
TAKES = dict(token_ids=[LONG[4:15], LONG[4:15]], max_tokens=25, seed=9, **SAMPLE_KEYS)
TEXT_A = [LONG[:2], LONG[2:10]]                          # two text-stream requests that begin with the same token
TEXT_B = [LONG[:1], [44, 45, 46], [301, 302]]


def _server(packs, sock, prefix_cache):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    main, voc = packs
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=160, max_tokens=80, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, concurrent=True, prefix_cache=prefix_cache, prefix_cache_rows=48)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(400):
        if os.path.exists(sock) and srv.sched is not None:
            break
        time.sleep(0.05)
    return srv, th


def _stop(srv, th):
    """-> the engine's prefix-cache counters once the engine thread has stopped."""
    srv._running = False
    th.join(timeout=60)
    assert not th.is_alive()
    stats = srv.eng.prefix_stats()
    srv.close()
    return stats


def _session(sock, sched=None):
    """The requests of this test, one after the other -> (replies as lists of (codes, pcm), hits gained by each repeated case)."""
    replies, gained = [], []

    def hits():
        return sched.prefix_hits if sched is not None else 0

    h = hits()
    replies.append(_call(sock, REPEATED))
    replies.append(_call(sock, dict(REPEATED, stream=True)))             # the same request again (its records joined)
    gained.append(hits() - h)
    h = hits()
    replies.append([_text_call(sock, TEXT_A, 0.0, max_tokens=30)])
    replies.append([_text_call(sock, TEXT_A, 0.0, max_tokens=30)])       # the same text-stream request again
    replies.append([_text_call(sock, TEXT_B, 0.0, max_tokens=30, seed=3, **SAMPLE_KEYS)])   # another text, the same first token
    gained.append(hits() - h)
    h = hits()
    replies.append(_call(sock, TAKES))                                   # one text listed twice with a seed
    gained.append(hits() - h)
    return replies, gained


def test_replies_with_the_cache_are_the_replies_without_it(gpu_lib, packs, tmp_path):
    srv, th = _server(packs, str(tmp_path / "pc_on.sock"), prefix_cache=8)
    try:
        got, gained = _session(str(tmp_path / "pc_on.sock"), srv.sched)
        hits, misses = srv.sched.prefix_hits, srv.sched.prefix_misses
    finally:
        stats = _stop(srv, th)
    srv, th = _server(packs, str(tmp_path / "pc_off.sock"), prefix_cache=0)
    try:
        want, _ = _session(str(tmp_path / "pc_off.sock"))
        assert (srv.sched.prefix_hits, srv.sched.prefix_misses) == (0, 0)
    finally:
        off_stats = _stop(srv, th)
    print("hits gained per repeated case:", gained, "engine:", stats)
    assert gained[0] >= 1 and gained[1] >= 2 and gained[2] >= 1, gained
    assert (hits, misses) == (stats["hits"], stats["misses"] + stats["too_long"]) and hits + misses == 7
    assert stats["stores"] == stats["misses"] == 3 and stats["evictions"] == 0 and stats["in_use"] == 3
    assert off_stats == dict.fromkeys(off_stats, 0)                      # without the option the engine never sees a key
    assert len(got) == len(want) == 6
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w)
        for u, ((c, p), (rc, rp)) in enumerate(zip(g, w)):
            assert rc.shape[0] >= 1 and rp.shape[0] > 0, (i, u)
            np.testing.assert_array_equal(c, rc, err_msg=f"reply {i} utterance {u}: codes")
            np.testing.assert_array_equal(p, rp, err_msg=f"reply {i} utterance {u}: pcm")
    # the repeats are repeats, the two takes are two draws
    np.testing.assert_array_equal(got[1][0][0], got[0][0][0])
    np.testing.assert_array_equal(got[3][0][0], got[2][0][0])
    assert not np.array_equal(got[5][0][0], got[5][1][0])
