"""Streamed batch-server replies ({"stream": true}): records of PCM and utterance ends while the frame loop runs.  Per utterance the
joined PCM records and the codes of its end record are the unstreamed reply's, bit for bit."""
import os
import socket
import struct
import threading
import time

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import weights as W
from tests.util import CACHE

pytestmark = pytest.mark.gpu

REQS = {
    "within": [[5, 17, 200, 33, 41, 7, 90, 120, 64, 3, 11, 250, 77, 8, 19, 300, 45, 60, 2, 150, 99, 21, 13, 55, 180],
               [9, 8, 7], [301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311, 312]],
    "refills": [[5, 17, 200, 33, 41, 7, 90, 120, 64, 3, 11, 250, 77, 8, 19, 300, 45, 60, 2, 150, 99, 21, 13, 55, 180],
                [9, 8, 7], [301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311, 312], [9, 8, 7, 6, 5], [4, 4, 4, 4],
                [301, 302, 303]],
    "empty": [[9, 8, 7, 6, 5], [], [5, 17, 200, 33, 41, 7, 90]],
}


@pytest.fixture(scope="module")
def packs():
    os.makedirs(CACHE, exist_ok=True)
    cfg = W.tiny_config(2, 2, text_vocab=512)
    cfg.text_dim = 64
    main = os.path.join(CACHE, "srv_tiny_t2c2.q3w")
    if not os.path.exists(main):
        W.write_synthetic(main, cfg, seed=1234, parts=("talker", "cp", "text"))
    voc = os.path.join(CACHE, "srv_voc_tiny.q3w")
    if not os.path.exists(voc):
        W.write_pack(voc, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    return main, voc


def _wait(path):
    for _ in range(200):
        if os.path.exists(path):
            return
        time.sleep(0.05)
    raise RuntimeError(f"{path} did not appear")


def _collect(bs, sock, ids):
    recs = list(bs.synthesize_batch_stream(sock, token_ids=ids))
    pcm = {u: [] for u in range(len(ids))}
    ends = {}
    for r in recs:
        if r[0] == "audio":
            assert r[1] not in ends                   # no audio of an utterance after its end record
            pcm[r[1]].append(r[2])
        else:
            assert r[0] == "end" and r[1] not in ends
            ends[r[1]] = r[2]
    assert sorted(ends) == list(range(len(ids)))
    return recs, [(ends[u], np.concatenate(pcm[u] + [np.zeros(0, np.int16)])) for u in range(len(ids))]


@pytest.mark.parametrize("pipeline", [False, True])
def test_streamed_replies_are_the_unstreamed_ones(gpu_lib, packs, tmp_path, pipeline):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    main, voc = packs
    sock = str(tmp_path / "stream.sock")
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=128, max_tokens=70, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, pipeline=pipeline)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    _wait(sock)
    try:
        for name, ids in REQS.items():
            want = bs.synthesize_batch(sock, token_ids=ids)
            recs, got = _collect(bs, sock, ids)
            assert len(got) == len(want) == len(ids)
            for u, ((gc, gp), (wc, wp)) in enumerate(zip(got, want)):
                np.testing.assert_array_equal(gc, wc, err_msg=f"{name} utt {u}")
                np.testing.assert_array_equal(gp, wp, err_msg=f"{name} utt {u}")
            # audio goes out before the request has ended (an utterance of 64 or more frames hands out its first chunk)
            last_end = max(i for i, r in enumerate(recs) if r[0] == "end")
            assert any(r[0] == "audio" for r in recs[:last_end]), name
        assert max(len(c) for c, _ in got) >= 1
        # an invalid request gets the error sentinel; the server goes on
        s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        s.connect(sock)
        s.sendall(bs.pack_batch_request(token_ids=[], stream=True))
        assert struct.unpack("<i", s.recv(4))[0] == -2
        s.close()
        with pytest.raises(RuntimeError):
            list(bs.synthesize_batch_stream(sock, token_ids=[]))
        _, again = _collect(bs, sock, REQS["empty"])
        want = bs.synthesize_batch(sock, token_ids=REQS["empty"])
        for (gc, gp), (wc, wp) in zip(again, want):
            np.testing.assert_array_equal(gc, wc)
            np.testing.assert_array_equal(gp, wp)
    finally:
        srv._running = False
        th.join(timeout=10)
        srv.close()
    assert gpu_lib.voc_set_max_workgroups(0) == 0
