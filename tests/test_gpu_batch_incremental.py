"""The batch server's "vocoder": "incremental" request key: a streamed reply carries the carry-state decode's PCM from the first
check on, and per utterance its joined records are, bit for bit, the unstreamed reply with the key (synthesize_incremental) --
in the plain streamed mode and under --concurrent, greedy and seeded-sampled.  A request without the key is answered by the
chunk walk exactly as before."""
import socket
import struct
import threading

import numpy as np
import pytest

from tests.test_gpu_batch_stream import REQS, _wait, packs  # noqa: F401  (the module's server fixtures)

pytestmark = pytest.mark.gpu


def _collect(bs, sock, ids, **kw):
    recs = list(bs.synthesize_batch_stream(sock, token_ids=ids, **kw))
    pcm, ends = {u: [] for u in range(len(ids))}, {}
    for r in recs:
        if r[0] == "audio":
            assert r[1] not in ends
            pcm[r[1]].append(r[2])
        else:
            assert r[0] == "end" and r[1] not in ends
            ends[r[1]] = r[2]
    assert sorted(ends) == list(range(len(ids)))
    return recs, [(ends[u], np.concatenate(pcm[u] + [np.zeros(0, np.int16)])) for u in range(len(ids))]


def _same(got, want, what):
    assert len(got) == len(want)
    for u, ((gc, gp), (wc, wp)) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(gc, wc, err_msg=f"{what} utt {u}: codes")
        np.testing.assert_array_equal(gp, wp, err_msg=f"{what} utt {u}: pcm")


@pytest.mark.parametrize("concurrent", [False, True])
def test_streamed_and_unstreamed_incremental_replies_are_the_same_bits(gpu_lib, packs, tmp_path, concurrent):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    main, voc = packs
    sock = str(tmp_path / "incr.sock")
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=128, max_tokens=70, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, concurrent=concurrent)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    _wait(sock)
    kept, served = [], False
    try:
        modes = [("greedy", {})]
        if concurrent:       # the per-request sampling keys and seed are --concurrent's
            modes.append(("sampled", dict(temperature=0.9, top_k=20, cp_temperature=0.5, seed=1234)))
        for mode, kw in modes:
            for name, ids in REQS.items():
                what = f"{mode} {name}"
                walk = bs.synthesize_batch(sock, token_ids=ids, **kw)                         # no key: the parent's path
                _same(bs.synthesize_batch(sock, token_ids=ids, vocoder="walk", **kw), walk, what + " walk key")
                _same(_collect(bs, sock, ids, **kw)[1], walk, what + " streamed walk")
                want = bs.synthesize_batch(sock, token_ids=ids, vocoder="incremental", **kw)
                recs, got = _collect(bs, sock, ids, vocoder="incremental", **kw)
                _same(got, want, what + " incremental")
                for (wc, wp), (ic, ip) in zip(walk, want):
                    np.testing.assert_array_equal(wc, ic)                                     # same frames, another vocoder
                # first audio after the first check, not after 64 frames: every utterance of 2 or more frames has audio
                # records, and audio goes out before the request's last utterance has ended
                last_end = max(i for i, r in enumerate(recs) if r[0] == "end")
                assert any(r[0] == "audio" for r in recs[:last_end]), what
                for u, (c, p) in enumerate(want):
                    assert len(p) == srv.voc.incremental_samples(len(c)), (what, u)
                kept += [(c, wp, ip) for (c, wp), (_, ip) in zip(walk, want)]
        # any other value of the key is answered with -2; the server goes on
        for stream in (False, True):
            s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
            s.connect(sock)
            s.sendall(bs.pack_batch_request(token_ids=[[9, 8, 7]], stream=stream, vocoder="fast"))
            assert struct.unpack("<i", s.recv(4))[0] == -2
            s.close()
        assert len(bs.synthesize_batch(sock, token_ids=REQS["empty"])) == len(REQS["empty"])
        served = True
    finally:
        srv._running = False
        th.join(timeout=10)
        # the server has stopped: this thread is the vocoder's one caller now
        try:
            assert not served or any(len(c) > 64 for c, _, _ in kept)
            for c, walk_pcm, incr_pcm in (kept if served else []):
                np.testing.assert_array_equal(walk_pcm, srv.voc.synthesize_batch([c])[0])       # the chunk walk, untouched
                np.testing.assert_array_equal(incr_pcm, srv.voc.synthesize_incremental(c, int16=True))
                if len(c) > 64:
                    assert len(incr_pcm) != len(walk_pcm) or not np.array_equal(incr_pcm, walk_pcm)
        finally:
            srv.close()
    assert gpu_lib.voc_set_max_workgroups(0) == 0
