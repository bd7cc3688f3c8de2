"""The batch server's "vocoder_arithmetic": "split" request key: the incremental decode on its split-fp16 convolutions, streamed
and unstreamed the same bits; an "exact" request on the same server afterwards is today's incremental reply (the server keeps one
incremental object per arithmetic)."""
import socket
import struct
import threading

import numpy as np
import pytest

from tests.test_gpu_batch_incremental import _collect, _same
from tests.test_gpu_batch_stream import REQS, _wait, packs  # noqa: F401  (the module's server fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("concurrent", [False, True])
def test_split_requests_stream_the_bits_they_reply_and_leave_exact_alone(gpu_lib, packs, tmp_path, concurrent):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    main, voc = packs
    sock = str(tmp_path / "split.sock")
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=128, max_tokens=70, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, concurrent=concurrent)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    _wait(sock)
    kept, served = [], False
    try:
        for name, ids in REQS.items():
            before = bs.synthesize_batch(sock, token_ids=ids, vocoder="incremental")
            want = bs.synthesize_batch(sock, token_ids=ids, vocoder="incremental", vocoder_arithmetic="split")
            _, got = _collect(bs, sock, ids, vocoder="incremental", vocoder_arithmetic="split")
            _same(got, want, name + " split")
            for (ec, ep), (sc, sp) in zip(before, want):
                np.testing.assert_array_equal(ec, sc)                                 # same frames, another arithmetic
                assert len(ep) == len(sp)
                if len(ep):       # each within the waveform tolerance (2e-4 of full scale) of the model: 2 x that + 1 for the truncation
                    assert int(np.abs(ep.astype(np.int32) - sp.astype(np.int32)).max()) <= 2 * 2e-4 * 32767 + 1
            # "exact" afterwards, by the key and by default, streamed and not: the reply from before the split requests
            _same(bs.synthesize_batch(sock, token_ids=ids, vocoder="incremental", vocoder_arithmetic="exact"), before, name + " exact key")
            _same(bs.synthesize_batch(sock, token_ids=ids, vocoder="incremental"), before, name + " exact")
            _same(_collect(bs, sock, ids, vocoder="incremental")[1], before, name + " exact streamed")
            kept += [(c, ep, sp) for (c, ep), (_, sp) in zip(before, want)]
        for stream in (False, True):           # a bad value, and the key without "vocoder": "incremental": -2, the server goes on
            for kw in (dict(vocoder="incremental", vocoder_arithmetic="half"), dict(vocoder_arithmetic="split"),
                       dict(vocoder="walk", vocoder_arithmetic="split")):
                s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
                s.connect(sock)
                s.sendall(bs.pack_batch_request(token_ids=[[9, 8, 7]], stream=stream, **kw))
                assert struct.unpack("<i", s.recv(4))[0] == -2
                s.close()
        assert len(bs.synthesize_batch(sock, token_ids=REQS["empty"])) == len(REQS["empty"])
        served = True
    finally:
        srv._running = False
        th.join(timeout=10)
        try:      # the server has stopped: this thread is the vocoder's one caller now
            assert not served or any(len(c) > 64 for c, _, _ in kept)
            for c, exact_pcm, split_pcm in (kept if served else []):
                np.testing.assert_array_equal(exact_pcm, srv.voc.synthesize_incremental(c, int16=True))
                np.testing.assert_array_equal(split_pcm, srv.voc.synthesize_incremental(c, int16=True, arithmetic="split"))
            assert not served or any(len(e) and not np.array_equal(e, s) for _, e, s in kept)   # the split path really ran
        finally:
            srv.close()
    assert gpu_lib.voc_set_max_workgroups(0) == 0
