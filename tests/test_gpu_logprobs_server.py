"""batch_server --concurrent --logprobs on the GPU, tiny synthetic packs (tests/test_gpu_concurrent.py's) over a Unix socket:
a request with "logprobs" gets the codes and PCM of the same request without it, bit for bit, and the scores FrameEngine.scores()
gives for the same utterances and seed; streamed, record 3 comes once per utterance, directly before its end record; a request
without the key gets the records it always got; a server without the flag answers the key with -2 and goes on serving."""
import os
import threading
import time

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd.engine import FrameEngine
from tests.test_gpu_concurrent import LONG, SAMPLE_KEYS, _call, _stop, packs  # noqa: F401 -- (packs: the fixture)

pytestmark = pytest.mark.gpu


def _server(packs, sock, **kw):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    main, voc = packs
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=160, max_tokens=40, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, concurrent=True, **kw)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(400):
        if os.path.exists(sock) and srv.sched is not None:
            break
        time.sleep(0.05)
    return srv, th


@pytest.fixture(scope="module")
def servers(gpu_lib, packs, tmp_path_factory):
    d = tmp_path_factory.mktemp("logprobs")
    scored = _server(packs, str(d / "scored.sock"), logprobs=True)
    plain = _server(packs, str(d / "plain.sock"))
    yield str(d / "scored.sock"), str(d / "plain.sock"), scored[0]
    _stop(*scored)
    _stop(*plain)


def _records(sock, req):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    req = dict(req)
    req.pop("stream", None)
    return list(bs.synthesize_batch_stream(sock, **req))


def _call_scored(sock, req):
    """-> (list of (codes, pcm) per utterance, list of scores per utterance, the kinds of the streamed records or None)."""
    from qwen3_tts_axera_russian_amd import batch_server as bs
    if not req.get("stream"):
        out = bs.synthesize_batch(sock, **{k: v for k, v in req.items() if k != "stream"}, logprobs=True)
        return [(c, p) for c, p, _ in out], [s for _, _, s in out], None
    recs = _records(sock, dict(req, logprobs=True))
    n = len(req["token_ids"])
    pcm, codes, scores = [[] for _ in range(n)], [None] * n, [None] * n
    for kind, utt, a in recs:
        if kind == "audio":
            pcm[utt].append(a)
        elif kind == "scores":
            scores[utt] = a
        else:
            codes[utt] = a
    res = [(codes[u], np.concatenate(pcm[u]) if pcm[u] else np.zeros(0, np.int16)) for u in range(n)]
    return res, scores, [(k, u) for k, u, _ in recs]


def _same(a, b):
    assert len(a) == len(b)
    for (c, p), (rc, rp) in zip(a, b):
        assert rc.shape[0] >= 1
        np.testing.assert_array_equal(c, rc)
        np.testing.assert_array_equal(p, rp)


REQS = [dict(token_ids=[LONG[:12], [9, 8, 7]], max_tokens=24),
        dict(token_ids=[LONG[3:20], LONG[:9]], max_tokens=30, seed=6, **SAMPLE_KEYS),
        dict(token_ids=[LONG[3:20], [44, 45]], max_tokens=30, seed=6, stream=True, **SAMPLE_KEYS)]


@pytest.mark.parametrize("req", REQS, ids=["greedy", "sampled", "sampled-streamed"])
def test_logprobs_change_no_code_and_no_sample_and_are_the_engines(servers, packs, req):
    scored, plain, srv = servers
    want = _call(plain, req)
    _same(_call(scored, req), want)                       # the flag alone changes no reply
    got, scores, order = _call_scored(scored, req)
    _same(got, want)                                      # nor does the key
    for (c, _), s in zip(got, scores):
        assert s.dtype == np.float32 and s.shape == c.shape and np.isfinite(s).all() and (s < 0).all()
    if order is not None:   # record 3 once per utterance, directly before that utterance's record 2
        marks = [(k, u) for k, u in order if k != "audio"]
        assert sorted(marks) == sorted([(k, u) for u in range(len(got)) for k in ("scores", "end")])
        for i, (k, u) in enumerate(order):
            if k == "scores":
                assert order[i + 1] == ("end", u)
    # the same utterances through FrameEngine: the server's own prefix rows, parameters and seed
    utts = sorted(srv._prepare({k: v for k, v in req.items() if k != "stream"}), key=lambda u: u.utt)
    eng = FrameEngine(packs[0], max_batch=4, n_ctx=160, max_frames=40)
    try:
        eng.set_pad_embed(srv.front.tts_pad_embed)
        eng.scores_reserve()
        eng.open(4)
        slots = (2, 0)[:len(utts)]
        eng.admit(list(slots), [u.prefix for u in utts], [u.n_text for u in utts], [u.params for u in utts])
        while eng.run(8) > 0:
            pass
        codes, per = eng.codes()
        sc, _ = eng.scores()
        for u, b in zip(utts, slots):
            n = int(per[b])
            np.testing.assert_array_equal(got[u.utt][0], codes[:n, b])
            assert scores[u.utt].tobytes() == np.ascontiguousarray(sc[:n, b]).tobytes()
    finally:
        eng.destroy()


def test_a_request_without_the_key_gets_the_records_it_always_got(servers):
    scored, plain, _ = servers
    req = dict(token_ids=[LONG[:12], [9, 8, 7]], max_tokens=24)
    for sock in (scored, plain):
        kinds = [(k, u) for k, u, _ in _records(sock, req)]
        assert {k for k, _ in kinds} == {"audio", "end"}
        assert sorted(x for x in kinds if x[0] == "end") == [("end", 0), ("end", 1)]
    # "logprobs": false is such a request
    kinds = [k for k, _, _ in _records(scored, dict(req, logprobs=False))]
    assert "scores" not in kinds and kinds.count("end") == 2


def test_streamed_text_carries_its_scores(servers):
    """A "text_stream" request (token-id pieces) with the key: one record 3, directly before the end record, a score per id;
    the codes and the PCM are those of the same request without the key."""
    from qwen3_tts_axera_russian_amd import batch_server as bs
    scored, _, _ = servers
    pieces = [LONG[:3], LONG[3:7], LONG[7:9]]
    plain = list(bs.synthesize_text_stream(scored, pieces, max_tokens=20))
    recs = list(bs.synthesize_text_stream(scored, pieces, max_tokens=20, logprobs=True))
    kinds = [r[0] for r in recs]
    assert kinds.count("scores") == 1 and kinds[-2:] == ["scores", "end"] and "scores" not in [r[0] for r in plain]
    codes, sc = recs[-1][2], recs[-2][2]
    assert codes.shape[0] >= 1 and sc.shape == codes.shape and np.isfinite(sc).all() and (sc < 0).all()
    np.testing.assert_array_equal(codes, plain[-1][2])
    pcm = lambda rs: np.concatenate([r[2] for r in rs if r[0] == "audio"])
    np.testing.assert_array_equal(pcm(recs), pcm(plain))


def test_the_key_without_the_flag_fails_alone(servers):
    scored, plain, _ = servers
    req = dict(token_ids=[LONG[:12]], max_tokens=24)
    want = _call(plain, req)
    out = {}
    th = threading.Thread(target=lambda: out.setdefault("neighbour", _call(plain, req)))
    th.start()
    for sock, bad in ((plain, dict(logprobs=True)), (plain, dict(logprobs=True, stream=True)), (plain, dict(logprobs=False)),
                      (scored, dict(logprobs=1)), (scored, dict(logprobs="true", stream=True))):
        with pytest.raises(RuntimeError, match="server error"):
            _call(sock, dict(req, **bad))
    th.join(timeout=120)
    _same(out["neighbour"], want)
    _same(_call(plain, req), want)                        # both servers go on serving
    _same(_call_scored(scored, req)[0], want)


def test_the_flag_needs_concurrent(packs, tmp_path):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    with pytest.raises(ValueError, match="--concurrent"):
        bs.BatchSynthesisServer(packs[0], packs[1], str(tmp_path / "x.sock"), concurrent=False, logprobs=True,
                                install_signal_handlers=False)
