"""batch_server --concurrent --sampler_rules on the GPU, tiny synthetic packs (tests/test_gpu_concurrent.py's): default rules
spelled out give the reply of a request without them and of a server without the flag, bit for bit (codes and PCM); the
"upstream" preset gives the codes FrameEngine.admit gives under the same rules and seed, whatever runs beside it; the keys
without the flag, and a bad value, are answered -2 for that request alone."""
import os
import threading
import time

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotRules
from tests.test_gpu_concurrent import LONG, SAMPLE_KEYS, _call, _stop, packs  # noqa: F401 -- (packs: the fixture)

pytestmark = pytest.mark.gpu

DEFAULT_KEYS = dict(repetition_penalty=1.2, repetition_window=30, eos_boost=15.0, eos_force=2.0, min_tokens=0, cp_top_p=1.0)
UPSTREAM = SlotRules(rep_penalty=1.05, rep_window=0, eos_boost=0.0, eos_force=0.0, min_frames=2)


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
    d = tmp_path_factory.mktemp("rules")
    ruled = _server(packs, str(d / "ruled.sock"), sampler_rules=True)
    plain = _server(packs, str(d / "plain.sock"))
    yield str(d / "ruled.sock"), str(d / "plain.sock"), ruled[0]
    _stop(*ruled)
    _stop(*plain)


def _same(a, b):
    assert len(a) == len(b)
    for (c, p), (rc, rp) in zip(a, b):
        assert rc.shape[0] >= 1
        np.testing.assert_array_equal(c, rc)
        np.testing.assert_array_equal(p, rp)


@pytest.mark.parametrize("req", [dict(token_ids=[LONG[:12], [9, 8, 7]], max_tokens=24),
                                 dict(token_ids=[LONG[3:20]], max_tokens=30, seed=6, stream=True, **SAMPLE_KEYS)],
                         ids=["greedy", "sampled-streamed"])
def test_default_rules_spelled_out_change_no_reply(servers, req):
    ruled, plain, _ = servers
    want = _call(plain, req)
    _same(_call(ruled, req), want)
    _same(_call(ruled, dict(req, **DEFAULT_KEYS)), want)
    _same(_call(ruled, dict(req, sampler="reference")), want)


def test_upstream_preset_is_admit_with_those_rules(servers, packs):
    ruled, _, srv = servers
    req = dict(token_ids=[LONG[:10], LONG[5:17]], max_tokens=20, seed=11, **SAMPLE_KEYS)
    beside = dict(token_ids=[LONG], max_tokens=40, seed=3, repetition_penalty=2.0, cp_top_p=0.5, **SAMPLE_KEYS)
    out = {}
    th = threading.Thread(target=lambda: out.setdefault("beside", _call(ruled, beside)))
    th.start()
    got = _call(ruled, dict(req, sampler="upstream"))
    th.join(timeout=120)
    assert "beside" in out and out["beside"][0][0].shape[0] >= 1
    # the same utterances through FrameEngine.admit: the server's own prefix rows and parameters, the rules written out here
    utts = sorted(srv._prepare(dict(req)), key=lambda u: u.utt)
    assert all(u.rules is None for u in utts)
    eng = FrameEngine(packs[0], max_batch=4, n_ctx=160, max_frames=40)
    try:
        eng.set_pad_embed(srv.front.tts_pad_embed)
        eng.rules()
        eng.open(4)
        eng.admit([2, 0], [u.prefix for u in utts], [u.n_text for u in utts], [u.params for u in utts], rules=[UPSTREAM] * 2)
        while eng.run(8) > 0:
            pass
        codes, per = eng.codes()
        for u, b in zip(utts, (2, 0)):
            np.testing.assert_array_equal(got[u.utt][0], codes[:int(per[b]), b])
            assert got[u.utt][0].shape[0] >= 2                # min_tokens
    finally:
        eng.destroy()
    assert not all(np.array_equal(a[0], b[0]) for a, b in zip(got, _call(ruled, req)))    # and they are not the default's


def test_keys_without_the_flag_and_bad_values_fail_alone(servers):
    ruled, plain, _ = servers
    req = dict(token_ids=[LONG[:12]], max_tokens=24)
    want = _call(plain, req)
    out = {}
    th = threading.Thread(target=lambda: out.setdefault("neighbour", _call(ruled, req)))
    th.start()
    for sock, bad in ((plain, dict(sampler="reference")), (plain, dict(cp_top_p=1.0)), (plain, dict(min_tokens=2, stream=True)),
                      (ruled, dict(repetition_penalty=0.5)), (ruled, dict(sampler="hf")), (ruled, dict(repetition_window=31, stream=True)),
                      (ruled, dict(cp_top_p="1"))):
        with pytest.raises(RuntimeError, match="server error"):
            _call(sock, dict(req, **bad))
    th.join(timeout=120)
    _same(out["neighbour"], want)
    _same(_call(plain, req), want)                            # both servers go on serving
