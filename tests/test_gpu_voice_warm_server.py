"""batch_server --concurrent --voice_warm on the GPU, on the tiny packs of tests/test_gpu_concurrent.py: two servers, one with
voice_warm=2 and one without.  With the flag every reply -- codes and PCM, streamed and not, both arithmetics -- is bit for bit
the reply without it, and the counters say which requests decoded their prompt (a miss) and which copied its snapshot (a hit).
Array equality throughout.  Every test uses prompts of its own, so none depends on what another left in the cache."""
import os
import threading
import time

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from tests.test_gpu_codec_prompt_server import CharTokenizer
from tests.test_gpu_concurrent import LONG, _call, _stop, packs  # noqa: F401 -- packs is a fixture
from tests.test_gpu_text_stream import _text_call

pytestmark = pytest.mark.gpu

RNG = np.random.default_rng(903)
PROMPT = RNG.integers(0, 2048, size=(33, 16)).astype(np.int32)      # the voice "anna"
SHORT = RNG.integers(0, 2048, size=(9, 16)).astype(np.int32)        # the voice "bare"
TV = RNG.integers(0, 2048, size=(70, 16)).astype(np.int32)          # the voice "tess" (beyond chunk_tokens: two warm-up pushes)
FRESH = [RNG.integers(0, 2048, size=(n, 16)).astype(np.int32) for n in (12, 40, 65, 21)]
IDS = [LONG, LONG[::-1][:20]]
MT = 24
TEXT = "".join(chr(t) for t in (21, 22, 23))                        # the text spoken in PROMPT


class Tokenizer(CharTokenizer):
    """CharTokenizer for the voice's text; the text streams of this file send token ids, so nothing is tokenised piecewise."""

    @staticmethod
    def incremental():
        raise AssertionError("the text stream sends token ids")


def _start(packs, sock, voices, **kw):
    main, voc = packs
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=160, max_tokens=80, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, concurrent=True, text_wait_ms=5000.0, voices=voices,
                                  text_voice=True, **kw)
    srv.tokenizer = Tokenizer()
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(400):
        if os.path.exists(sock) and srv.sched is not None:
            break
        time.sleep(0.05)
    return srv, th


@pytest.fixture(scope="module")
def servers(gpu_lib, packs, tmp_path_factory):
    """(server with voice_warm=2, its socket, socket of the server without the flag)"""
    d = tmp_path_factory.mktemp("vw")
    voices = {}
    for name, codes in (("anna", PROMPT), ("bare", SHORT), ("tess", TV)):
        (d / name).mkdir()
        np.save(d / name / "ref_codec_tokens.npy", codes.astype(np.int64))      # as encode_reference_audio --output_dir
        voices[name] = str(d / name)
    (d / "anna" / "ref_text.txt").write_text(TEXT)
    warm, th_w = _start(packs, str(d / "warm.sock"), voices, voice_warm=2)
    plain, th_p = _start(packs, str(d / "plain.sock"), voices)
    yield warm, str(d / "warm.sock"), str(d / "plain.sock")
    _stop(warm, th_w)
    _stop(plain, th_p)


def counters(srv):
    return np.array([srv.voice_warm_hits, srv.voice_warm_misses, srv.voice_warm_evictions])


def same(got, want):
    assert len(got) == len(want)
    for (c, pcm), (wc, wpcm) in zip(got, want):
        np.testing.assert_array_equal(c, wc)
        np.testing.assert_array_equal(pcm, wpcm)
        assert len(pcm) > 0


@pytest.mark.parametrize("arithmetic", ["exact", "split"])
def test_bits_with_and_without_the_flag(servers, arithmetic):
    srv, warm, plain = servers
    req = dict(token_ids=IDS, max_tokens=MT, voice="anna", vocoder="incremental", vocoder_arithmetic=arithmetic)
    want = _call(plain, req)
    c0 = counters(srv)
    same(_call(warm, req), want)                   # the key (anna, this arithmetic) is new: the first utterance decodes the prompt
    assert list(counters(srv) - c0)[:2] == [1, 1]
    same(_call(warm, req), want)                   # a second identical request: hits only, the same bits again
    assert list(counters(srv) - c0)[:2] == [3, 1]
    want_s = _call(plain, dict(req, stream=True))
    same(want_s, want)                             # (streamed and unstreamed replies carry the same bits)
    same(_call(warm, dict(req, stream=True)), want_s)
    assert list(counters(srv) - c0)[:2] == [5, 1]


def test_inline_codes_share_the_voice(servers):
    srv, warm, plain = servers
    by_voice = dict(token_ids=IDS[:1], max_tokens=MT, voice="bare", vocoder="incremental", stream=True)
    inline = dict(token_ids=IDS[:1], max_tokens=MT, prompt_codes=SHORT, vocoder="incremental")
    c0 = counters(srv)
    same(_call(warm, by_voice), _call(plain, by_voice))
    assert list(counters(srv) - c0)[:2] == [0, 1]
    same(_call(warm, inline), _call(plain, inline))
    same(_call(warm, dict(inline, stream=True)), _call(plain, dict(inline, stream=True)))
    assert list(counters(srv) - c0)[:2] == [2, 1]


def test_eviction_of_the_least_recently_used(servers):
    srv, warm, plain = servers
    req = [dict(token_ids=IDS[:1], max_tokens=MT, prompt_codes=p, vocoder="incremental", stream=True) for p in FRESH[:3]]
    want = [_call(plain, r) for r in req]
    c0 = counters(srv)
    for k, hits, misses in ((0, 0, 1), (1, 0, 2), (2, 0, 3), (1, 1, 3), (0, 1, 4), (1, 2, 4)):
        same(_call(warm, req[k]), want[k])         # two slots: the third prompt evicts the first, the second stays; the first
        assert list(counters(srv) - c0)[:2] == [hits, misses], k       # comes back as a miss (evicting the third), same bits
    assert (counters(srv) - c0)[2] >= 2            # (the third and the returning first found both slots taken)
    assert srv.voc.snapshot_frames(0) in (len(FRESH[0]), len(FRESH[1])) and srv.voc.snapshot_frames(1) in (len(FRESH[0]), len(FRESH[1]))


def test_requests_without_a_prompt_or_on_the_walk_touch_nothing(servers):
    srv, warm, plain = servers
    c0 = counters(srv)
    for req in (dict(token_ids=IDS, max_tokens=MT, vocoder="incremental"), dict(token_ids=IDS, max_tokens=MT, vocoder="incremental", stream=True),
                dict(token_ids=IDS, max_tokens=MT, voice="anna"), dict(token_ids=IDS, max_tokens=MT, voice="anna", stream=True)):
        same(_call(warm, req), _call(plain, req))
    assert list(counters(srv) - c0) == [0, 0, 0]


def test_two_utterances_admitted_together_with_a_new_voice(servers):
    srv, warm, plain = servers
    req = dict(token_ids=IDS, max_tokens=MT, prompt_codes=FRESH[3], vocoder="incremental", stream=True)
    want = _call(plain, req)
    c0 = counters(srv)
    same(_call(warm, req), want)
    assert list(counters(srv) - c0)[:2] == [1, 1]  # one decoded the prompt, the other copied what it left


def test_a_voiced_text_stream_goes_the_same_way(servers):
    srv, warm, plain = servers
    text = LONG[:18]
    pieces = [text[:2], text[2:9], text[9:]]
    kw = dict(max_tokens=MT, vocoder="incremental", voice="tess")
    want = _text_call(plain, pieces, 0.004, **kw)
    c0 = counters(srv)
    for hits in (0, 1):
        codes, pcm = _text_call(warm, pieces, 0.004, **kw)
        np.testing.assert_array_equal(codes, want[0])
        np.testing.assert_array_equal(pcm, want[1])
        assert len(pcm) > 0 and list(counters(srv) - c0)[:2] == [hits, 1]


def test_the_flag_needs_concurrent(packs, tmp_path):
    with pytest.raises(ValueError):
        bs.BatchSynthesisServer(packs[0], packs[1], str(tmp_path / "x.sock"), concurrent=False, voice_warm=2,
                                install_signal_handlers=False)
    with pytest.raises(ValueError):
        bs.BatchSynthesisServer(packs[0], packs[1], str(tmp_path / "x.sock"), concurrent=True, voice_warm=-1,
                                install_signal_handlers=False)
