"""batch_server --concurrent --text_voice on the GPU, on the tiny packs of tests/test_gpu_concurrent.py: a text-stream
request that carries a codec prompt against a direct FrameEngine run of the same prefix, prompt and rows (codes and PCM,
with both vocoders), a bystander beside it under --text_hold, and the refusal of a server without the flag.  Array
equality throughout."""
import os
import threading
import time

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from qwen3_tts_axera_russian_amd.frontend import text_stream_rows
from tests.test_gpu_codec_prompt_server import _answer
from tests.test_gpu_concurrent import LONG, _call, _stop, packs  # noqa: F401 -- packs is a fixture
from tests.test_gpu_text_stream import _text_call

pytestmark = pytest.mark.gpu

RNG = np.random.default_rng(902)
PROMPT = RNG.integers(0, 2048, size=(33, 16)).astype(np.int32)
HEAD = [21, 22, 23]                                      # the text spoken in PROMPT, as token ids
TEXT = LONG[:18]
PIECES = [TEXT[:2], TEXT[2:9], TEXT[9:]]                 # the text in three pieces
MT = 24


def _start(packs, sock, **kw):
    main, voc = packs
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=160, max_tokens=80, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, concurrent=True, text_wait_ms=5000.0, **kw)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(400):
        if os.path.exists(sock) and srv.sched is not None:
            break
        time.sleep(0.05)
    return srv, th


@pytest.fixture(scope="module")
def servers(gpu_lib, packs, tmp_path_factory):
    """{text_hold: (server, socket)} of two --text_voice servers that know the voice "anna"."""
    d = tmp_path_factory.mktemp("tv")
    (d / "anna").mkdir()
    np.save(d / "anna" / "ref_codec_tokens.npy", PROMPT.astype(np.int64))      # as encode_reference_audio --output_dir
    out, ths = {}, []
    for hold in (False, True):
        sock = str(d / f"tv{int(hold)}.sock")
        srv, th = _start(packs, sock, text_voice=True, text_hold=hold, voices={"anna": str(d / "anna")})
        out[hold] = (srv, sock)
        ths.append((srv, th))
    yield out
    for srv, th in ths:
        _stop(srv, th)


@pytest.fixture(scope="module")
def direct(servers, packs):
    """The codes a FrameEngine of the server's shape gives the same prefix, prompt and rows, every row at admission."""
    srv = servers[False][0]
    eng = FrameEngine(packs[0], max_batch=4, n_ctx=160, max_frames=80)
    eng.set_pad_embed(srv.front.tts_pad_embed)
    eng.reserve_text(80)
    d = srv.defaults
    out = {}
    for name, head, prompt in (("voiced", HEAD, PROMPT), ("plain", [], None)):
        eng.open(4)
        S = SlotParams(max_frames=MT, temperature=d.temperature, top_k=d.top_k, top_p=d.top_p, cp_temperature=d.cp_temperature,
                       cp_top_k=d.cp_top_k, seed=d.seed, utt=0, text_stream=True, text_after_prompt=prompt is not None)
        eng.admit([0], [srv.front.build_prefix_stream(TEXT[0], head)], [0], [S], prompts=[prompt])
        eng.push_text(0, text_stream_rows(srv.front, TEXT[1:], final=True), final=True, n_text=len(head) + len(TEXT))
        while eng.run(8) > 0:
            pass
        codes, per = eng.codes()
        out[name] = np.ascontiguousarray(codes[:int(per[0]), 0, :])
    eng.destroy()
    return out


@pytest.mark.parametrize("vocoder", ["incremental", None])
@pytest.mark.parametrize("hold", [False, True])
def test_a_voiced_text_stream_gets_the_codes_and_pcm_of_a_direct_run(servers, direct, hold, vocoder):
    srv, sock = servers[hold]
    want = direct["voiced"]
    assert 1 <= len(want) <= MT
    assert not np.array_equal(want, direct["plain"])         # the prompt is not ignored
    codes, pcm = _text_call(sock, PIECES, 0.004, max_tokens=MT, vocoder=vocoder, prompt_codes=PROMPT, prompt_token_ids=HEAD)
    np.testing.assert_array_equal(codes, want)
    if vocoder == "incremental":                             # the prompt's frames warm the stream up, their samples are dropped
        drop = srv.voc.incremental_samples(len(PROMPT))
        whole = srv.voc.synthesize_incremental(np.concatenate([PROMPT, want]), int16=True)
        assert drop > 0 and len(whole) == srv.voc.incremental_samples(len(PROMPT) + len(want))
        np.testing.assert_array_equal(pcm, whole[drop:])
        alone = srv.voc.synthesize_incremental(want, int16=True)
        assert not np.array_equal(pcm[:len(alone)], alone[:len(pcm)])
    else:                                                    # the chunk walk decodes the generated frames alone
        (walk,) = srv.voc.synthesize_batch([want])
        np.testing.assert_array_equal(pcm, walk)
    # the named voice is its inline keys (this voice has no text: the head is part of the prefix, so the codes differ)
    by_voice = _text_call(sock, PIECES, 0.0, max_tokens=MT, vocoder=vocoder, voice="anna")
    inline = _text_call(sock, [TEXT], 0.0, max_tokens=MT, vocoder=vocoder, prompt_codes=PROMPT)
    np.testing.assert_array_equal(by_voice[0], inline[0])
    np.testing.assert_array_equal(by_voice[1], inline[1])
    assert not np.array_equal(by_voice[0], want)


def test_a_bystander_s_reply_does_not_depend_on_a_held_voiced_text_stream(servers):
    srv, sock = servers[True]
    ordinary = dict(token_ids=[LONG, [301, 302, 303, 304, 305, 306]], max_tokens=80, stream=True)
    alone = _call(sock, ordinary)
    held0 = srv.sched.held_steps
    got = {}

    def client():
        got["ordinary"] = _call(sock, ordinary)
    t = threading.Thread(target=client)
    t.start()
    got["text"] = _text_call(sock, [TEXT[:2], TEXT[2:3], TEXT[3:9], [], TEXT[9:]], 0.01, max_tokens=MT, voice="anna")
    t.join(timeout=120)
    assert "ordinary" in got
    print("held steps", srv.sched.held_steps - held0)
    assert srv.sched.held_steps > held0                      # it was held, beside the bystander
    whole = _text_call(sock, [TEXT], 0.0, max_tokens=MT, voice="anna")
    np.testing.assert_array_equal(got["text"][0], whole[0])
    np.testing.assert_array_equal(got["text"][1], whole[1])
    assert len(alone) == len(got["ordinary"]) == 2
    for (c, pc), (rc, rp) in zip(got["ordinary"], alone):
        np.testing.assert_array_equal(c, rc)
        np.testing.assert_array_equal(pc, rp)


def test_without_the_flag_the_request_gets_minus_two(gpu_lib, packs, tmp_path):
    sock = str(tmp_path / "tv_off.sock")
    srv, th = _start(packs, sock)
    try:
        (c, pcm), = _call(sock, dict(token_ids=[LONG[:6]], max_tokens=8))
        steps0 = srv.sched.frame_steps
        raw = bs.pack_batch_request(token_ids=[TEXT[:2]], stream=True, text_stream=True, max_tokens=MT, prompt_codes=PROMPT,
                                    prompt_token_ids=HEAD)
        assert _answer(sock, raw) == P.SENTINEL_ERROR
        assert srv.sched.frame_steps == steps0 and srv.sched.alive
        codes, _ = _text_call(sock, PIECES, 0.0, max_tokens=MT)      # ... and an unvoiced text stream is served as before
        assert 1 <= len(codes) <= MT
    finally:
        _stop(srv, th)
    with pytest.raises(ValueError):
        bs.BatchSynthesisServer(packs[0], packs[1], sock, concurrent=False, text_voice=True, install_signal_handlers=False)
