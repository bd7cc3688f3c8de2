"""batch_server --concurrent with codec prompts on the GPU, on the tiny packs of tests/test_gpu_concurrent.py: a prompted
request's codes against a direct FrameEngine run, a named voice against the inline keys, the incremental vocoder continuing
the prompt bit for bit, and the refusals.  Array equality throughout."""
import socket
import struct
import threading

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from tests.test_gpu_concurrent import LONG, _call, _stop, packs  # noqa: F401 -- packs is a fixture

pytestmark = pytest.mark.gpu

RNG = np.random.default_rng(901)
PROMPT = RNG.integers(0, 2048, size=(33, 16)).astype(np.int32)
SHORT = RNG.integers(0, 2048, size=(9, 16)).astype(np.int32)
HEAD = [21, 22, 23]                                      # the text spoken in PROMPT, as token ids
IDS = [LONG, LONG[::-1][:20]]                            # long enough that the prompt's 33 frames leave the EOS heuristics room
MT = 24


class CharTokenizer:
    """Stands where the byte-level BPE stands (no vocabulary files here): one id per character."""

    @staticmethod
    def encode(text, add_special_tokens=False):
        return [ord(c) % 500 for c in text]


TEXT = "".join(chr(t) for t in HEAD)                     # CharTokenizer.encode(TEXT) == HEAD


def _start(packs, sock, concurrent=True, voices=None):
    main, voc = packs
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=160, max_tokens=80, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, concurrent=concurrent, voices=voices)
    srv.tokenizer = CharTokenizer()
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    import os
    import time
    for _ in range(400):
        if os.path.exists(sock) and (srv.sched is not None or not concurrent):
            break
        time.sleep(0.05)
    return srv, th


@pytest.fixture(scope="module")
def server(gpu_lib, packs, tmp_path_factory):
    d = tmp_path_factory.mktemp("voices")
    (d / "anna").mkdir()
    np.save(d / "anna" / "ref_codec_tokens.npy", PROMPT.astype(np.int64))      # as encode_reference_audio --output_dir
    (d / "anna" / "ref_text.txt").write_text(TEXT)
    (d / "bare").mkdir()
    np.save(d / "bare" / "ref_codec_tokens.npy", SHORT.astype(np.int64))
    sock = str(d / "prompt.sock")
    srv, th = _start(packs, sock, voices={"anna": str(d / "anna"), "bare": str(d / "bare")})
    yield srv, sock
    _stop(srv, th)


def _direct(packs, srv, ids, prompts, max_tokens):
    """The codes a FrameEngine of the server's shape gives the same utterances, admitted together."""
    eng = FrameEngine(packs[0], max_batch=4, n_ctx=160, max_frames=80)
    eng.set_pad_embed(srv.front.tts_pad_embed)
    eng.reserve_text(80)                                 # (the frame the server captures)
    eng.open(4)
    d = srv.defaults
    params = [SlotParams(max_frames=max_tokens, temperature=d.temperature, top_k=d.top_k, top_p=d.top_p,
                         cp_temperature=d.cp_temperature, cp_top_k=d.cp_top_k, seed=d.seed, utt=u) for u in range(len(ids))]
    eng.admit(list(range(len(ids))), [srv.front.build_prefix(i) for i in ids], [len(i) for i in ids], params, prompts=prompts)
    while eng.run(8) > 0:
        pass
    codes, per = eng.codes()
    out = [np.ascontiguousarray(codes[:int(per[b]), b, :]) for b in range(len(ids))]
    eng.destroy()
    return out


def test_a_prompted_request_gets_the_codes_of_a_direct_run(server, packs):
    srv, sock = server
    full = [HEAD + i for i in IDS]
    want = _direct(packs, srv, full, [PROMPT, PROMPT], MT)
    assert all(1 <= len(w) <= MT for w in want)
    plain = _direct(packs, srv, full, None, MT)
    assert not all(np.array_equal(a, b) for a, b in zip(want, plain))       # the prompt is not ignored
    req = dict(token_ids=IDS, max_tokens=MT, prompt_codes=PROMPT, prompt_token_ids=HEAD)
    alone = _call(sock, req)
    for (c, pcm), w in zip(alone, want):
        np.testing.assert_array_equal(c, w)
        assert len(pcm) > 0
    # the chunk walk decodes the generated frames on their own
    walk = srv.voc.synthesize_batch([w for w in want])
    for (c, pcm), p in zip(alone, walk):
        np.testing.assert_array_equal(pcm, p)
    # beside other traffic, streamed and not: the same reply
    others = [dict(token_ids=[LONG], max_tokens=60), dict(token_ids=[LONG[:9], [44, 45]], max_tokens=40, stream=True),
              dict(token_ids=[LONG[:10]], max_tokens=30, prompt_codes=SHORT)]
    got, errs = {}, []

    def client(k, r):
        try:
            got[k] = _call(sock, r)
        except Exception as e:      # noqa: BLE001 -- reported below
            errs.append((k, repr(e)))
    ths = [threading.Thread(target=client, args=(k, r)) for k, r in enumerate(others + [req, dict(req, stream=True)])]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not errs, errs
    for k in (3, 4):
        for (c, pcm), (ac, apcm) in zip(got[k], alone):
            np.testing.assert_array_equal(c, ac)
            np.testing.assert_array_equal(pcm, apcm)


def test_a_voice_is_its_inline_keys(server):
    srv, sock = server
    by_voice = _call(sock, dict(token_ids=IDS, max_tokens=MT, voice="anna"))
    for inline in (dict(prompt_codes=PROMPT, prompt_token_ids=HEAD), dict(prompt_codes=PROMPT, prompt_text=TEXT)):
        for (c, pcm), (ic, ipcm) in zip(by_voice, _call(sock, dict(token_ids=IDS, max_tokens=MT, **inline))):
            np.testing.assert_array_equal(c, ic)
            np.testing.assert_array_equal(pcm, ipcm)
    bare = _call(sock, dict(token_ids=IDS[:1], max_tokens=MT, voice="bare"))
    inline = _call(sock, dict(token_ids=IDS[:1], max_tokens=MT, prompt_codes=SHORT))
    np.testing.assert_array_equal(bare[0][0], inline[0][0])
    np.testing.assert_array_equal(bare[0][1], inline[0][1])
    assert not np.array_equal(bare[0][0], by_voice[0][0])


@pytest.mark.parametrize("stream", [False, True])
def test_the_incremental_vocoder_continues_the_prompt(server, stream):
    srv, sock = server
    req = dict(token_ids=IDS, max_tokens=MT, voice="anna", vocoder="incremental", stream=stream)
    got = _call(sock, req)
    walk = _call(sock, dict(req, vocoder=None, stream=False))
    T = len(PROMPT)
    drop = srv.voc.incremental_samples(T)
    assert drop > 0
    for (c, pcm), (wc, _) in zip(got, walk):
        np.testing.assert_array_equal(c, wc)                 # the codes do not depend on the vocoder
        whole = srv.voc.synthesize_incremental(np.concatenate([PROMPT, c]), int16=True)
        assert len(whole) == srv.voc.incremental_samples(T + len(c))
        np.testing.assert_array_equal(pcm, whole[drop:])
        assert len(pcm) == srv.voc.incremental_samples(T + len(c)) - drop > 0
        alone = srv.voc.synthesize_incremental(c, int16=True)
        assert not np.array_equal(pcm[:len(alone)], alone[:len(pcm)])   # not a decode of the generated frames alone


def _answer(sock, raw):
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.settimeout(60)
    s.connect(sock)
    try:
        s.sendall(raw)
        return struct.unpack("<i", P.recv_exact(s, 4))[0]
    finally:
        s.close()


def test_refusals_are_the_request_s_own(server, packs, tmp_path):
    srv, sock = server
    neighbour = dict(token_ids=[LONG[:12]], max_tokens=40)
    want = _call(sock, neighbour)
    res, errs = [], []

    def client():
        try:
            res.append(_call(sock, neighbour))
        except Exception as e:      # noqa: BLE001 -- reported below
            errs.append(repr(e))
    th = threading.Thread(target=client)
    th.start()
    steps0 = srv.sched.frame_steps
    bad = [
        bs.pack_batch_request(token_ids=[[5, 6]], stream=True, text_stream=True, prompt_codes=SHORT),
        bs.pack_batch_request(token_ids=IDS, voice="nobody"),
        bs.pack_batch_request(token_ids=IDS, prompt_codes=[[0] * 15 + [4096]]),
        bs.pack_batch_request(token_ids=IDS, max_tokens=80, prompt_codes=np.zeros((160 - (len(LONG) + 9) - 80 + 1, 16), np.int32)),
    ]
    for raw in bad:
        assert _answer(sock, raw) == P.SENTINEL_ERROR
    th.join(timeout=120)
    assert not errs and len(res) == 1
    np.testing.assert_array_equal(res[0][0][0], want[0][0])
    np.testing.assert_array_equal(res[0][0][1], want[0][1])
    assert srv.sched.alive and srv.sched.frame_steps >= steps0


def test_a_server_that_is_not_concurrent_answers_minus_two(gpu_lib, packs, tmp_path):
    sock = str(tmp_path / "plain.sock")
    srv, th = _start(packs, sock, concurrent=False)
    try:
        assert _answer(sock, bs.pack_batch_request(token_ids=IDS[:1], max_tokens=8, prompt_codes=SHORT)) == P.SENTINEL_ERROR
        (c, pcm), = _call(sock, dict(token_ids=IDS[:1], max_tokens=8))       # ... and goes on serving
        assert 1 <= len(c) <= 8 and len(pcm) > 0
    finally:
        _stop(srv, th)
    with pytest.raises(ValueError):
        bs.BatchSynthesisServer(packs[0], packs[1], sock, concurrent=False, voices={"anna": str(tmp_path)},
                                install_signal_handlers=False)
