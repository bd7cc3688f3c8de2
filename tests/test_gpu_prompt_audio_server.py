"""batch_server --concurrent --encoder on the GPU, on the tiny packs of tests/test_gpu_concurrent.py and the tiny encoder table
of tests/enc_common.py: a clip sent as "prompt_audio" gives, bit for bit, the reply of the same request with "prompt_codes" =
Encoder.encode_pcm's ids -- unstreamed, streamed, with "vocoder": "incremental" and as a "text_stream" request under
--text_voice; a second send is a hit of the id cache and runs no encode; "register_voice" then "voice"; a bystander's reply
does not change while a clip is encoded; the refusals, with the server still serving.  Array equality throughout."""
import json
import os
import socket
import struct
import threading
import time

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from qwen3_tts_axera_russian_amd import weights as W
from tests import enc_common as C
from tests.test_gpu_concurrent import LONG, _call, _stop, packs  # noqa: F401 -- packs is a fixture
from tests.test_gpu_text_stream import _text_call

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mimi_encode_golden.npz")
# 0.5 s of 16 kHz stereo s16: 12000 samples at 24 kHz, 7 frames
CLIP = np.stack([C.seeded_clip(31, 8000) * 20000, C.seeded_clip(32, 8000) * 9000], 1).astype(np.int16)
CLIP2 = (C.seeded_clip(33, 22050) * 0.8).astype(np.float32)               # 1 s of 44.1 kHz mono f32: 13 frames
HEAD = [21, 22, 23]
IDS = [LONG, LONG[::-1][:20]]
TEXT = LONG[:18]
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
def enc_table(tmp_path_factory):
    gold = np.load(GOLDEN)
    keys = json.loads(bytes(gold["mimi.keys"]).decode())
    state = C.seeded_state(C.CASES["mimi"]["seed"], [(k, tuple(s)) for k, s in keys])
    _, t, _ = W.state_to_enc(state, json.loads(bytes(gold["mimi.config"]).decode()), 16)
    path = str(tmp_path_factory.mktemp("pa_enc") / "enc_mimi.q3w")
    W.write_pack(path, {"enc_sample_rate": 24000.0}, t)
    return path


@pytest.fixture(scope="module")
def server(gpu_lib, packs, enc_table, tmp_path_factory):
    d = tmp_path_factory.mktemp("pa")
    (d / "fixed").mkdir()
    np.save(d / "fixed" / "ref_codec_tokens.npy", np.zeros((3, 16), np.int64))
    sock = str(d / "pa.sock")
    srv, th = _start(packs, sock, encoder=enc_table, prompt_audio_seconds=2.0, text_voice=True, voices={"fixed": str(d / "fixed")},
                     max_voices=2)
    yield srv, sock
    _stop(srv, th)


def _answer(sock, raw):
    """the first i32 of the reply; a refusal may close the connection while the payload is still being sent"""
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.settimeout(60)
    s.connect(sock)
    try:
        try:
            s.sendall(raw)
        except (BrokenPipeError, ConnectionResetError):
            pass
        return struct.unpack("<i", P.recv_exact(s, 4))[0]
    finally:
        s.close()


def same(a, b):
    assert len(a) == len(b)
    for (c1, p1), (c2, p2) in zip(a, b):
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(p1, p2)
        assert len(c1) >= 1 and len(p1) > 0


def test_prompt_audio_is_prompt_codes_in_four_modes_and_a_second_send_is_a_hit(server):
    srv, sock = server
    with srv._encoder_lock:
        ids = srv.encoder.encode_pcm([CLIP], 16000, channels=2)[0]
    assert ids.shape == (7, 16) and len({tuple(f) for f in ids.tolist()}) > 1
    calls0 = srv.encoder.pcm_calls
    assert (srv.prompt_audio_hits, srv.prompt_audio_misses) == (0, 0)
    base = dict(token_ids=IDS, max_tokens=MT, prompt_token_ids=HEAD)
    modes = [dict(), dict(stream=True), dict(vocoder="incremental"), dict(stream=True, vocoder="incremental")]
    for k, mode in enumerate(modes):
        want = _call(sock, dict(base, prompt_codes=ids, **mode))
        got = _call(sock, dict(base, prompt_audio=(CLIP, 16000), **mode))
        same(got, want)
        # the first send encoded the clip (one library call), every later one is a hit and runs no encode
        assert (srv.prompt_audio_hits, srv.prompt_audio_misses, srv.encoder.pcm_calls - calls0) == (k, 1, 1)
    plain = _call(sock, dict(token_ids=[HEAD + i for i in IDS], max_tokens=MT))
    assert not all(np.array_equal(a[0], b[0]) for a, b in zip(plain, want))          # the prompt is not ignored
    # as a "text_stream" request under --text_voice: the payload goes out before any text record
    pieces = [TEXT[:2], TEXT[2:9], TEXT[9:]]
    for vocoder in (None, "incremental"):
        want = _text_call(sock, pieces, 0.0, max_tokens=MT, vocoder=vocoder, prompt_codes=ids, prompt_token_ids=HEAD)
        got = _text_call(sock, pieces, 0.0, max_tokens=MT, vocoder=vocoder, prompt_audio=(CLIP, 16000), prompt_token_ids=HEAD)
        same([got], [want])
    assert (srv.prompt_audio_misses, srv.encoder.pcm_calls - calls0) == (1, 1) and srv.prompt_audio_hits == len(modes) + 1
    # "max_frames" keeps the first K ids (another cache entry: one more encode)
    got = _call(sock, dict(base, prompt_audio=(CLIP, 16000), prompt_audio_max_frames=4))
    same(got, _call(sock, dict(base, prompt_codes=ids[:4])))
    assert srv.prompt_audio_misses == 2
    # per-utterance clips, of two formats and rates: two library calls
    with srv._encoder_lock:
        ids2 = srv.encoder.encode_pcm([CLIP2], 44100)[0]
    calls1 = srv.encoder.pcm_calls
    got = _call(sock, dict(token_ids=IDS, max_tokens=MT, prompt_audio=[(CLIP2, 44100), (CLIP, 16000)]))
    same(got, _call(sock, dict(token_ids=IDS, max_tokens=MT, prompt_codes=[ids2.tolist(), ids.tolist()])))
    assert srv.encoder.pcm_calls - calls1 == 1                                        # CLIP was a hit, CLIP2 a miss


def test_register_voice_then_voice(server):
    srv, sock = server
    with srv._encoder_lock:
        ids = srv.encoder.encode_pcm([CLIP], 16000, channels=2)[0]
    assert bs.synthesize_batch(sock, texts=[], prompt_audio=(CLIP, 16000), register_voice="anna", prompt_token_ids=HEAD) == []
    want = _call(sock, dict(token_ids=IDS, max_tokens=MT, prompt_codes=ids, prompt_token_ids=HEAD))
    same(_call(sock, dict(token_ids=IDS, max_tokens=MT, voice="anna")), want)
    same(_call(sock, dict(token_ids=IDS, max_tokens=MT, voice="anna", stream=True, vocoder="incremental")),
         _call(sock, dict(token_ids=IDS, max_tokens=MT, prompt_codes=ids, prompt_token_ids=HEAD, stream=True, vocoder="incremental")))
    # registering with utterances serves them too; the name is then known
    got = _call(sock, dict(token_ids=IDS, max_tokens=MT, prompt_audio=(CLIP, 16000), register_voice="bella"))
    bare = _call(sock, dict(token_ids=IDS, max_tokens=MT, prompt_codes=ids))
    same(got, bare)
    same(_call(sock, dict(token_ids=IDS, max_tokens=MT, voice="bella")), bare)
    # a start-up name is protected, the third run-time name is refused, a run-time one is replaced
    raw = lambda name, clip=CLIP: bs.pack_batch_request(texts=[], prompt_audio=(clip, 16000), register_voice=name)
    assert _answer(sock, raw("fixed")) == -2 and _answer(sock, raw("carla")) == -2
    assert _answer(sock, raw("anna", CLIP[:4000])) == 0
    with srv._encoder_lock:
        short = srv.encoder.encode_pcm([CLIP[:4000]], 16000, channels=2)[0]
    same(_call(sock, dict(token_ids=IDS, max_tokens=MT, voice="anna")), _call(sock, dict(token_ids=IDS, max_tokens=MT, prompt_codes=short)))
    with pytest.raises(RuntimeError):
        _call(sock, dict(token_ids=IDS, max_tokens=MT, voice="carla"))


def test_a_bystander_is_unchanged_while_a_clip_is_encoded(server):
    srv, sock = server
    ordinary = dict(token_ids=[LONG, [301, 302, 303, 304, 305, 306]], max_tokens=80, stream=True)
    alone = _call(sock, ordinary)
    got, errs = {}, []

    def client():
        try:
            got["ordinary"] = _call(sock, ordinary)
        except Exception as e:      # noqa: BLE001 -- reported below
            errs.append(repr(e))
    misses0, steps0 = srv.prompt_audio_misses, srv.sched.frame_steps
    t = threading.Thread(target=client)
    t.start()
    clips = [(np.roll(CLIP, k, axis=0), 16000) for k in range(1, 4)]        # three clips nobody has sent: three encodes
    for c in clips:
        got[id(c)] = _call(sock, dict(token_ids=[LONG[:9]], max_tokens=12, prompt_audio=c))
    t.join(timeout=120)
    assert not errs and "ordinary" in got
    same(got["ordinary"], alone)
    assert srv.prompt_audio_misses == misses0 + 3 and srv.sched.frame_steps > steps0


def test_refusals(server, packs, tmp_path):
    srv, sock = server
    neighbour = dict(token_ids=[LONG[:12]], max_tokens=30)
    want = _call(sock, neighbour)
    good = dict(token_ids=IDS, max_tokens=MT, prompt_audio=(CLIP, 16000))
    raw = bs.pack_batch_request(**good)
    (n,) = struct.unpack("<I", raw[:4])
    msg = json.loads(raw[4:4 + n].decode())

    def with_descriptor(**kw):
        body = json.dumps(dict(msg, prompt_audio=dict(msg["prompt_audio"], **kw))).encode()
        return struct.pack("<I", len(body)) + body + raw[4 + n:]
    hits0, misses0 = srv.prompt_audio_hits, srv.prompt_audio_misses
    assert _answer(sock, with_descriptor(format="s24")) == -2                          # bad descriptors
    assert _answer(sock, with_descriptor(rate=44101)) == -2
    assert _answer(sock, with_descriptor(channels=9)) == -2
    assert _answer(sock, with_descriptor(frames=0)) == -2
    assert _answer(sock, with_descriptor(frames=32001)) == -2                          # more than --prompt_audio_seconds 2
    assert _answer(sock, bs.pack_batch_request(**dict(good, prompt_codes=np.zeros((3, 16), np.int32)))) == -2
    assert _answer(sock, bs.pack_batch_request(**dict(good, voice="fixed"))) == -2
    assert (srv.prompt_audio_hits, srv.prompt_audio_misses) == (hits0, misses0)        # none of them got as far as the cache
    # a payload that ends early fails that request alone
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.settimeout(60)
    s.connect(sock)
    try:
        s.sendall(raw[:-1000])
        s.shutdown(socket.SHUT_WR)
        assert struct.unpack("<i", P.recv_exact(s, 4))[0] == -2
    finally:
        s.close()
    # a non-finite f32 sample: the encoder's refusal, -2
    bad = CLIP2.copy()
    bad[100] = np.nan
    assert _answer(sock, bs.pack_batch_request(token_ids=IDS, max_tokens=MT, prompt_audio=(bad, 44100))) == -2
    # ids that do not fit n_ctx: as for "prompt_codes"
    assert _answer(sock, bs.pack_batch_request(token_ids=IDS, max_tokens=80, prompt_audio=(np.zeros(48000, np.int16), 24000),
                                               prompt_token_ids=list(range(60)))) == -2
    # the server still serves, and the good request still works
    same(_call(sock, neighbour), want)
    assert len(_call(sock, good)) == 2
    # a server without --encoder answers -2
    sock2 = str(tmp_path / "noenc.sock")
    srv2, th2 = _start(packs, sock2)
    try:
        assert _answer(sock2, raw) == -2
        same(_call(sock2, neighbour), want)
    finally:
        _stop(srv2, th2)
    with pytest.raises(ValueError, match="--concurrent"):
        bs.BatchSynthesisServer(packs[0], packs[1], sock2, concurrent=False, encoder="x.q3w", install_signal_handlers=False)
