"""batch_server --concurrent with speaker embeddings on the GPU, on the tiny packs of tests/test_gpu_concurrent.py at 2
slots, the tiny encoder table of tests/enc_common.py and a tiny speaker encoder whose dim is the model's hidden size.

A "speaker_embedding" request's codes are those of a direct FrameEngine run on the hand-built speaker prefix; "speaker":
"only" / "with_prompt" on an s16 16 kHz payload give, bit for bit, the reply of the request with the embedding (and the
codes) inline; a repeated clip is a prompt-audio hit that runs no embed; a --voice directory with ref_spk_embedding.npy gives
both halves; under --prefix_cache two voices with the same text do not hit each other and the same voice twice does; a
text-stream request takes the same keys; the refusals are the request's own; a request without the keys gets, byte for byte,
the reply of a server started without the flags.  Array equality throughout."""
import dataclasses
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
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from tests import enc_common as C
from tests.test_gpu_concurrent import LONG, _call, _stop, packs  # noqa: F401 -- packs is a fixture
from tests.test_gpu_text_stream import _text_call

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mimi_encode_golden.npz")
# 0.5 s of 16 kHz stereo s16: 12000 samples at 24 kHz, 7 frames
CLIP = np.stack([C.seeded_clip(41, 8000) * 20000, C.seeded_clip(42, 8000) * 9000], 1).astype(np.int16)
CLIP2 = np.stack([C.seeded_clip(43, 8000) * 15000, C.seeded_clip(44, 8000) * 12000], 1).astype(np.int16)
IDS = [LONG, LONG[::-1][:20]]
HEAD = [21, 22, 23]
MT = 24
R = np.random.default_rng(91)
SPK = (0.5 * R.standard_normal(1024)).astype(np.float32)
SPK2 = (0.5 * R.standard_normal(1024)).astype(np.float32)
CODES = R.integers(0, 2048, size=(6, 16)).astype(np.int32)
PLAIN_REQUESTS = [dict(token_ids=IDS, max_tokens=MT), dict(token_ids=[LONG[:9]], max_tokens=12, stream=True),
                  dict(token_ids=IDS[:1], max_tokens=MT, prompt_codes=CODES, prompt_token_ids=HEAD, vocoder="incremental")]


def _start(packs, sock, **kw):
    main, voc = packs
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=2, n_ctx=160, max_tokens=80, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, concurrent=True, text_wait_ms=5000.0, **kw)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(400):
        if os.path.exists(sock) and srv.sched is not None:
            break
        time.sleep(0.05)
    return srv, th


def _raw_reply(sock, req):
    """every byte the server answers a request with"""
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.settimeout(120)
    s.connect(sock)
    try:
        s.sendall(bs.pack_batch_request(**req))
        out = b""
        while True:
            part = s.recv(1 << 20)
            if not part:
                return out
            out += part
    finally:
        s.close()


def _answer(sock, raw):
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


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("spk_srv")
    gold = np.load(GOLDEN)
    keys = json.loads(bytes(gold["mimi.keys"]).decode())
    state = C.seeded_state(C.CASES["mimi"]["seed"], [(k, tuple(s)) for k, s in keys])
    _, t, _ = W.state_to_enc(state, json.loads(bytes(gold["mimi.config"]).decode()), 16)
    W.write_pack(str(d / "enc.q3w"), {"enc_sample_rate": 24000.0}, t)
    W.make_synthetic_spk(str(d / "spk.q3w"), dataclasses.replace(W.tiny_spk_config(), dim=1024), seed=11)
    W.make_synthetic_spk(str(d / "spk32.q3w"), W.tiny_spk_config(), seed=11)       # dim 32: not this model's hidden size
    (d / "anna").mkdir()
    np.save(d / "anna" / "ref_codec_tokens.npy", CODES.astype(np.int64))
    np.save(d / "anna" / "ref_spk_embedding.npy", SPK)                            # as encode_reference_audio --speaker_model
    (d / "bare").mkdir()
    np.save(d / "bare" / "ref_codec_tokens.npy", CODES.astype(np.int64))
    return d


@pytest.fixture(scope="module")
def plain_replies(gpu_lib, packs, tables):
    """the replies of a server started without any of the new flags (stopped before the flagged one starts)"""
    sock = str(tables / "plain.sock")
    srv, th = _start(packs, sock)
    try:
        out = [_raw_reply(sock, r) for r in PLAIN_REQUESTS]
        # any --concurrent server takes an embedding sent inline; "speaker" needs --speaker_encoder
        inline = _call(sock, dict(token_ids=IDS, max_tokens=MT, speaker_embedding=SPK))
        assert _answer(sock, bs.pack_batch_request(token_ids=IDS, max_tokens=MT, speaker="only")) == P.SENTINEL_ERROR
    finally:
        _stop(srv, th)
    return out, inline


@pytest.fixture(scope="module")
def server(plain_replies, packs, tables):
    sock = str(tables / "spk.sock")
    srv, th = _start(packs, sock, encoder=str(tables / "enc.q3w"), speaker_encoder=str(tables / "spk.q3w"), prompt_audio_seconds=2.0,
                     text_voice=True, prefix_cache=8, voices={"anna": str(tables / "anna"), "bare": str(tables / "bare")})
    yield srv, sock
    _stop(srv, th)


def same(a, b):
    assert len(a) == len(b)
    for (c1, p1), (c2, p2) in zip(a, b):
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(p1, p2)
        assert len(c1) >= 1 and len(p1) > 0


def differ(a, b):
    return not all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))


def _direct(packs, srv, prefixes, n_text, max_tokens):
    """The codes a FrameEngine of the server's shape gives these prefixes, admitted together."""
    eng = FrameEngine(packs[0], max_batch=2, n_ctx=160, max_frames=80)
    eng.set_pad_embed(srv.front.tts_pad_embed)
    eng.reserve_text(80)                                 # (the frame the server captures)
    eng.open(2)
    d = srv.defaults
    params = [SlotParams(max_frames=max_tokens, temperature=d.temperature, top_k=d.top_k, top_p=d.top_p,
                         cp_temperature=d.cp_temperature, cp_top_k=d.cp_top_k, seed=d.seed, utt=u) for u in range(len(prefixes))]
    eng.admit(list(range(len(prefixes))), prefixes, n_text, params)
    while eng.run(8) > 0:
        pass
    codes, per = eng.codes()
    out = [np.ascontiguousarray(codes[:int(per[b]), b, :]) for b in range(len(prefixes))]
    eng.destroy()
    return out


def _embedding(srv, clip):
    with srv._encoder_lock:
        samples = srv.encoder.resample_pcm([clip], 16000, channels=2)
        return srv.speaker.embed(samples)[0], srv.encoder.encode_pcm([clip], 16000, channels=2)[0]


def test_a_speaker_embedding_request_gets_the_codes_of_a_direct_run(server, packs, plain_replies):
    srv, sock = server
    prefixes = [srv.front.build_prefix(i, speaker=SPK) for i in IDS]
    assert all(p.shape == (len(i) + 10, 1024) for p, i in zip(prefixes, IDS))
    want = _direct(packs, srv, prefixes, [len(i) for i in IDS], MT)
    plain = _direct(packs, srv, [srv.front.build_prefix(i) for i in IDS], [len(i) for i in IDS], MT)
    assert all(1 <= len(w) <= MT for w in want) and not all(np.array_equal(a, b) for a, b in zip(want, plain))   # the row is not ignored
    got = _call(sock, dict(token_ids=IDS, max_tokens=MT, speaker_embedding=SPK))
    for (c, pcm), w in zip(got, want):
        np.testing.assert_array_equal(c, w)
        assert len(pcm) > 0
    same(got, plain_replies[1])                          # ... as on the server without the flags
    same(_call(sock, dict(token_ids=IDS, max_tokens=MT, speaker_embedding=SPK, stream=True)), got)
    # one embedding per utterance
    per = _call(sock, dict(token_ids=IDS, max_tokens=MT, speaker_embedding=[SPK2, SPK]))
    np.testing.assert_array_equal(per[1][0], got[1][0])
    assert differ(per[:1], got[:1])
    # beside a codec prompt: both halves
    both = _call(sock, dict(token_ids=IDS, max_tokens=MT, speaker_embedding=SPK, prompt_codes=CODES, prompt_token_ids=HEAD))
    half = _call(sock, dict(token_ids=IDS, max_tokens=MT, prompt_codes=CODES, prompt_token_ids=HEAD))
    assert differ(both, half) and differ(both, got)


def test_only_and_with_prompt_are_the_request_with_the_embedding_inline(server):
    srv, sock = server
    emb, ids = _embedding(srv, CLIP)
    assert emb.shape == (1024,) and np.isfinite(emb).all() and ids.shape == (7, 16)
    hits0, misses0 = srv.prompt_audio_hits, srv.prompt_audio_misses
    spk_calls0, enc_calls0 = srv.speaker.calls, srv.encoder.pcm_calls
    base = dict(token_ids=IDS, max_tokens=MT)
    # "only": the clip feeds the speaker encoder alone -- no codec prompt, no encode
    only = _call(sock, dict(base, prompt_audio=(CLIP, 16000), speaker="only"))
    same(only, _call(sock, dict(base, speaker_embedding=emb)))
    assert (srv.speaker.calls - spk_calls0, srv.encoder.pcm_calls - enc_calls0) == (1, 0)
    assert (srv.prompt_audio_hits - hits0, srv.prompt_audio_misses - misses0) == (0, 1)
    # a repeated clip is a hit that runs no embed
    same(_call(sock, dict(base, prompt_audio=(CLIP, 16000), speaker="only", stream=True)), only)
    assert (srv.speaker.calls - spk_calls0, srv.prompt_audio_hits - hits0, srv.prompt_audio_misses - misses0) == (1, 1, 1)
    # "with_prompt": the embedding beside the clip's codec prompt (the ids are missing: one encode, no second embed)
    for k, mode in enumerate((dict(), dict(stream=True, vocoder="incremental"))):
        got = _call(sock, dict(base, prompt_audio=(CLIP, 16000), speaker="with_prompt", prompt_token_ids=HEAD, **mode))
        same(got, _call(sock, dict(base, speaker_embedding=emb, prompt_codes=ids, prompt_token_ids=HEAD, **mode)))
        assert (srv.speaker.calls - spk_calls0, srv.encoder.pcm_calls - enc_calls0) == (1, 1)
        assert (srv.prompt_audio_hits - hits0, srv.prompt_audio_misses - misses0) == (1 + k, 2)
    assert differ(got, only)
    # "off" (and no key) is today's request: the codec prompt alone
    off = _call(sock, dict(base, prompt_audio=(CLIP, 16000), speaker="off", prompt_token_ids=HEAD))
    same(off, _call(sock, dict(base, prompt_codes=ids, prompt_token_ids=HEAD)))
    same(off, _call(sock, dict(base, prompt_audio=(CLIP, 16000), prompt_token_ids=HEAD)))
    assert srv.speaker.calls - spk_calls0 == 1
    # per-utterance clips: CLIP is a hit, CLIP2 is embedded
    emb2, _ = _embedding(srv, CLIP2)
    calls1 = srv.speaker.calls
    got = _call(sock, dict(base, prompt_audio=[(CLIP2, 16000), (CLIP, 16000)], speaker="only"))
    same(got, _call(sock, dict(base, speaker_embedding=[emb2, emb])))
    assert srv.speaker.calls - calls1 == 1
    # "register_voice" keeps the embedding with the voice
    assert bs.synthesize_batch(sock, texts=[], prompt_audio=(CLIP, 16000), register_voice="carla", speaker="with_prompt",
                               prompt_token_ids=HEAD) == []
    carla = _call(sock, dict(base, voice="carla"))
    same(carla, _call(sock, dict(base, speaker_embedding=emb, prompt_codes=ids, prompt_token_ids=HEAD)))
    same(_call(sock, dict(base, voice="carla", speaker="off")), _call(sock, dict(base, prompt_codes=ids, prompt_token_ids=HEAD)))


def test_a_voice_directory_with_an_embedding_gives_both_halves(server):
    srv, sock = server
    base = dict(token_ids=IDS, max_tokens=MT)
    anna = _call(sock, dict(base, voice="anna"))
    same(anna, _call(sock, dict(base, prompt_codes=CODES, speaker_embedding=SPK)))
    bare = _call(sock, dict(base, voice="bare"))
    same(bare, _call(sock, dict(base, prompt_codes=CODES)))
    same(_call(sock, dict(base, voice="anna", speaker="off")), bare)
    assert differ(anna, bare)


def test_two_voices_do_not_share_a_prefix_cache_entry(server):
    srv, sock = server
    text = [[301, 302, 303, 304, 305, 306, 307]]
    r = np.random.default_rng(5)
    a, b = (0.5 * r.standard_normal(1024)).astype(np.float32), (0.5 * r.standard_normal(1024)).astype(np.float32)

    def call(**kw):
        h, m = srv.sched.prefix_hits, srv.sched.prefix_misses
        out = _call(sock, dict(token_ids=text, max_tokens=MT, **kw))
        return out, (srv.sched.prefix_hits - h, srv.sched.prefix_misses - m)
    va, d = call(speaker_embedding=a)
    assert d == (0, 1)
    vb, d = call(speaker_embedding=b)
    assert d == (0, 1) and differ(va, vb)                # the other voice, the same text: no hit
    none, d = call()
    assert d == (0, 1) and differ(none, va)              # nor does the unspeakered text hit a voice
    again, d = call(speaker_embedding=a)
    assert d == (1, 0)                                   # the same voice twice does
    same(again, va)
    again, d = call(speaker_embedding=b, stream=True)
    assert d == (1, 0)
    same(again, vb)


def test_a_text_stream_request_takes_the_same_keys(server):
    srv, sock = server
    text = LONG[:18]
    pieces = [text[:2], text[2:9], text[9:]]
    emb, ids = _embedding(srv, CLIP)
    plain = _text_call(sock, pieces, 0.0, max_tokens=MT)
    got = _text_call(sock, pieces, 0.0, max_tokens=MT, speaker_embedding=emb)
    same([got], [_text_call(sock, [text[:5], text[5:]], 0.0, max_tokens=MT, speaker_embedding=emb)])     # whatever the cut
    assert differ([got], [plain])
    same([_text_call(sock, pieces, 0.0, max_tokens=MT, prompt_audio=(CLIP, 16000), speaker="only")], [got])
    both = _text_call(sock, pieces, 0.0, max_tokens=MT, prompt_audio=(CLIP, 16000), speaker="with_prompt", prompt_token_ids=HEAD)
    same([both], [_text_call(sock, pieces, 0.0, max_tokens=MT, speaker_embedding=emb, prompt_codes=ids, prompt_token_ids=HEAD)])


def test_refusals_are_the_request_s_own(server, packs, tables):
    srv, sock = server
    neighbour = dict(token_ids=[LONG[:12]], max_tokens=30)
    want = _call(sock, neighbour)
    base = dict(token_ids=IDS, max_tokens=MT)
    bad = SPK.copy()
    bad[5] = np.nan
    for req in (dict(base, speaker_embedding=SPK[:-1]), dict(base, speaker_embedding=np.zeros(32, np.float32)),
                dict(base, speaker_embedding=[SPK, SPK, SPK]), dict(base, speaker_embedding=bad),
                dict(base, speaker="only"), dict(base, speaker="with_prompt", prompt_codes=CODES),
                dict(base, speaker="loud"), dict(base, speaker="only", prompt_codes=CODES, prompt_audio=(CLIP, 16000)),
                dict(base, speaker="only", speaker_embedding=SPK, prompt_audio=(CLIP, 16000)),
                dict(base, speaker="only", prompt_audio=(CLIP[:50], 16000)),             # 75 samples at 24 kHz: below the shortest clip
                dict(base, speaker="only", prompt_audio=(CLIP, 16000), prompt_token_ids=HEAD),   # a prompt text without a codec prompt
                dict(texts=[], speaker="only", prompt_audio=(CLIP, 16000), register_voice="dora")):
        assert _answer(sock, bs.pack_batch_request(**req)) == P.SENTINEL_ERROR, sorted(req)
    assert srv.speaker.min_samples == 80
    same(_call(sock, neighbour), want)                   # the server still serves
    # start-up: the flag needs --encoder and --concurrent, and the model's hidden size
    main, voc = packs
    kw = dict(install_signal_handlers=False)
    with pytest.raises(ValueError, match="--encoder"):
        bs.BatchSynthesisServer(main, voc, str(tables / "x.sock"), concurrent=True, speaker_encoder=str(tables / "spk.q3w"), **kw)
    with pytest.raises(ValueError):
        bs.BatchSynthesisServer(main, voc, str(tables / "x.sock"), concurrent=False, encoder=str(tables / "enc.q3w"),
                                speaker_encoder=str(tables / "spk.q3w"), **kw)
    with pytest.raises(ValueError, match="hidden|1024"):
        bs.BatchSynthesisServer(main, voc, str(tables / "x.sock"), max_batch=2, n_ctx=160, max_tokens=80, concurrent=True,
                                encoder=str(tables / "enc.q3w"), speaker_encoder=str(tables / "spk32.q3w"), **kw)


def test_a_request_without_the_keys_gets_the_reply_of_a_server_without_the_flags(server, plain_replies):
    srv, sock = server
    for req, want in zip(PLAIN_REQUESTS, plain_replies[0]):
        got = _raw_reply(sock, req)
        assert len(want) > 16 and got == want, sorted(req)


def test_a_server_that_is_not_concurrent_answers_minus_two(gpu_lib, packs, tmp_path):
    main, voc = packs
    sock = str(tmp_path / "plain.sock")
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=2, n_ctx=160, max_tokens=80, temperature=0.0, cp_temperature=0.0,
                                  install_signal_handlers=False, concurrent=False)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(400):
        if os.path.exists(sock):
            break
        time.sleep(0.05)
    try:
        assert _answer(sock, bs.pack_batch_request(token_ids=IDS[:1], max_tokens=8, speaker_embedding=SPK)) == P.SENTINEL_ERROR
        assert _answer(sock, bs.pack_batch_request(token_ids=IDS[:1], max_tokens=8, speaker="off")) == P.SENTINEL_ERROR
        (c, pcm), = _call(sock, dict(token_ids=IDS[:1], max_tokens=8))       # ... and goes on serving
        assert 1 <= len(c) <= 8 and len(pcm) > 0
    finally:
        _stop(srv, th)
