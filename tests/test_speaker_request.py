"""batch_server --concurrent with speaker embeddings, without a GPU: the request keys ("speaker_embedding", "speaker"), what
_prepare queues and refuses, the prefix key, the voice table and the prompt-audio LRU that keep an embedding beside the ids,
the client's packing.  Over the small host front end of tests/test_text_stream_scheduler.py.  CPU only."""
import hashlib
import json
import socket
import struct

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_request as R
from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from tests.test_concurrent_scheduler import CAP
from tests.test_text_stream_scheduler import TextFakeEngine, _bare_server, make

RNG = np.random.default_rng(77)
H = 16                                                   # the bare server's hidden size
SPK = RNG.standard_normal(H).astype(np.float32)
SPK2 = RNG.standard_normal(H).astype(np.float32)
PROMPT = RNG.integers(0, 2048, size=(5, 16)).astype(np.int32)
IDS = [[5, 6, 7], [9], [5, 6, 7]]


def _msg(**req):
    raw = bs.pack_batch_request(**req)
    (n,) = struct.unpack("<I", raw[:4])
    return json.loads(raw[4:4 + n].decode())


def _server(text_voice=False):
    srv = _bare_server()
    srv.voices = {}
    srv.text_voice = text_voice
    srv.runtime_voices = R.VoiceTable({}, 4)
    return srv


def test_the_embedding_travels_exactly_and_is_parsed():
    m = _msg(token_ids=IDS, speaker_embedding=SPK)
    assert isinstance(m["speaker_embedding"], list) and len(m["speaker_embedding"]) == H
    (a, b, c) = R.request_speaker_embedding(m["speaker_embedding"], 3, H)
    assert a is b is c and a.dtype == np.float32 and np.array_equal(a.view(np.uint32), SPK.view(np.uint32))
    per = R.request_speaker_embedding(_msg(token_ids=IDS[:2], speaker_embedding=[SPK, SPK2])["speaker_embedding"], 2, H)
    assert np.array_equal(per[0], SPK) and np.array_equal(per[1], SPK2)
    assert "speaker_embedding" not in _msg(token_ids=IDS) and "speaker" not in _msg(token_ids=IDS)
    assert _msg(token_ids=IDS, speaker="only")["speaker"] == "only"
    for bad, n in (([0.0] * (H - 1), 1), ([0.0] * (H + 1), 1), ([], 1), ("abc", 1), (None, 1), ([[0.0] * H], 2),
                   ([[0.0] * H, [0.0] * (H - 1)], 2), ([0.0] * (H - 1) + [float("nan")], 1), ([0.0] * (H - 1) + [float("inf")], 1),
                   ([0.0] * (H - 1) + [1e39], 1), ([0.0] * (H - 1) + [True], 1), ([0.0] * (H - 1) + ["1"], 1),
                   ([0.0] * (H - 1) + [10 ** 400], 1), ({"a": 1}, 1)):
        with pytest.raises(ValueError):
            R.request_speaker_embedding(bad, n, H)
    for mode in ("off", "only", "with_prompt", None):
        assert R.request_speaker_mode({"speaker": mode}) == (mode or "off")
    for bad in ("on", 1, True, ["only"]):
        with pytest.raises(ValueError):
            R.request_speaker_mode({"speaker": bad})
    assert R.request_has_speaker({"speaker": "off"}) and R.request_has_speaker({"speaker_embedding": [1]}) and not R.request_has_speaker({})


def test_the_prefix_key_digests_the_embedding_and_the_kind():
    ids = [5, 6, 7]
    plain = bs.prefix_key(b"full", ids)
    assert plain == hashlib.sha256(b"full\0" + np.asarray(ids, "<i4").tobytes()).digest()[:16]     # what it always was
    assert bs.prefix_key(b"full", ids, speaker=None) == plain
    k = bs.prefix_key(b"full", ids, speaker=SPK)
    assert len(k) == 16 and k != plain and k == bs.prefix_key(b"full", ids, speaker=SPK.astype(np.float64))
    seen = {k}                                           # the speakered keys
    for i in range(H):                                   # only the embedding differs, by one ulp of one value
        q = SPK.copy()
        q[i] = np.nextafter(q[i], np.float32(np.inf))
        kk = bs.prefix_key(b"full", ids, speaker=q)
        assert kk not in seen
        seen.add(kk)
    # the kind of prefix: a speakered key is no unspeakered key of any kind, with the embedding's bytes taken for ids or not
    as_ids = ids + [int(x) for x in SPK.view(np.int32)]
    assert plain not in seen
    for kind in (b"full", b"stream", b"full+spk"):
        assert bs.prefix_key(kind, ids) not in seen and bs.prefix_key(kind, as_ids) not in seen
    kp, kps = bs.prefix_key(b"prompt", ids, PROMPT), bs.prefix_key(b"prompt", ids, PROMPT, SPK)
    assert kps not in seen | {kp, plain} and kps != bs.prefix_key(b"prompt", ids, PROMPT, SPK2)
    assert bs.prefix_key(b"stream", ids[:1], None, SPK) not in seen | {kp, kps, plain, bs.prefix_key(b"stream", ids[:1])}


def test_prepare_builds_the_speaker_prefix():
    srv = _server()
    items = srv._prepare(_msg(token_ids=IDS, seed=3, speaker_embedding=SPK))
    for it in items:
        want = srv.front.build_prefix(IDS[it.utt], speaker=SPK)
        assert it.prefix.shape == (len(IDS[it.utt]) + 10, H) and np.array_equal(it.prefix, want)
        assert np.array_equal(it.prefix[6], srv.front.tts_pad_embed + SPK)
        assert it.prompt is None and it.n_text == len(IDS[it.utt]) and it.params.max_frames == CAP
        assert it.prefix_key == bs.prefix_key(b"full", IDS[it.utt], speaker=SPK)
    by = {it.utt: it for it in items}
    assert by[0].prefix_key == by[2].prefix_key != by[1].prefix_key
    # one per utterance; beside a codec prompt: both halves, and the prompted key digests the embedding too
    items = srv._prepare(_msg(token_ids=IDS[:2], speaker_embedding=[SPK, SPK2], prompt_codes=PROMPT, prompt_token_ids=[11, 12]))
    for it, spk in zip(sorted(items, key=lambda i: i.utt), (SPK, SPK2)):
        full = [11, 12] + IDS[it.utt]
        assert np.array_equal(it.prefix, srv.front.build_prefix(full, speaker=spk)) and np.array_equal(it.prompt, PROMPT)
        assert it.prefix_key == bs.prefix_key(b"prompt", full, PROMPT, spk) != bs.prefix_key(b"prompt", full, PROMPT)
    # without the keys nothing changes
    for it in srv._prepare(_msg(token_ids=IDS, seed=3)):
        assert np.array_equal(it.prefix, srv.front.build_prefix(IDS[it.utt])) and it.prefix_key == bs.prefix_key(b"full", IDS[it.utt])
    # "speaker": "off" alone is a request without an embedding
    for it in srv._prepare(_msg(token_ids=IDS, speaker="off")):
        assert it.prefix.shape[0] == len(IDS[it.utt]) + 9


def test_a_voice_with_an_embedding_gives_both_halves():
    srv = _server()
    srv.runtime_voices.register("anna", PROMPT.tolist(), [11, 12], speaker=SPK)
    srv.runtime_voices.register("bare", PROMPT.tolist(), None)
    (it,) = srv._prepare(_msg(token_ids=IDS[:1], voice="anna"))
    full = [11, 12] + IDS[0]
    assert np.array_equal(it.prefix, srv.front.build_prefix(full, speaker=SPK)) and np.array_equal(it.prompt, PROMPT)
    assert it.prefix_key == bs.prefix_key(b"prompt", full, PROMPT, SPK)
    (off,) = srv._prepare(_msg(token_ids=IDS[:1], voice="anna", speaker="off"))          # suppressed
    assert np.array_equal(off.prefix, srv.front.build_prefix(full)) and off.prefix_key == bs.prefix_key(b"prompt", full, PROMPT)
    (own,) = srv._prepare(_msg(token_ids=IDS[:1], voice="anna", speaker_embedding=SPK2))  # the request's own wins
    assert np.array_equal(own.prefix, srv.front.build_prefix(full, speaker=SPK2))
    (bare,) = srv._prepare(_msg(token_ids=IDS[:1], voice="bare"))
    assert bare.prefix.shape[0] == len(IDS[0]) + 9
    srv.runtime_voices.register("anna", PROMPT.tolist(), None)                            # replaced without one: it is gone
    assert srv.runtime_voices.speaker("anna") is None and srv.runtime_voices.speaker("nobody") is None


def test_voice_directories(tmp_path):
    assert R.load_voice_speaker(str(tmp_path), H) is None
    np.save(tmp_path / "ref_spk_embedding.npy", SPK)
    got = R.load_voice_speaker(str(tmp_path), H)
    assert got.dtype == np.float32 and np.array_equal(got, SPK)
    for bad in (SPK[:-1], np.stack([SPK, SPK]), np.where(np.arange(H) == 3, np.nan, SPK).astype(np.float32), np.arange(H)):
        np.save(tmp_path / "ref_spk_embedding.npy", bad)
        with pytest.raises(ValueError):
            R.load_voice_speaker(str(tmp_path), H)


def test_text_stream_requests_take_the_same_keys_under_text_voice():
    good = dict(token_ids=[[5, 6, 7]], stream=True, text_stream=True)
    with pytest.raises(ValueError, match="speaker embedding"):
        _server()._prepare(_msg(speaker_embedding=SPK, **good))
    srv = _server(text_voice=True)
    (plain,) = srv._prepare(_msg(**good))
    (it,) = srv._prepare(_msg(speaker_embedding=SPK, **good))
    assert it.prefix.shape == (9, H) and np.array_equal(it.prefix, srv.front.build_prefix_stream(5, speaker=SPK))
    assert np.array_equal(it.prefix[:6], plain.prefix[:6]) and np.array_equal(it.prefix[7:], plain.prefix[6:])
    assert it.prefix_key == bs.prefix_key(b"stream", [5], None, SPK) != plain.prefix_key == bs.prefix_key(b"stream", [5])
    (both,) = srv._prepare(_msg(speaker_embedding=SPK, prompt_codes=PROMPT, prompt_token_ids=[11], **good))
    assert np.array_equal(both.prefix, srv.front.build_prefix_stream(5, [11], speaker=SPK)) and both.prefix.shape[0] == 10
    assert both.prefix_key == bs.prefix_key(b"stream", [11, 5], PROMPT, SPK)
    srv.n_ctx = 8 + CAP                                  # the speaker row counts: 9 rows + max_tokens no longer fit
    srv._prepare(_msg(**good))
    with pytest.raises(ValueError, match="n_ctx"):
        srv._prepare(_msg(speaker_embedding=SPK, **good))


BAD = [dict(speaker_embedding=SPK[:-1]), dict(speaker_embedding=[SPK, SPK]),
       dict(speaker="only"), dict(speaker="with_prompt"), dict(speaker="loud"),
       dict(speaker="only", prompt_codes=PROMPT), dict(speaker="with_prompt", prompt_codes=PROMPT),
       dict(speaker="only", speaker_embedding=SPK)]


@pytest.mark.parametrize("bad", BAD)
def test_a_malformed_request_gets_minus_two_alone(bad):
    srv = _server()
    sched = make(TextFakeEngine(), prepare=srv._prepare)
    s, cli = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    cli.settimeout(5)
    assert sched.submit(s, _msg(token_ids=IDS, **bad)) is False and len(sched._queue) == 0
    assert struct.unpack("<i", cli.recv(4))[0] == P.SENTINEL_ERROR
    sched.stop()


def test_a_non_finite_value_gets_minus_two():
    srv = _server()
    m = _msg(token_ids=IDS, speaker_embedding=SPK)
    for v in (float("nan"), float("inf"), 1e300):
        m["speaker_embedding"][3] = v
        with pytest.raises(ValueError):
            srv._prepare(json.loads(json.dumps(m)))        # (NaN / Infinity as Python's json writes and reads them)


def test_prompt_audio_speaker_modes_are_refused_from_the_json_alone():
    """_resolve_prompt_audio before any payload byte: no --speaker_encoder, "only" beside "register_voice", "speaker" beside
    "speaker_embedding", a clip below the speaker encoder's shortest."""
    class Enc:
        pass

    class Spk:
        min_samples = 1280
    srv = _server()
    srv.encoder, srv._encoder_samples = Enc(), 48000
    clip = (np.zeros(4000, np.int16), 16000)               # 6000 samples at 24 kHz
    for mode in ("only", "with_prompt"):
        with pytest.raises(ValueError, match="--speaker_encoder"):
            srv._resolve_prompt_audio(None, _msg(token_ids=IDS[:1], prompt_audio=clip, speaker=mode))
    srv.speaker = Spk()
    with pytest.raises(ValueError, match="register_voice"):
        srv._resolve_prompt_audio(None, _msg(texts=[], token_ids=None, prompt_audio=clip, speaker="only", register_voice="x"))
    with pytest.raises(ValueError, match="speaker_embedding"):
        srv._resolve_prompt_audio(None, _msg(token_ids=IDS[:1], prompt_audio=clip, speaker="only", speaker_embedding=SPK))
    with pytest.raises(ValueError, match="speaker must be"):
        srv._resolve_prompt_audio(None, _msg(token_ids=IDS[:1], prompt_audio=clip, speaker="loud"))
    short = (np.zeros(800, np.int16), 16000)                # 1200 samples at 24 kHz: below 1280
    for mode in ("only", "with_prompt"):
        with pytest.raises(ValueError, match="speaker encoder needs 1280"):
            srv._resolve_prompt_audio(None, _msg(token_ids=IDS[:1], prompt_audio=short, speaker=mode))


def test_the_prompt_audio_cache_keeps_the_embedding_beside_the_ids():
    c = R.PromptAudioCache(2)
    ids = np.zeros((3, 16), np.int64)
    assert c.get(b"a") is None and (c.hits, c.misses) == (0, 1)
    c.put(b"a", ids)
    assert c.get(b"a") is ids and (c.hits, c.misses) == (1, 1)                 # the old interface, the old counters
    assert c.lookup(b"a", True, True) == (ids, None) and (c.hits, c.misses) == (1, 2)      # ids there, embedding wanted: a miss
    c.put(b"a", speaker=SPK)
    got = c.lookup(b"a", True, True)
    assert got[0] is ids and got[1] is SPK and (c.hits, c.misses) == (2, 2)
    assert c.lookup(b"a", False, True)[1] is SPK and c.hits == 3
    c.put(b"b", speaker=SPK2)                                                              # "only": no ids
    assert c.lookup(b"b", False, True) == (None, SPK2) and c.lookup(b"b", True, False) == (None, SPK2) and c.misses == 3
    c.put(b"c", ids)
    assert len(c) == 2 and c.evictions == 1 and c.get(b"a") is None            # the least recently used went, ids and embedding
    z = R.PromptAudioCache(0)
    z.put(b"a", ids, SPK)
    assert z.lookup(b"a", True, True) == (None, None) and len(z) == 0
