"""batch_server --concurrent --encoder without a GPU: the "prompt_audio" descriptor and every refusal the JSON alone decides,
the payload's framing behind the JSON (one clip, per-utterance clips, a short payload), the id cache's digest and LRU, the
run-time voice table, and the client's pack_batch_request -- with a stand-in encoder injected into a bare server, as
tests/test_codec_prompt_request.py injects its pieces.  CPU only."""
import json
import socket
import struct
import threading

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_request as br
from qwen3_tts_axera_russian_amd import batch_server as bs
from qwen3_tts_axera_russian_amd import protocol as P
from tests.test_text_stream_scheduler import _bare_server

MAX_SAMPLES = 24000 * 2          # --prompt_audio_seconds 2
R = np.random.default_rng(17)
CLIP = R.integers(-3000, 3000, size=(1600, 2)).astype(np.int16)        # 0.1 s of 16 kHz stereo
OTHER = (0.1 * R.standard_normal(4410)).astype(np.float32)              # 0.1 s of 44.1 kHz mono


class FakeEncoder:
    """Encoder.encode_pcm's interface: ids that depend on every sample, rate and channel count; remembers its calls."""

    def __init__(self):
        self.calls = []

    def encode_pcm(self, clips, rate, channels=1):
        self.calls.append((len(clips), rate, channels))
        out = []
        for c in clips:
            c = np.asarray(c)
            assert c.dtype in (np.int16, np.float32) and (c.ndim == 1 if channels == 1 else c.shape[1] == channels)
            seed = int(np.frombuffer(np.ascontiguousarray(c).tobytes(), np.uint8).astype(np.int64).sum()) + rate + channels
            T = max(1, -(-c.shape[0] * 24000 // rate) // 480)
            out.append(((seed + np.arange(T * 16).reshape(T, 16) * 7) % 64).astype(np.int64))
        return out


def server(voices=None, cache=4, max_voices=2, encoder=True):
    srv = _bare_server()
    srv.voices = dict(voices or {})
    srv.runtime_voices = br.VoiceTable(srv.voices, max_voices)
    srv._prompt_audio = br.PromptAudioCache(cache)
    srv._encoder_lock, srv._encoder_samples = threading.Lock(), MAX_SAMPLES
    srv.encoder = FakeEncoder() if encoder else None
    return srv


def resolve(srv, raw, cut=None):
    """the request's bytes as a client sends them -> (msg after _resolve_prompt_audio, its return value, what came back)"""
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    try:
        a.settimeout(5)
        b.settimeout(5)
        b.sendall(raw if cut is None else raw[:cut])
        b.shutdown(socket.SHUT_WR)
        msg = P.read_talker_request(a)
        done = srv._resolve_prompt_audio(a, msg)
        rest = a.recv(16) if not done else b""
        return msg, done, (b.recv(16) if done else rest)
    finally:
        a.close()
        b.close()


def test_pack_batch_request_round_trip():
    raw = bs.pack_batch_request(token_ids=[[5, 6]], prompt_audio=(CLIP, 16000), prompt_audio_max_frames=3, register_voice="anna", seed=4)
    (n,) = struct.unpack("<I", raw[:4])
    msg = json.loads(raw[4:4 + n].decode())
    assert msg["prompt_audio"] == {"format": "s16", "rate": 16000, "channels": 2, "frames": 1600, "max_frames": 3}
    assert msg["register_voice"] == "anna" and msg["seed"] == 4 and raw[4 + n:] == CLIP.astype("<i2").tobytes()
    (d,), shared = br.request_prompt_audio(msg["prompt_audio"], 1, MAX_SAMPLES)
    assert shared and d.nbytes == len(raw) - 4 - n and np.array_equal(d.array(raw[4 + n:]), CLIP) and d.samples_24k == 2400
    # per-utterance clips: a list of descriptors, the payloads in order
    raw = bs.pack_batch_request(token_ids=[[5], [6]], prompt_audio=[(OTHER, 44100), (CLIP[:, 0], 16000)])
    (n,) = struct.unpack("<I", raw[:4])
    msg = json.loads(raw[4:4 + n].decode())
    assert [d["format"] for d in msg["prompt_audio"]] == ["f32", "s16"] and [d["channels"] for d in msg["prompt_audio"]] == [1, 1]
    assert raw[4 + n:] == OTHER.astype("<f4").tobytes() + CLIP[:, 0].astype("<i2").tobytes()
    # without the keys the request is what it was
    assert bs.pack_batch_request(token_ids=[[5]]) == struct.pack("<I", len(json.dumps({"language": "russian", "token_ids": [[5]]}))) + \
        json.dumps({"language": "russian", "token_ids": [[5]]}).encode()
    with pytest.raises(TypeError):
        bs.pack_batch_request(token_ids=[[5]], prompt_audio=(CLIP.astype(np.int32), 16000))


GOOD = {"format": "s16", "rate": 16000, "channels": 2, "frames": 1600}
BAD_DESCRIPTORS = [
    "s16", 5, [GOOD, GOOD], [],                                                       # not an object / 2 or 0 clips for 1 utterance
    dict(GOOD, format="s24"), dict(GOOD, format=0), {k: v for k, v in GOOD.items() if k != "format"},
    dict(GOOD, rate=7999), dict(GOOD, rate=192001), dict(GOOD, rate=16000.0), dict(GOOD, rate="16000"), dict(GOOD, rate=True),
    dict(GOOD, rate=44101), dict(GOOD, rate=8001),                                    # max(up, down) > 640
    dict(GOOD, channels=0), dict(GOOD, channels=9), dict(GOOD, channels=1.5),
    dict(GOOD, frames=0), dict(GOOD, frames=-1), dict(GOOD, frames=2 ** 31), {k: v for k, v in GOOD.items() if k != "frames"},
    dict(GOOD, frames=32001),                                                         # 2 s at 16 kHz are 32000 frames
    dict(GOOD, rate=48000, frames=96001), dict(GOOD, rate=8000, frames=16001),
    dict(GOOD, max_frames=0), dict(GOOD, max_frames="3"), dict(GOOD, bits=16),
]


@pytest.mark.parametrize("bad", BAD_DESCRIPTORS, ids=lambda b: json.dumps(b)[:48])
def test_a_bad_descriptor_is_refused_from_the_json_alone(bad):
    with pytest.raises(ValueError):
        br.request_prompt_audio(bad, 1, MAX_SAMPLES)
    # through the server: refused before a byte of the payload is read (none is sent here: a read would raise another error)
    srv = server()
    raw = json.dumps({"token_ids": [[5, 6]], "prompt_audio": bad}).encode()
    with pytest.raises(ValueError, match="prompt_audio"):
        resolve(srv, struct.pack("<I", len(raw)) + raw)
    assert not srv.encoder.calls


def test_the_limits_are_the_front_ends():
    ok = lambda **kw: br.request_prompt_audio(dict(GOOD, **kw), 1, MAX_SAMPLES)[0][0]
    assert ok(frames=32000).samples_24k == MAX_SAMPLES and ok(rate=48000, frames=96000).samples_24k == MAX_SAMPLES
    assert ok(rate=8000, frames=16000).samples_24k == MAX_SAMPLES and ok(rate=8120, frames=10).samples_24k == 30
    assert ok(rate=44100, frames=7, channels=8, format="f32").nbytes == 7 * 8 * 4 and ok(max_frames=5).max_frames == 5
    from tests import pcm_ref
    for rate in (8000, 11025, 22050, 44100, 96000):
        assert ok(rate=rate, frames=1001).samples_24k == pcm_ref.out_len(1001, *pcm_ref.factors(rate))


def test_other_json_level_refusals():
    raw = lambda **kw: bs.pack_batch_request(**dict(dict(token_ids=[[5, 6]], prompt_audio=(CLIP, 16000)), **kw))
    with pytest.raises(ValueError, match="--encoder"):
        resolve(server(encoder=False), raw())
    with pytest.raises(ValueError, match="takes the place"):
        resolve(server(), raw(prompt_codes=[[1] * 16]))
    with pytest.raises(ValueError, match="takes the place"):
        resolve(server({"anna": ([[1] * 16], None)}), raw(voice="anna"))
    with pytest.raises(ValueError, match="2 utterances"):
        resolve(server(), raw(prompt_audio=[(CLIP, 16000)], token_ids=[[5], [6]]))
    with pytest.raises(ValueError, match="at least one utterance"):
        resolve(server(), raw(token_ids=[]))
    body = json.dumps({"token_ids": [[5]], "register_voice": "anna"}).encode()          # a name without audio
    with pytest.raises(ValueError, match='needs "prompt_audio"'):
        resolve(server(), struct.pack("<I", len(body)) + body)
    with pytest.raises(ValueError, match="single"):
        resolve(server(), raw(prompt_audio=[(CLIP, 16000)], register_voice="anna"))
    # a non-concurrent server's checks see the keys as a codec prompt's
    assert br.request_has_prompt({"prompt_audio": GOOD}) and br.request_has_prompt({"register_voice": "x"})


def test_one_clip_becomes_prompt_codes():
    srv = server()
    msg, done, rest = resolve(srv, bs.pack_batch_request(token_ids=[[5, 6], [7]], prompt_audio=(CLIP, 16000), prompt_token_ids=[11], seed=3))
    want = srv.encoder.__class__().encode_pcm([CLIP], 16000, 2)[0]
    assert not done and rest == b"" and "prompt_audio" not in msg
    assert msg["prompt_codes"] == want.tolist() and srv.encoder.calls == [(1, 16000, 2)]
    # from here on it is the "prompt_codes" request: the same utterances, keys and all
    a = srv._prepare(msg)
    b = srv._prepare(json.loads(bs.pack_batch_request(token_ids=[[5, 6], [7]], prompt_codes=want, prompt_token_ids=[11], seed=3)[4:].decode()))
    for x, y in zip(a, b):
        assert x.prefix_key == y.prefix_key and np.array_equal(x.prompt, y.prompt) and np.array_equal(x.prefix, y.prefix)
        assert (x.utt, x.n_text, x.params) == (y.utt, y.n_text, y.params)
    # "max_frames" keeps the first K ids
    msg, _, _ = resolve(srv, bs.pack_batch_request(token_ids=[[5]], prompt_audio=(CLIP, 16000), prompt_audio_max_frames=2))
    assert msg["prompt_codes"] == want[:2].tolist()


def test_per_utterance_clips_and_grouping():
    srv = server()
    mono = np.ascontiguousarray(CLIP[:, 0])
    clips = [(CLIP, 16000), (OTHER, 44100), (CLIP[:800], 16000), (mono, 16000), (CLIP, 16000)]
    msg, done, rest = resolve(srv, bs.pack_batch_request(token_ids=[[5]] * 5, prompt_audio=clips) + b"TAIL")
    fake = FakeEncoder()
    want = [fake.encode_pcm([a], r, 1 if a.ndim == 1 else a.shape[1])[0].tolist() for a, r in clips]
    assert msg["prompt_codes"] == want and rest == b"TAIL"          # exactly the payload was read: what follows stays
    # one call per (format, channels, rate); the repeated clip is encoded once
    assert sorted(srv.encoder.calls) == sorted([(2, 16000, 2), (1, 44100, 1), (1, 16000, 1)])
    assert (srv.prompt_audio_hits, srv.prompt_audio_misses) == (0, 4)


def test_a_short_payload_fails_the_request():
    srv = server()
    raw = bs.pack_batch_request(token_ids=[[5]], prompt_audio=(CLIP, 16000))
    for cut in (len(raw) - 1, len(raw) - CLIP.nbytes, len(raw) - CLIP.nbytes + 100):
        with pytest.raises(ValueError, match="payload ended"):
            resolve(srv, raw, cut=cut)
    assert not srv.encoder.calls and len(srv._prompt_audio) == 0
    msg, _, _ = resolve(srv, raw)                                    # the server goes on
    assert len(msg["prompt_codes"]) >= 1


def test_digest_and_lru():
    d = br.AudioDescriptor("s16", 16000, 2, 1600)
    raw = CLIP.tobytes()
    k = br.prompt_audio_digest(d, raw)
    assert len(k) == 32 and k == br.prompt_audio_digest(br.AudioDescriptor("s16", 16000, 2, 1600), bytes(raw))
    others = [br.AudioDescriptor("f32", 16000, 2, 800), br.AudioDescriptor("s16", 16000, 1, 3200), br.AudioDescriptor("s16", 8000, 2, 1600),
              br.AudioDescriptor("s16", 16000, 2, 1600, max_frames=1)]
    assert len({k} | {br.prompt_audio_digest(o, raw) for o in others}) == 5
    flipped = bytearray(raw)
    flipped[777] ^= 1
    assert br.prompt_audio_digest(d, flipped) != k
    # through the server: a second send is a hit and runs no encode; the LRU holds `cache` entries
    srv = server(cache=2)
    send = lambda a, r, **kw: resolve(srv, bs.pack_batch_request(token_ids=[[5]], prompt_audio=(a, r), **kw))[0]["prompt_codes"]
    first = send(CLIP, 16000)
    assert (srv.prompt_audio_hits, srv.prompt_audio_misses, len(srv.encoder.calls)) == (0, 1, 1)
    assert send(CLIP, 16000) == first
    assert (srv.prompt_audio_hits, srv.prompt_audio_misses, len(srv.encoder.calls)) == (1, 1, 1)
    assert send(CLIP, 16000, prompt_audio_max_frames=1) == first[:1]             # another K: another entry
    send(OTHER, 44100)                                                            # the third entry evicts the least recent: CLIP
    assert (srv.prompt_audio_misses, srv.prompt_audio_evictions, len(srv._prompt_audio)) == (3, 1, 2)
    send(CLIP, 16000, prompt_audio_max_frames=1)                                  # still there (and now the most recent)
    assert srv.prompt_audio_hits == 2
    assert send(CLIP, 16000) == first and srv.prompt_audio_misses == 4 and len(srv.encoder.calls) == 4
    none = server(cache=0)                                                        # 0 entries: nothing kept
    for _ in range(2):
        resolve(none, bs.pack_batch_request(token_ids=[[5]], prompt_audio=(CLIP, 16000)))
    assert (none.prompt_audio_hits, none.prompt_audio_misses, len(none.encoder.calls)) == (0, 2, 2)
    with pytest.raises(ValueError):
        br.PromptAudioCache(-1)


def test_registration_rules():
    srv = server({"fixed": ([[1] * 16], None)}, max_voices=2)
    reg = lambda name, clip=CLIP, **kw: resolve(srv, bs.pack_batch_request(**dict(dict(texts=[], prompt_audio=(clip, 16000), register_voice=name), **kw)))
    msg, done, reply = reg("anna", prompt_token_ids=[11, 12])
    assert done and reply == struct.pack("<i", 0)                                 # only registers: i32 0
    want = FakeEncoder().encode_pcm([CLIP], 16000, 2)[0].tolist()
    assert srv.runtime_voices.get("anna") == (want, [11, 12])
    # "voice": "anna" is then the request with the ids and the text
    by_voice = srv._prepare(json.loads(bs.pack_batch_request(token_ids=[[5, 6]], voice="anna")[4:].decode()))
    inline = srv._prepare(json.loads(bs.pack_batch_request(token_ids=[[5, 6]], prompt_codes=want, prompt_token_ids=[11, 12])[4:].decode()))
    assert by_voice[0].prefix_key == inline[0].prefix_key and np.array_equal(by_voice[0].prompt, inline[0].prompt)
    assert by_voice[0].n_text == inline[0].n_text == 4
    # with utterances the request registers AND is served as the "prompt_codes" request
    msg, done, _ = reg("bella", clip=CLIP[:800], token_ids=[[5]], texts=None)
    assert not done and "register_voice" not in msg and msg["prompt_codes"] == srv.runtime_voices.get("bella")[0]
    # a start-up name is protected, a run-time one is replaced, the third run-time name is refused
    with pytest.raises(ValueError, match="start-up"):
        reg("fixed")
    assert srv.voices["fixed"] == ([[1] * 16], None)
    reg("anna", clip=CLIP[:400])
    assert srv.runtime_voices.get("anna")[0] != want and srv.runtime_voices.get("anna")[1] is None
    with pytest.raises(ValueError, match="max_voices"):
        reg("carla")
    assert sorted(srv.runtime_voices.runtime_names()) == ["anna", "bella"] and "carla" not in srv.runtime_voices
    for bad in ("", 5, None):
        if bad is None:
            continue
        with pytest.raises(ValueError):
            reg(bad)
    with pytest.raises(ValueError, match="unknown voice"):
        srv._prepare(json.loads(bs.pack_batch_request(token_ids=[[5]], voice="carla")[4:].decode()))
    # every other request still answers "texts": [] as before
    with pytest.raises(ValueError, match="at least one utterance"):
        srv._prepare(json.loads(bs.pack_batch_request(token_ids=[])[4:].decode()))
