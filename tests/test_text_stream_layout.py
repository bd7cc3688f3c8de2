"""Layout of a text-stream utterance on the host (TextFrontEnd.build_prefix_stream, text_stream_rows) against a numpy
restatement of the layout as include/qwen3tts_engine.h states it, and the text records of the wire protocol.  CPU only."""
import socket

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import frontend as fe
from qwen3_tts_axera_russian_amd import protocol as P
from qwen3_tts_axera_russian_amd.weights import ModelConfig


@pytest.fixture(scope="module")
def front():
    r = np.random.default_rng(11)
    emb = (0.05 * r.standard_normal((640, 96))).astype(np.float32)
    fc1_w, fc1_b = (0.1 * r.standard_normal((80, 96))).astype(np.float32), (0.02 * r.standard_normal(80)).astype(np.float32)
    fc2_w, fc2_b = (0.1 * r.standard_normal((64, 80))).astype(np.float32), (0.02 * r.standard_normal(64)).astype(np.float32)
    codec = (0.05 * r.standard_normal((3072, 64))).astype(np.float32)
    cfg = ModelConfig(text_vocab=640, tts_pad=151671 % 640, tts_bos=151672 % 640, tts_eos=151673 % 640,
                      im_start=151644 % 640, assistant=77091 % 640, newline=198 % 640)
    return cfg, fe.TextFrontEnd(cfg, emb, fc1_w, fc1_b, fc2_w, fc2_b, codec), (emb, fc1_w, fc1_b, fc2_w, fc2_b, codec)


def _project(tables, ids):
    emb, fc1_w, fc1_b, fc2_w, fc2_b, _ = tables
    h = emb[np.asarray(ids)] @ fc1_w.T + fc1_b
    h = h * (1.0 / (1.0 + np.exp(-h)))
    return (h @ fc2_w.T + fc2_b).astype(np.float32)


def test_streaming_prefix_and_trailing_rows(front):
    cfg, f, tables = front
    codec = tables[5]
    ids = [5, 17, 200, 33, 41, 7]
    got = f.build_prefix_stream(ids[0])
    pad, bos, eos = _project(tables, [cfg.tts_pad, cfg.tts_bos, cfg.tts_eos])
    want = np.stack(list(_project(tables, [cfg.im_start, cfg.assistant, cfg.newline]))                 # rows 0..2: role rows
                    + [pad + codec[c] for c in (cfg.codec_nothink, cfg.codec_think_bos, cfg.codec_think_eos)]   # rows 3..5
                    + [bos + codec[cfg.codec_pad]]                                                      # row 6
                    + [_project(tables, [ids[0]])[0] + codec[cfg.codec_bos]])                           # row 7: T[0] + codec_bos
    assert got.shape == (8, 64) and got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    np.testing.assert_array_equal(got[:7], f.build_prefix(ids)[:7])        # today's prefix up to tts_bos, bit for bit
    assert not np.array_equal(got[7], f.build_prefix(ids)[7])              # (there: T[0] + codec_pad)
    # trailing rows R = [T[1], .., T[n-1], E]: n rows, each token projected on its own
    R = fe.text_stream_rows(f, ids[1:], final=True)
    assert R.shape == (len(ids), 64) and R.dtype == np.float32
    np.testing.assert_allclose(R[:-1], _project(tables, ids[1:]), rtol=0, atol=1e-6)
    np.testing.assert_array_equal(R[-1], f.tts_eos_embed)
    np.testing.assert_allclose(R[-1], eos, rtol=0, atol=1e-6)
    # a row does not depend on how the text was cut into pieces
    cut = np.concatenate([fe.text_stream_rows(f, ids[1:3]), fe.text_stream_rows(f, ids[3:4]), fe.text_stream_rows(f, []),
                          fe.text_stream_rows(f, ids[4:], final=True)])
    np.testing.assert_array_equal(cut, R)
    assert fe.text_stream_rows(f, []).shape == (0, 64)
    np.testing.assert_array_equal(fe.text_stream_rows(f, [], final=True), f.tts_eos_embed[None])


def test_text_records_round_trip_and_survive_any_cut():
    recs = [(P.TEXT_BYTES, "Привет, ми".encode()), (P.TEXT_IDS, [5, 17, 2 ** 31 - 1]), (P.TEXT_BYTES, b""), (P.TEXT_IDS, []),
            (P.TEXT_BYTES, "р!".encode()), (P.TEXT_END, None)]
    wire = b"".join(P.pack_text_record(k, b if b is not None else b"") for k, b in recs)
    assert P.pack_text_record(P.TEXT_BYTES, "р!") == P.pack_text_record(P.TEXT_BYTES, "р!".encode())

    def same(got):
        assert len(got) == len(recs)
        for (k, b), (gk, gb) in zip(recs, got):
            assert gk == k
            if k == P.TEXT_BYTES:
                assert gb == b
            elif k == P.TEXT_IDS:
                assert gb.dtype == np.int32 and list(gb) == list(b)
            else:
                assert gb is None
    same(P.TextRecordParser().feed(wire))
    for cut in range(len(wire) + 1):                         # a record split across two recvs, at every byte
        p = P.TextRecordParser()
        got = p.feed(wire[:cut]) + p.feed(wire[cut:])
        same(got)
        assert p.ended
    # through a socket, read the way the server reads: whatever has arrived, without blocking
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
    try:
        p, got = P.TextRecordParser(), []
        for part in (wire[:13], wire[13:14], wire[14:]):
            a.sendall(part)
            got += p.feed(b.recv(65536, socket.MSG_DONTWAIT))
            with pytest.raises(BlockingIOError):
                b.recv(65536, socket.MSG_DONTWAIT)
        same(got)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("bad", [b"\x03\0\0\0\0\0\0\0", b"\x01\0\0\0\xff\xff\xff\xff", b"\0\0\0\0\x01\0\0\0",
                                 b"\x02\0\0\0\0\0\x10\0", P.pack_text_record(P.TEXT_END) + b"\x01"])
def test_malformed_text_records_raise(bad):
    with pytest.raises(ValueError):
        P.TextRecordParser().feed(bad)
