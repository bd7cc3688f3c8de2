"""Record framing of the batch server's streamed reply (CPU only): pack -> parse round trip over a socket pair, and a reply cut
short raises instead of returning a partial record."""
import socket
import struct

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import batch_server as bs


def _reader(payload):
    a, b = socket.socketpair()
    a.sendall(payload)
    a.close()
    return b


def test_records_round_trip():
    rng = np.random.default_rng(3)
    pcm = rng.integers(-32768, 32767, size=1000).astype(np.int16)
    codes = rng.integers(0, 2048, size=(7, 16)).astype(np.int32)
    payload = (bs.pack_stream_audio(2, pcm) + bs.pack_stream_audio(0, np.zeros(0, np.int16)) + bs.pack_stream_end(2, codes)
               + bs.pack_stream_end(1, np.zeros((0, 16), np.int32)) + struct.pack("<i", -1))
    assert payload[:12] == struct.pack("<iii", 1, 2, 1000)
    r = _reader(payload)
    try:
        kind, utt, got = bs.read_stream_record(r)
        assert (kind, utt) == ("audio", 2)
        np.testing.assert_array_equal(got, pcm)
        kind, utt, got = bs.read_stream_record(r)
        assert (kind, utt, len(got)) == ("audio", 0, 0)
        kind, utt, got = bs.read_stream_record(r)
        assert (kind, utt) == ("end", 2)
        np.testing.assert_array_equal(got, codes)
        kind, utt, got = bs.read_stream_record(r)
        assert (kind, utt, got.shape) == ("end", 1, (0, 16))
        assert bs.read_stream_record(r) == ("done",)
    finally:
        r.close()


def test_request_carries_the_stream_flag():
    import json
    raw = bs.pack_batch_request(token_ids=[[1, 2]], stream=True)
    assert json.loads(raw[4:])["stream"] is True
    assert "stream" not in json.loads(bs.pack_batch_request(token_ids=[[1, 2]])[4:])


@pytest.mark.parametrize("cut", [2, 4, 10, 12, 13, 12 + 2 * 50 - 1])
def test_truncated_records_raise(cut):
    payload = bs.pack_stream_audio(0, np.arange(50, dtype=np.int16))
    r = _reader(payload[:cut])
    try:
        with pytest.raises(RuntimeError):
            bs.read_stream_record(r)
    finally:
        r.close()


def test_error_and_unknown_records_raise():
    for head in (struct.pack("<i", -2), struct.pack("<iii", 7, 0, 0)):
        r = _reader(head)
        try:
            with pytest.raises(RuntimeError):
                bs.read_stream_record(r)
        finally:
            r.close()


def test_new_entries_cuts_each_slots_new_frames():
    """new_entries over two successive checks of three slots: slot 0 grows in both, slot 1 grows once and then finishes with
    no new frame, slot 2 never has a frame and is not finished."""
    codes = (np.arange(5 * 3 * 16, dtype=np.int64).reshape(5, 3, 16) * 7) % 2048       # [frames][B=3][16]
    slots, pushed = [(0, 4), (1, 9), (2, 5)], [0, 0, 0]
    first = bs.new_entries(codes, [2, 3, 0], slots, pushed, finished=[])
    assert [(e.slot, e.utt, e.finished) for e in first] == [(0, 4, False), (1, 9, False)]      # nothing new, not finished: no entry
    np.testing.assert_array_equal(first[0].frames, codes[0:2, 0, :])
    np.testing.assert_array_equal(first[1].frames, codes[0:3, 1, :])
    assert first[0].codes is None and first[1].codes is None and pushed == [2, 3, 0]
    second = bs.new_entries(codes, [5, 3, 0], slots, pushed, finished={1})
    assert [(e.slot, e.utt, e.finished) for e in second] == [(0, 4, False), (1, 9, True)]
    np.testing.assert_array_equal(second[0].frames, codes[2:5, 0, :])                    # exactly codes[pushed:n]
    assert second[0].frames.flags["C_CONTIGUOUS"] and second[0].codes is None
    slot, utt, frames, finished, whole = second[1]                                       # (a push unpacks five values)
    assert frames.shape == (0, 16) and finished                                          # finished with no new frame: empty slice
    assert whole.dtype == np.int32 and whole.shape == (3, 16) and whole.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(whole, codes[0:3, 1, :])
    assert pushed == [5, 3, 0]


def test_the_wire_module_imports_no_engine_vocoder_or_loader():
    import os
    import subprocess
    import sys
    pkg = "qwen3_tts_axera_russian_amd"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import sys, {pkg}.batch_wire; "
            f"print([m for m in ('hiplib', 'engine', 'vocoder') if '{pkg}.' + m in sys.modules])")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True, cwd=root)
    assert out.stdout.strip() == "[]"
