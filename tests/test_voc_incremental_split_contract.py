"""The split-fp16 arithmetic of the incremental decode, checked without a GPU: the batch server reads a request's
"vocoder_arithmetic" key (and refuses it outside "vocoder": "incremental"), the library exports the new entry points, the header
declares them and states the per-entry overflow contract, and the new kernel is on the build's no-spill list."""
import ctypes
import json
import os
import re
import socket
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("voc_incr_set_arithmetic", "voc_incr_arithmetic", "voc_incr_last_split_launches", "voc_incr_last_redone")


def test_request_key_is_validated():
    from qwen3_tts_axera_russian_amd import batch_server as bs
    assert bs.request_vocoder_arithmetic({}) == "exact"
    assert bs.request_vocoder_arithmetic({"vocoder": "walk"}) == "exact"
    assert bs.request_vocoder_arithmetic({"vocoder": "incremental"}) == "exact"
    assert bs.request_vocoder_arithmetic({"vocoder": "incremental", "vocoder_arithmetic": "exact"}) == "exact"
    assert bs.request_vocoder_arithmetic({"vocoder": "incremental", "vocoder_arithmetic": "split"}) == "split"
    for bad in ("Split", "", "fp16", None, 1, True, ["split"]):
        with pytest.raises(ValueError):
            bs.request_vocoder_arithmetic({"vocoder": "incremental", "vocoder_arithmetic": bad})
    for arith in ("exact", "split"):            # the key without "vocoder": "incremental"
        for msg in ({"vocoder_arithmetic": arith}, {"vocoder": "walk", "vocoder_arithmetic": arith}):
            with pytest.raises(ValueError):
                bs.request_vocoder_arithmetic(msg)
    with pytest.raises(ValueError):
        bs.request_vocoder_arithmetic({"vocoder": "fast", "vocoder_arithmetic": "split"})
    raw = bs.pack_batch_request(token_ids=[[1, 2]], stream=True, vocoder="incremental", vocoder_arithmetic="split")
    (n,) = struct.unpack("<I", raw[:4])
    msg = json.loads(raw[4:4 + n])
    assert msg["vocoder"] == "incremental" and msg["vocoder_arithmetic"] == "split" and msg["stream"] is True
    assert "vocoder_arithmetic" not in json.loads(bs.pack_batch_request(token_ids=[[1, 2]], vocoder="incremental")[4:])


def test_scheduler_answers_minus_two_and_carries_the_arithmetic():
    """--concurrent, no GPU: a bad value, and the key on a request that is not incremental, are answered -2 by the accept side
    (the server's own send_error writes the sentinel); a good request carries its arithmetic to the workers in its state."""
    from qwen3_tts_axera_russian_amd import batch_server as bs

    def prepare(msg):
        bs.request_vocoder_arithmetic(msg)
        return [bs.Utterance(0, None, 1, None)]
    sched = bs.ConcurrentScheduler(None, 2, 8, prepare, None, None, None, bs.BatchSynthesisServer._send_error)
    try:
        for msg in ({"vocoder": "incremental", "vocoder_arithmetic": "half"}, {"vocoder_arithmetic": "split"},
                    {"vocoder": "walk", "vocoder_arithmetic": "exact", "stream": True}):
            a, b = socket.socketpair()
            assert sched.submit(a, msg) is False
            assert struct.unpack("<i", b.recv(4))[0] == -2
            b.close()
        for msg, want in (({"vocoder": "incremental", "vocoder_arithmetic": "split", "stream": True}, "split"),
                          ({"vocoder": "incremental"}, "exact"), ({}, "exact")):
            c, d = socket.socketpair()
            assert sched.submit(c, msg) is True
            req, _ = sched._queue[-1]
            assert req.state.arithmetic == want and req.state.vocoder == msg.get("vocoder", "walk")
            c.close()
            d.close()
    finally:
        sched._pool.shutdown(wait=True)


def test_symbols_are_exported_declared_and_bound():
    from qwen3_tts_axera_russian_amd import build
    lib = ctypes.CDLL(build.build())
    src = open(os.path.join(ROOT, "include", "qwen3tts_voc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    binding = open(os.path.join(ROOT, "qwen3_tts_axera_russian_amd", "hiplib.py")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*void\s*\*", code), name
        assert f'"{name}"' in binding, name
    for phrase in ("transaction per entry", "never degrades a result silently", "never depend on whether a neighbour overflowed",
                   "which push was redone"):
        assert phrase in src, phrase
    assert "voc_incr_prepend_split_kernel" in build.NO_SPILL
    assert lib.voc_incr_set_arithmetic(None, 1) < 0 and lib.voc_incr_arithmetic(None) < 0      # no handle: an error, no crash
