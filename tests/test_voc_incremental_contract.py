"""What the carry-state incremental decode (voc_incr_*) rests on, checked without a GPU: S(n), the sample count of a whole
decode of n frames, is the table's convt_out chain; the model is causal, so the decode of the first n frames IS the first S(n)
samples of the decode of all N; the batch server reads the request's "vocoder" key; the header declares the entry points."""
import os
import re

import numpy as np
import pytest

from oracle.voc_ref import voc_reference
from qwen3_tts_axera_russian_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def samples_of(prog, n):
    """S(n): the convt_out chain of the table applied to n frames (0 where it is not positive)"""
    L = int(n)
    for row in np.asarray(prog):
        if int(row[0]) == W.VOP_CONVT:
            L = max(0, (L - 1) * int(row[4]) + int(row[3]) - int(row[6]) - int(row[7]))
    return L


def tiny(trim):
    vc = W.tiny_full_voc_config()      # transformer (window 24) + ConvNeXt: every op kind
    vc.convt_trim = trim
    return vc, W.make_synthetic_voc(vc, seed=7)


def test_sample_count_of_the_default_table():
    prog, _ = W.voc_program(W.VocConfig())
    assert samples_of(prog, 8) == 14805 and samples_of(prog, 64) == 122325 and samples_of(prog, 0) == 0
    right = W.VocConfig()
    right.convt_trim = "right"
    prog, _ = W.voc_program(right)
    assert [samples_of(prog, n) for n in (0, 1, 8, 64)] == [0, 1920, 8 * 1920, 64 * 1920]


@pytest.mark.parametrize("trim", ["both", "right"])
def test_sample_count_is_the_oracles_output_length(trim):
    vc, tens = tiny(trim)
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 8, 25, 70):
        codes = rng.integers(0, 2048, size=(1, n, 16)).astype(np.int64)
        assert voc_reference(tens, codes).shape == (1, samples_of(tens["voc.program"], n)), (trim, n)
        assert samples_of(tens["voc.program"], n) == W.voc_chunk_samples(vc, n)
    # every streamable table trims k - s on the right: a push of L more columns then adds exactly L * s samples
    for row in tens["voc.program"]:
        if int(row[0]) == W.VOP_CONVT:
            assert int(row[7]) == int(row[3]) - int(row[4]) and int(row[6]) <= int(row[4])


@pytest.mark.parametrize("trim", ["both", "right"])
def test_prefix_property(trim):
    """Decode of the first n frames == the first S(n) samples of the decode of all N = 100 frames, for every n in 1..N (the
    window of 24 is crossed four times).  Causality makes the two the same sums, but not in the same order: torch's CPU kernels
    block their reductions by the tensor's length (the first difference, one ulp, appears at the first RMSNorm's mean over the
    channels and is carried on from there), so float32 prefixes differ from the float32 whole decode by rounding noise --
    measured here up to 1.2e-6 of full scale, printed below for a sample of n, not asserted.  What is asserted is the property
    itself, on the same oracle evaluated in float64 (voc_reference's dtype), where that noise is 1e-15: every prefix within 1e-6."""
    vc, tens = tiny(trim)
    assert vc.tf_window == 24
    prog = tens["voc.program"]
    N = 100
    codes = np.random.default_rng(4).integers(0, 2048, size=(1, N, 16)).astype(np.int64)
    whole = voc_reference(tens, codes, dtype=np.float64)[0]
    assert whole.dtype == np.float64 and len(whole) == samples_of(prog, N) and np.abs(whole).max() > 0.05
    worst = 0.0
    for n in range(1, N + 1):
        part = voc_reference(tens, codes[:, :n], dtype=np.float64)[0]
        assert len(part) == samples_of(prog, n)
        if len(part):
            worst = max(worst, float(np.abs(part - whole[:len(part)]).max()))
    whole32 = voc_reference(tens, codes)[0]
    noise = max(float(np.abs(voc_reference(tens, codes[:, :n])[0] - whole32[:samples_of(prog, n)]).max()) for n in (2, 24, 25, 50, 99))
    print(f"{trim}: prefix decodes vs the whole decode, worst max abs difference {worst:.2e} in float64 "
          f"(float32 rounding noise of the same comparison: {noise:.2e})")
    assert worst <= 1e-6


def test_request_key_is_parsed_without_a_gpu():
    import json
    import struct
    from qwen3_tts_axera_russian_amd import batch_server as bs
    assert bs.request_vocoder({}) == "walk"
    assert bs.request_vocoder({"vocoder": "walk"}) == "walk"
    assert bs.request_vocoder({"vocoder": "incremental"}) == "incremental"
    for bad in ("Incremental", "", "chunk", None, 1, True, ["incremental"]):
        with pytest.raises(ValueError):
            bs.request_vocoder({"vocoder": bad})
    raw = bs.pack_batch_request(token_ids=[[1, 2]], stream=True, vocoder="incremental")
    (n,) = struct.unpack("<I", raw[:4])
    msg = json.loads(raw[4:4 + n])
    assert msg["vocoder"] == "incremental" and msg["stream"] is True
    assert "vocoder" not in json.loads(bs.pack_batch_request(token_ids=[[1, 2]])[4:])     # the default request is unchanged


def test_scheduler_refuses_a_bad_key_and_passes_a_good_one():
    """--concurrent, no GPU: a request with an unknown vocoder value is answered -2 by the accept side; the mode of a good
    request reaches the push worker through the request's state."""
    import socket
    from qwen3_tts_axera_russian_amd import batch_server as bs

    def prepare(msg):
        bs.request_vocoder(msg)
        return [bs.Utterance(0, None, 1, None)]
    errors = []
    sched = bs.ConcurrentScheduler(None, 2, 8, prepare, None, None, None, lambda conn: errors.append(conn))
    a, b = socket.socketpair()
    try:
        assert sched.submit(a, {"vocoder": "nope", "stream": True}) is False and errors == [a]
        c, d = socket.socketpair()
        assert sched.submit(c, {"vocoder": "incremental", "stream": True}) is True
        req, _ = sched._queue[0]
        assert req.state.vocoder == "incremental" and req.stream
        c.close()
        d.close()
    finally:
        b.close()
        sched._pool.shutdown(wait=True)


def test_header_declares_the_entry_points_and_the_contract():
    src = open(os.path.join(ROOT, "include", "qwen3tts_voc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("voc_incr_create", "voc_incr_free", "voc_incr_reset", "voc_incr_push_max_samples", "voc_incr_push",
                 "voc_incr_push_f32", "voc_incr_last_ms", "voc_incr_last_launches", "voc_incr_samples"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
    for phrase in ("S(8) = 14 805", "S(64) = 122 325", "exact-fp32", "chunk_tokens"):
        assert phrase in src, phrase
    from qwen3_tts_axera_russian_amd import build
    assert {"voc_attn_incr_kernel", "voc_incr_prepend_kernel"} <= set(build.NO_SPILL)
