"""The speaker row in the host text front-end (frontend.TextFrontEnd.build_prefix / build_prefix_stream, speaker=): rows
0..5 are the old rows 0..5, row 6 is tts_pad_embed + speaker (f32, in that order), rows 7.. are the old rows 6..;
speaker=None is the old output bit for bit; a wrong length or a non-finite value is refused.  CPU only."""
import os

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import frontend as fe
from qwen3_tts_axera_russian_amd import weights as W
from tests.util import CACHE


@pytest.fixture(scope="module")
def host():
    os.makedirs(CACHE, exist_ok=True)
    cfg = W.tiny_config(2, 2, text_vocab=640)
    path = os.path.join(CACHE, "text_t2c2_v640.q3w")
    if not os.path.exists(path):
        W.write_synthetic(path, cfg, seed=77, parts=("talker", "text"))
    return fe.load_text_front_end(path, cfg=cfg)[1]


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n", [0, 1, 17])
def test_build_prefix_speaker_row(host, n):
    r = np.random.default_rng(n)
    ids = r.integers(0, 600, size=n).tolist()
    spk = r.standard_normal(1024).astype(np.float32)
    old = host.build_prefix(ids)
    new = host.build_prefix(ids, speaker=spk)
    assert new.shape == (n + 10, 1024) and new.dtype == np.float32
    assert same(new[:6], old[:6]) and same(new[7:], old[6:])
    assert same(new[fe.SPEAKER_ROW], host.tts_pad_embed + spk) and fe.SPEAKER_ROW == 6
    assert same(host.build_prefix(ids, speaker=None), old) and same(host.build_prefix(ids, "russian", None), old)


@pytest.mark.parametrize("head", [(), (5, 6, 7)])
def test_build_prefix_stream_speaker_row(host, head):
    spk = np.random.default_rng(9).standard_normal(1024).astype(np.float32)
    old = host.build_prefix_stream(11, head)
    new = host.build_prefix_stream(11, head, speaker=spk)
    assert new.shape == (9 + len(head), 1024)
    assert same(new[:6], old[:6]) and same(new[7:], old[6:]) and same(new[6], host.tts_pad_embed + spk)
    assert same(host.build_prefix_stream(11, head, speaker=None), old)
    # the stream prefix shares rows 0..6 (+ the speaker row) with the whole prefix
    assert same(new[:8], host.build_prefix([11], speaker=spk)[:8])


def test_refusals(host):
    good = np.zeros(1024, np.float32)
    for bad in (np.zeros(1023, np.float32), np.zeros(2048, np.float32), np.full(1024, np.nan, np.float32),
                np.where(np.arange(1024) == 7, np.inf, good).astype(np.float32)):
        with pytest.raises(ValueError):
            host.build_prefix([1, 2], speaker=bad)
        with pytest.raises(ValueError):
            host.build_prefix_stream(1, speaker=bad)
    assert host.build_prefix([1, 2], speaker=good.tolist()).shape == (12, 1024)
