"""tfe_build_prefix_spk / tfe_build_prefix_stream_spk on the GPU (include/qwen3tts_text.h): bit for bit the rows of the
unspeakered call with ONE row inserted at index 6, the call's own projected tts_pad row + the embedding as an f32 add; spk ==
NULL is bit for bit the old call; a non-finite value or a wrong length is refused and the handle stays good.

The projected tts_pad row of a call is read through tfe_embed_text of the ids the call projects (the six special ids, then the
text): the projection's GEMM variant follows the number of rows, so a row's bits are those of a call of the same size, not
those of the three-row call that fills DeviceTextFrontEnd.tts_pad_embed."""
import os

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import frontend as fe
from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from tests.util import CACHE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu_lib):
    os.makedirs(CACHE, exist_ok=True)
    cfg = W.tiny_config(2, 2, text_vocab=640)
    path = os.path.join(CACHE, "text_t2c2_v640.q3w")
    if not os.path.exists(path):
        W.write_synthetic(path, cfg, seed=77, parts=("talker", "text"))
    d = fe.DeviceTextFrontEnd(cfg, path, max_tokens=100)
    yield d
    d.destroy()


def dev_codec(dev):
    _, t = W.read_pack(os.path.join(CACHE, "text_t2c2_v640.q3w"))
    return np.asarray(t["talker.codec_embedding"], np.float32)


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n", [0, 1, 17, 100])
def test_prefix_spk(dev, n):
    r = np.random.default_rng(n)
    ids = r.integers(0, 600, size=n).tolist()
    spk = r.standard_normal(1024).astype(np.float32)
    old, new = dev.build_prefix(ids), dev.build_prefix(ids, speaker=spk)
    assert new.shape == (n + 10, 1024)
    assert same(new[:6], old[:6]) and same(new[7:], old[6:])
    pad = dev.embed_text([int(x) for x in dev._special[:6]] + ids)[3]
    assert same(old[5], pad + np.asarray(dev_codec(dev)[dev.cfg.codec_think_eos], np.float32))   # (the row before it: the same pad row)
    assert same(new[6], pad + spk)
    # spk == NULL is the old function, through the new symbol
    idp = np.ascontiguousarray(ids, np.int32)
    out = np.full((n + 10, 1024), np.nan, np.float32)
    rows = dev._lib.tfe_build_prefix_spk(dev.h, hiplib.iptr(idp) if n else None, n, hiplib.iptr(dev._special), None, hiplib.fptr(out))
    assert rows == n + 9 and same(out[:n + 9], old)


@pytest.mark.parametrize("head", [(), (5, 6, 7)])
def test_prefix_stream_spk(dev, head):
    spk = np.random.default_rng(5).standard_normal(1024).astype(np.float32)
    old, new = dev.build_prefix_stream(11, head), dev.build_prefix_stream(11, head, speaker=spk)
    assert new.shape == (9 + len(head), 1024)
    pad = dev.embed_text([int(x) for x in dev._special[:5]] + [11])[3]
    assert same(new[:6], old[:6]) and same(new[7:], old[6:])
    if not head:
        assert same(new[6], pad + spk)
    out = np.full((9, 1024), np.nan, np.float32)
    assert dev._lib.tfe_build_prefix_stream_spk(dev.h, 11, hiplib.iptr(dev._special), None, hiplib.fptr(out)) == 8
    assert same(out[:8], dev.build_prefix_stream(11))


def test_refusals_leave_the_handle_usable(dev, capfd):
    ids = np.array([1, 2, 3], np.int32)
    good = np.ones(1024, np.float32)
    want = dev.build_prefix(ids, speaker=good)
    out = np.zeros((13, 1024), np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        v = good.copy()
        v[1023] = bad
        capfd.readouterr()
        assert dev._lib.tfe_build_prefix_spk(dev.h, hiplib.iptr(ids), 3, hiplib.iptr(dev._special), hiplib.fptr(v), hiplib.fptr(out)) < 0
        assert dev._lib.tfe_build_prefix_stream_spk(dev.h, 1, hiplib.iptr(dev._special), hiplib.fptr(v), hiplib.fptr(out)) < 0
        assert capfd.readouterr().err.count("[qwen3tts] ") == 2
        with pytest.raises(ValueError):
            dev.build_prefix(ids, speaker=v)
    with pytest.raises(ValueError):          # spk_dim != hidden: refused at the Python layer
        dev.build_prefix(ids, speaker=np.ones(512, np.float32))
    with pytest.raises(ValueError):
        dev.build_prefix_stream(1, speaker=np.ones(1025, np.float32))
    assert same(dev.build_prefix(ids, speaker=good), want)
