"""TextFrontEnd.build_prefix_stream(first, head): the prefix of a text-stream utterance that continues a codec prompt --
rows 0..6 of the streaming prefix, one `text + codec_pad` row per token of the prompt's text, then the first token +
codec_bos -- row by row against rows assembled from build_prefix and embed_text.  CPU only."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import frontend as fe
from qwen3_tts_axera_russian_amd.weights import ModelConfig


@pytest.fixture(scope="module")
def front():
    r = np.random.default_rng(5)
    cfg = ModelConfig(text_vocab=64, tts_pad=61, tts_bos=62, tts_eos=63, im_start=60, assistant=59, newline=58)
    return fe.TextFrontEnd(cfg, r.standard_normal((64, 8)).astype(np.float32), r.standard_normal((8, 8)).astype(np.float32),
                           r.standard_normal(8).astype(np.float32), r.standard_normal((16, 8)).astype(np.float32),
                           r.standard_normal(16).astype(np.float32), r.standard_normal((3072, 16)).astype(np.float32))


def todays_eight_rows(front, first):
    """build_prefix_stream as it was before `head`, restated from build_prefix: rows 0..6, then first token + codec_bos."""
    c = front.cfg
    return np.concatenate([front.build_prefix([])[:7], front.embed_text([first]) + front.codec[c.codec_bos]], axis=0)


@pytest.mark.parametrize("first", [5, 0, 57])
def test_without_head_it_is_todays_eight_rows(front, first):
    want = todays_eight_rows(front, first)
    assert want.shape == (8, 16) and want.dtype == np.float32
    for got in (front.build_prefix_stream(first), front.build_prefix_stream(first, ()), front.build_prefix_stream(first, head=[])):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("head", [[7], [11, 12, 13], list(range(20, 41))])
def test_with_head_row_by_row(front, head):
    c = front.cfg
    first = 5
    got = front.build_prefix_stream(first, head)
    n = len(head)
    assert got.shape == (8 + n, 16) and got.dtype == np.float32
    full = front.build_prefix(head)                          # [role x3, think x3, bos, head.., eos, pad + codec_bos]
    np.testing.assert_array_equal(got[:7], front.build_prefix_stream(first)[:7])
    np.testing.assert_array_equal(got[:7 + n], full[:7 + n])
    for i, t in enumerate(head):                             # one `text + codec_pad` row per head token
        np.testing.assert_array_equal(got[7 + i], (front.embed_text(head) + front.codec[c.codec_pad])[i])
        # (the token projected alone: the same sums in another order -- two dot products of <= 16 f32 terms of size <= 30,
        # so within 2 * 16 * 2^-24 * 30 ~ 6e-5)
        np.testing.assert_allclose(got[7 + i], front.embed_text([t])[0] + front.codec[c.codec_pad], rtol=0, atol=1e-4)
    np.testing.assert_array_equal(got[7 + n], front.build_prefix_stream(first)[7])
    np.testing.assert_array_equal(got[7 + n], front.embed_text([first])[0] + front.codec[c.codec_bos])
    # neither the tts_eos row nor the pad + codec_bos row of the unstreamed prefix is in it
    assert not any(np.array_equal(r, full[7 + n]) or np.array_equal(r, full[8 + n]) for r in got)
    # the head is part of the rows
    assert not np.array_equal(front.build_prefix_stream(first, head[:-1] + [head[-1] + 1]), got)
