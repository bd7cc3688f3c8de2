"""Prefix cache and codec prompts (q3e_admit_prompted with keys): an entry of a prompted utterance holds its n_rows + T
rows, a hit rebuilds the sampler's history from the codes and reads no prefix row.  Array equality throughout, as in
tests/test_gpu_prefix_cache.py."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from tests import prompt_ref as pr
from tests.test_gpu_concurrent import SAMPLED
from tests.test_gpu_engine import _prefixes
from tests.util import synthetic_pack

pytestmark = pytest.mark.gpu

F = 10
STAT_NAMES = ("hits", "misses", "stores", "evictions", "too_long", "in_use")


def _key(i):
    return bytes([i]) * 16


def _finish(eng):
    while eng.run(8) > 0:
        pass


def _column(eng, b):
    codes, per = eng.codes()
    return np.ascontiguousarray(codes[:int(per[b]), b, :])


def _stats(eng):
    s = eng.prefix_stats()
    return tuple(s[k] for k in STAT_NAMES)


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_a_prompted_hit_is_a_prompted_prefill(gpu_lib, mode):
    path, cfg, tensors = synthetic_pack(2, 2)
    rng = np.random.default_rng(801)
    p, q = _prefixes(rng, [12, 31])
    P, Q, P2 = pr.random_prompt(rng, 33), pr.random_prompt(rng, 33), pr.random_prompt(rng, 20)
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    if mode == "greedy":
        S = [SlotParams(max_frames=F)] * 2
    else:
        S = [SlotParams(max_frames=F, seed=21, utt=u, **SAMPLED) for u in range(2)]
    eng = FrameEngine(path, max_batch=4, n_ctx=128, max_frames=24)
    eng.set_pad_embed(pad)
    eng.prefix_cache(3, 64)                              # 12 + 33 and 31 + 33 rows fit, 31 + 33 + 1 would not
    eng.open(4, ignore_eos=True)
    hit = eng.admit([0, 1], [p, q], [30, 30], S, keys=[_key(1), _key(2)], prompts=[P, Q])
    assert not hit.any() and _stats(eng) == (0, 2, 2, 0, 0, 2)
    hid0 = eng.hidden()[:2].copy()
    _finish(eng)
    miss = [_column(eng, 0), _column(eng, 1)]
    assert miss[0].shape == (F, 16) and miss[1].shape == (F, 16)
    # the hit: other slots, beside each other in the other order, prefix rows of zeros -- the codes are still given
    eng.open(4, ignore_eos=True)
    hit = eng.admit([3, 2], [np.zeros_like(q), np.zeros_like(p)], [30, 30], S[::-1], keys=[_key(2), _key(1)], prompts=[Q, P])
    assert hit.all() and _stats(eng) == (2, 2, 2, 0, 0, 2)
    np.testing.assert_array_equal(eng.hidden()[[2, 3]], hid0)
    _finish(eng)
    np.testing.assert_array_equal(_column(eng, 2), miss[0])
    np.testing.assert_array_equal(_column(eng, 3), miss[1])
    # the same key with another T: a miss that replaces the entry (no eviction, no further entry) ...
    eng.open(4, ignore_eos=True)
    assert not eng.admit([0], [p], [30], S[:1], keys=[_key(1)], prompts=[P2]).any()
    assert _stats(eng) == (2, 3, 3, 0, 0, 2)
    _finish(eng)
    shorter = _column(eng, 0)
    assert not np.array_equal(shorter, miss[0])
    # ... which the old length no longer hits, and the new one does
    eng.open(4, ignore_eos=True)
    hit = eng.admit([1, 2], [np.zeros_like(p), p], [30, 30], [S[0], S[0]], keys=[_key(1), _key(1)], prompts=[P2, P])
    assert [bool(x) for x in hit] == [True, False] and _stats(eng) == (3, 4, 4, 0, 0, 2)
    _finish(eng)
    np.testing.assert_array_equal(_column(eng, 1), shorter)
    np.testing.assert_array_equal(_column(eng, 2), miss[0])
    # without a prompt the key's length is the prefix's alone: another miss
    eng.open(4, ignore_eos=True)
    assert not eng.admit([0], [p], [30], S[:1], keys=[_key(1)], prompts=[None]).any()
    assert _stats(eng) == (3, 5, 5, 0, 0, 2)
    eng.destroy()


def test_a_prompt_that_makes_the_utterance_too_long_to_cache(gpu_lib):
    path, cfg, tensors = synthetic_pack(2, 2)
    rng = np.random.default_rng(802)
    (p,) = _prefixes(rng, [12])
    P = pr.random_prompt(rng, 33)
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    G = SlotParams(max_frames=F)
    eng = FrameEngine(path, max_batch=4, n_ctx=128, max_frames=24)
    eng.set_pad_embed(pad)
    eng.open(4, ignore_eos=True)
    eng.admit([0], [p], [30], [G], prompts=[P])
    _finish(eng)
    want = _column(eng, 0)
    assert want.shape == (F, 16)
    eng.prefix_cache(2, 44)                              # the 12 prefix rows would fit; 12 + 33 rows do not
    for k in range(2):
        eng.open(4, ignore_eos=True)
        assert not eng.admit([1 + k], [p], [30], [G], keys=[_key(5)], prompts=[P]).any()
        assert _stats(eng) == (0, 0, 0, 0, 1 + k, 0)
        _finish(eng)
        np.testing.assert_array_equal(_column(eng, 1 + k), want)
    eng.prefix_cache(2, 45)                              # one row more: cached
    eng.open(4, ignore_eos=True)
    assert not eng.admit([0], [p], [30], [G], keys=[_key(5)], prompts=[P]).any()
    assert eng.admit([1], [np.zeros_like(p)], [30], [G], keys=[_key(5)], prompts=[P]).all()
    assert _stats(eng) == (1, 1, 1, 0, 2, 1)
    _finish(eng)
    np.testing.assert_array_equal(_column(eng, 0), want)
    np.testing.assert_array_equal(_column(eng, 1), want)
    eng.destroy()
