"""Prefix cache of the per-slot admissions (q3e_prefix_cache / q3e_admit_keyed / q3e_prefix_stats), on the tiny synthetic
pack of tests/test_gpu_concurrent.py.  A hit must leave the slot as a prefill leaves it, so every comparison here is array
equality: there is no tolerance (the one graded column uses tests/test_gpu_engine.py's _compare against the CPU pipeline,
as the per-slot tests do)."""
import numpy as np
import pytest

from oracle.pipeline import CpuPipeline
from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from tests.test_gpu_engine import _compare, _prefixes
from tests.util import synthetic_pack

pytestmark = pytest.mark.gpu

SAMPLED = dict(temperature=1.0, top_k=50, top_p=0.95, cp_temperature=1.0, cp_top_k=50)
F = 12
STAT_NAMES = ("hits", "misses", "stores", "evictions", "too_long", "in_use")


@pytest.fixture(scope="module")
def world():
    path, cfg, tensors = synthetic_pack(2, 2)
    return path, cfg, tensors, CpuPipeline(cfg, tensors, n_ctx=96)


def _engine(path, pad, cache=None):
    eng = FrameEngine(path, max_batch=4, n_ctx=96, max_frames=24)
    eng.set_pad_embed(pad)
    if cache:
        eng.prefix_cache(*cache)
    return eng


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
def test_a_hit_is_a_prefill_bit_for_bit(gpu_lib, world, mode):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(501)
    lens = [9, 16, 17, 33]                 # below the 16-row tile, the tile's edge, one past it, more than two tiles
    prefixes = _prefixes(rng, lens)
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    keys = [_key(i + 1) for i in range(4)]
    if mode == "greedy":
        params = [SlotParams(max_frames=F)] * 4
    else:
        params = [SlotParams(max_frames=F, seed=77, utt=u, **SAMPLED) for u in range(4)]
    eng = _engine(path, pad, cache=(4, 40))
    eng.open(4, ignore_eos=True)
    hit = eng.admit([0, 1, 2, 3], prefixes, [30] * 4, params, keys=keys)
    assert not hit.any()
    hid0 = eng.hidden()
    assert eng.run(F) == F
    codes, per = eng.codes()
    hid = eng.hidden()
    assert [int(x) for x in per] == [F] * 4 and (codes >= 0).all()
    # the same keys into other slots (the last one among them), the prefix rows replaced by zeros; the entries outlive q3e_open
    perm = [3, 2, 0, 1]
    eng.open(4, ignore_eos=True)
    hit = eng.admit(perm, [np.zeros_like(p) for p in prefixes], [30] * 4, params, keys=keys)
    assert hit.all()
    np.testing.assert_array_equal(eng.hidden()[perm], hid0)          # the frame-0 state, before any step
    assert eng.run(F) == F
    codes_hit, per_hit = eng.codes()
    assert [int(x) for x in per_hit] == [F] * 4
    np.testing.assert_array_equal(codes_hit[:, perm], codes)
    np.testing.assert_array_equal(eng.hidden()[perm], hid)
    assert _stats(eng) == (4, 4, 4, 0, 0, 4)
    eng.destroy()
    # ... and what q3e_admit gives on an engine that never had a cache
    plain = _engine(path, pad)
    plain.open(4, ignore_eos=True)
    assert plain.admit([0, 1, 2, 3], prefixes, [30] * 4, params) is None
    np.testing.assert_array_equal(plain.hidden(), hid0)
    assert plain.run(F) == F
    np.testing.assert_array_equal(plain.codes()[0], codes)
    np.testing.assert_array_equal(plain.hidden(), hid)
    plain.destroy()
    if mode == "greedy":
        b = 2
        ref, margins = cpu.generate(prefixes[b], 30, pad, F, ignore_eos=True, want_margins=True)
        print("hit column vs CPU pipeline:", _compare(codes_hit[:, perm[b]:perm[b] + 1], per_hit[perm[b]:perm[b] + 1], [ref], [margins]))


def test_neighbours_do_not_notice_a_hit(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(502)
    q0, q1, p = _prefixes(rng, [12, 19, 17])
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    S = [SlotParams(max_frames=F, seed=5, utt=u, **SAMPLED) for u in range(2)]
    eng = _engine(path, pad, cache=(2, 40))
    eng.open(4, ignore_eos=True)
    assert not eng.admit([2], [p], [30], [SlotParams(max_frames=F)], keys=[_key(9)]).any()   # stores the entry
    cols = []
    for with_hit in (False, True):
        eng.open(4, ignore_eos=True)
        eng.admit([0, 1], [q0, q1], [30, 30], S)
        assert eng.run(4) == 4
        if with_hit:
            assert eng.admit([3], [np.zeros_like(p)], [30], [SlotParams(max_frames=F)], keys=[_key(9)]).all()
        _finish(eng)
        cols.append((_column(eng, 0), _column(eng, 1)))
    assert cols[0][0].shape == (F, 16)
    np.testing.assert_array_equal(cols[1][0], cols[0][0])
    np.testing.assert_array_equal(cols[1][1], cols[0][1])
    eng.destroy()


def test_the_same_key_twice_in_one_call(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(503)
    (p,) = _prefixes(rng, [21])
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    G = SlotParams(max_frames=F)
    S = [SlotParams(max_frames=F, seed=31, utt=u, **SAMPLED) for u in range(2)]
    eng = _engine(path, pad, cache=(2, 40))
    eng.open(4, ignore_eos=True)
    hit = eng.admit([1, 3], [p, p], [30, 30], [G, G], keys=[_key(1), _key(1)])
    assert [bool(x) for x in hit] == [False, True]
    _finish(eng)
    assert _column(eng, 1).shape == (F, 16)
    np.testing.assert_array_equal(_column(eng, 3), _column(eng, 1))
    # two takes of one text with a seed: one prefill, two draws
    eng.open(4, ignore_eos=True)
    hit = eng.admit([0, 2], [p, p], [30, 30], S, keys=[_key(2), _key(2)])
    assert [bool(x) for x in hit] == [False, True]
    _finish(eng)
    takes = [_column(eng, 0), _column(eng, 2)]
    assert not np.array_equal(takes[0], takes[1])
    assert _stats(eng) == (2, 2, 2, 0, 0, 2)
    for u in range(2):                                   # each admitted apart, without the cache
        eng.open(4, ignore_eos=True)
        eng.admit([1], [p], [30], [S[u]])
        _finish(eng)
        np.testing.assert_array_equal(_column(eng, 1), takes[u])
    eng.destroy()


def test_least_recently_used_eviction_and_replacement(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(504)
    A, B, C, A2, L = _prefixes(rng, [9, 10, 11, 12, 21])
    a, b, c, l = _key(1), _key(2), _key(3), _key(4)
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    G = SlotParams(max_frames=6)
    eng = _engine(path, pad, cache=(2, 20))
    eng.open(4, ignore_eos=True)
    assert _stats(eng) == (0, 0, 0, 0, 0, 0)

    def admit(prefix, key, slot=0):
        eng.release([slot])
        return bool(eng.admit([slot], [prefix], [30], [G], keys=[key])[0])

    #                                   hits misses stores evictions too_long in_use
    assert not admit(A, a) and _stats(eng) == (0, 1, 1, 0, 0, 1)
    assert not admit(B, b) and _stats(eng) == (0, 2, 2, 0, 0, 2)
    assert not admit(C, c) and _stats(eng) == (0, 3, 3, 1, 0, 2)      # evicts A, the least recently used
    assert admit(B, b) and _stats(eng) == (1, 3, 3, 1, 0, 2)          # B is still there, and is now used after C
    assert not admit(A, a) and _stats(eng) == (1, 4, 4, 2, 0, 2)      # A is a miss again; it evicts C, not B
    assert admit(B, b) and _stats(eng) == (2, 4, 4, 2, 0, 2)
    assert not admit(C, c) and _stats(eng) == (2, 5, 5, 3, 0, 2)      # evicts A (B was touched after it)
    assert admit(B, b) and _stats(eng) == (3, 5, 5, 3, 0, 2)
    # a key with another n_rows is a miss that replaces its entry (no eviction, no further entry)
    assert not admit(A2, b) and _stats(eng) == (3, 6, 6, 3, 0, 2)
    assert admit(A2, b) and _stats(eng) == (4, 6, 6, 3, 0, 2)
    assert not admit(B, b) and _stats(eng) == (4, 7, 7, 3, 0, 2)
    assert admit(C, c) and _stats(eng) == (5, 7, 7, 3, 0, 2)          # the replacement touched nobody else
    # more rows than an entry holds: a plain admission, counted
    assert not admit(L, l) and _stats(eng) == (5, 7, 7, 3, 1, 2)
    assert not admit(L, l) and _stats(eng) == (5, 7, 7, 3, 2, 2)
    # after all that a hit still decodes what a prefill decodes
    eng.open(4, ignore_eos=True)
    assert eng.admit([3], [np.zeros_like(B)], [30], [G], keys=[b]).all()
    _finish(eng)
    from_cache = _column(eng, 3)
    # releasing the pool: keyed admissions are misses that store nothing
    eng.prefix_cache(0, 0)
    assert _stats(eng) == (6, 7, 7, 3, 2, 0)
    eng.open(4, ignore_eos=True)
    assert not eng.admit([0, 1], [B, B], [30, 30], [G, G], keys=[b, b]).any()
    assert _stats(eng) == (6, 9, 7, 3, 2, 0)
    _finish(eng)
    assert from_cache.shape == (6, 16)
    np.testing.assert_array_equal(_column(eng, 0), from_cache)
    np.testing.assert_array_equal(_column(eng, 1), from_cache)
    eng.destroy()


def test_a_keyed_text_slot(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(505)
    (p,) = _prefixes(rng, [8])
    rows = (0.05 * rng.standard_normal((7, 1024))).astype(np.float32)
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    T = SlotParams(max_frames=F, text_stream=True)
    eng = FrameEngine(path, max_batch=4, n_ctx=96, max_frames=24)
    eng.set_pad_embed(pad)
    eng.prefix_cache(2, 16)
    eng.reserve_text(16)                                 # (the entries and the pool outlive the reservation)
    cols = []
    for slot, prefix, want in ((1, p, False), (2, np.zeros_like(p), True), (0, np.zeros_like(p), True)):
        eng.open(4, ignore_eos=True)
        hit = eng.admit([slot], [prefix], [0], [T], keys=[_key(7)])
        assert bool(hit[0]) == want
        eng.push_text(slot, rows[:3])
        assert eng.run(8) == 3
        eng.push_text(slot, rows[3:], final=True, n_text=7)
        _finish(eng)
        cols.append(_column(eng, slot))
    assert cols[0].shape == (F, 16)
    np.testing.assert_array_equal(cols[1], cols[0])
    np.testing.assert_array_equal(cols[2], cols[0])
    assert _stats(eng) == (2, 1, 1, 0, 0, 1)
    eng.destroy()


def _raw_admit_keyed(eng, slots, prefixes, n_text, params, keys):
    """q3e_admit_keyed without FrameEngine.admit's own checks; params as (max_frames, temperature, top_k, top_p,
    cp_temperature, cp_top_k, seed, utt, reserved) -> (return code, hit flags)."""
    slots = np.asarray(slots, np.int32)
    cat = np.ascontiguousarray(np.concatenate(prefixes, axis=0), dtype=np.float32)
    n_rows = np.array([p.shape[0] for p in prefixes], np.int32)
    nt = np.asarray(n_text, np.int32)
    arr = (hiplib.SlotParamsC * len(params))(*[hiplib.SlotParamsC(*p) for p in params])
    kk = np.stack([np.frombuffer(k, "<u8") for k in keys]).astype(np.uint64)
    hit = np.full(len(slots), -7, np.int32)
    import ctypes
    rc = eng._lib.q3e_admit_keyed(eng.h, len(slots), hiplib.iptr(slots), hiplib.fptr(cat), hiplib.iptr(n_rows), hiplib.iptr(nt),
                                  arr, kk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), hiplib.iptr(hit))
    return rc, hit


def test_errors_change_nothing(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(506)
    p, q, r, too_long = _prefixes(rng, [14, 11, 10, 90])
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    G = SlotParams(max_frames=F)
    g = (F, 0.0, 50, 1.0, 0.0, 50, 0, 0, 0)
    eng = _engine(path, pad, cache=(2, 40))
    eng.open(4, ignore_eos=True)                         # what slot 0's utterance decodes when nothing disturbs it
    eng.admit([0], [p], [30], [G])
    _finish(eng)
    alone = _column(eng, 0)
    eng.open(4, ignore_eos=True)
    assert not eng.admit([0], [p], [30], [G], keys=[_key(1)]).any()
    assert eng.run(3) == 3
    before = _stats(eng)
    assert before == (0, 1, 1, 0, 0, 1)
    bad_calls = [
        ([1, 7], [q, r], [g, g]),                                                    # a slot out of range
        ([1, 1], [q, r], [g, g]),                                                    # ... or listed twice
        ([1, 2], [q, too_long], [g, g]),                                             # 90 rows + 12 frames > n_ctx = 96
        ([1, 2], [q, r], [g, (25,) + g[1:]]),                                        # a budget beyond max_frames = 24
        ([1, 2], [q, r], [g, (F, float("nan")) + g[2:]]),                            # a temperature that is no number
        ([1, 2], [q, r], [g, (F, 1.0, 50, 0.0) + g[4:]]),                            # top_p outside (0, 1]
        ([1, 2], [q, r], [g, g[:8] + (1,)]),                                         # a text slot without a reservation
    ]
    for slots, prefixes, params in bad_calls:
        rc, hit = _raw_admit_keyed(eng, slots, prefixes, [30, 30], params, [_key(2), _key(3)])
        assert rc < 0 and (hit == -7).all(), (slots, rc, hit)
        assert _stats(eng) == before
    done, per = eng.done()
    assert not done[0] and int(per[0]) == 3 and done[1:].all()           # utterance 0 of a refused call was not admitted
    _finish(eng)
    np.testing.assert_array_equal(_column(eng, 0), alone)
    # the refused calls stored nothing: their first key is still a miss, the stored one still a hit
    eng.open(4, ignore_eos=True)
    hit = eng.admit([1, 2], [q, np.zeros_like(p)], [30, 30], [G, G], keys=[_key(2), _key(1)])
    assert [bool(x) for x in hit] == [False, True]
    assert _stats(eng) == (1, 2, 2, 0, 0, 2)
    # a reservation that is refused leaves the pool and its entries
    for n_entries, max_rows in ((-1, 8), (2, -1), (2, 0)):
        with pytest.raises(ValueError):
            eng.prefix_cache(n_entries, max_rows)
    assert _stats(eng) == (1, 2, 2, 0, 0, 2)
    eng.release([2])
    assert eng.admit([2], [np.zeros_like(p)], [30], [G], keys=[_key(1)]).all()
    eng.release([1])
    _finish(eng)
    np.testing.assert_array_equal(_column(eng, 2), alone)
    with pytest.raises(ValueError):
        eng.admit([3], [q], [30], [G], keys=[b"short"])
    eng.destroy()
