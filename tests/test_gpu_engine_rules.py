"""Per-slot sampler rules in the engine (q3e_rules_reserve / q3e_admit_ruled) on the tiny synthetic pack, B = 4, at most 16
frames: the decisions the rules change against the CPU reference of tests/rules_ref.py (inputs drawn so that every graded
decision has an oracle margin >= 2 * NEAR_TIE, then compared exactly), and everything the rules must NOT change -- default
rules, neighbours, recycled slots, the prefix cache, refused calls -- as array equality between engines."""
import ctypes

import numpy as np
import pytest

from oracle.pipeline import CpuPipeline
from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams, SlotRules
from tests import prompt_ref as pr
from tests import rules_ref as rr
from tests.test_gpu_codec_prompt import _fixed_point
from tests.test_gpu_concurrent import SAMPLED
from tests.test_gpu_engine import NEAR_TIE, _compare, _prefixes
from tests.util import synthetic_pack

pytestmark = pytest.mark.gpu

N_CTX = 128
F = 16
DEFAULT = SlotRules()


@pytest.fixture(scope="module")
def world():
    path, cfg, tensors = synthetic_pack(2, 2)
    return path, cfg, tensors, CpuPipeline(cfg, tensors, n_ctx=N_CTX)


def _engine(path, pad, rules, text=0, hold=False):
    eng = FrameEngine(path, max_batch=4, n_ctx=N_CTX, max_frames=24)
    eng.set_pad_embed(pad)
    if text:
        eng.reserve_text(text)
        if hold:
            eng.hold_text()
    if rules:
        eng.rules()
    return eng


@pytest.fixture(scope="module")
def engines(gpu_lib, world):
    """(an engine with the rules reserved, one without), one pad row for both; every test opens its own batch."""
    pad = (0.05 * np.random.default_rng(900).standard_normal(1024)).astype(np.float32)
    ruled, plain = _engine(world[0], pad, True), _engine(world[0], pad, False)
    yield ruled, plain, pad
    ruled.destroy()
    plain.destroy()


def _finish(eng):
    while eng.run(8) > 0:
        pass


def _column(eng, b):
    codes, per = eng.codes()
    return np.ascontiguousarray(codes[:int(per[b]), b, :])


def _solo(eng, prefix, n_text, sp, prompt=None, rules=None, slot=0, ignore_eos=True):
    eng.open(4, ignore_eos=ignore_eos)
    kw = {} if rules is None else dict(rules=[rules])
    eng.admit([slot], [prefix], [n_text], [sp], prompts=None if prompt is None else [prompt], **kw)
    _finish(eng)
    return _column(eng, slot)


# ---- 1. default rules change nothing ----------------------------------------------------------------------------------------
def _scenario(eng, rules):
    """A plain greedy utterance, a prompted sampled one, a sampled one and a text slot (held while it waits for rows where
    the engine holds) in one batch -> their four columns."""
    rng = np.random.default_rng(901)
    p0, p1, p2, p3 = _prefixes(rng, [12, 9, 17, 8])
    P = pr.random_prompt(rng, 33)
    rows = (0.05 * rng.standard_normal((10, 1024))).astype(np.float32)
    sps = [SlotParams(max_frames=F), SlotParams(max_frames=F, seed=5, utt=1, **SAMPLED), SlotParams(max_frames=F, seed=6, **SAMPLED),
           SlotParams(max_frames=12, text_stream=True, seed=7, **SAMPLED)]
    kw = {} if rules is None else dict(rules=rules)
    eng.open(4)
    eng.admit([0, 1, 2, 3], [p0, p1, p2, p3], [4, 30, 30, 0], sps, prompts=[None, P, None, None], **kw)
    eng.push_text(3, rows[:3])
    eng.run(6)
    eng.push_text(3, rows[3:], final=True, n_text=10)
    _finish(eng)
    return [_column(eng, b) for b in range(4)], eng.held_steps().tolist()


@pytest.mark.parametrize("hold", [False, True])
def test_default_rules_change_nothing(gpu_lib, world, hold):
    pad = (0.05 * np.random.default_rng(902).standard_normal(1024)).astype(np.float32)
    plain = _engine(world[0], pad, False, text=16, hold=hold)
    ruled = _engine(world[0], pad, True, text=16, hold=hold)
    try:
        want, held = _scenario(plain, None)
        assert [len(c) > 0 for c in want] == [True] * 4 and (held[3] > 0) == hold
        for rules in (None, [DEFAULT] * 4, [None, DEFAULT, None, SlotRules(rep_penalty=1.2, rep_window=30)]):
            got, held2 = _scenario(ruled, rules)
            assert held2 == held
            for b in range(4):
                np.testing.assert_array_equal(got[b], want[b], err_msg=f"slot {b}, rules {rules}")
    finally:
        plain.destroy()
        ruled.destroy()


# ---- 2. the whole-history window ----------------------------------------------------------------------------------------------
def find_history_case(cpu, pad):
    """A prompt of T = 40 whose clear frame-0 arg-max c stands only at frame T - 35: outside the last 30, outside the ring of
    32.  The default rules pick c; rep_window 0 penalises it and picks another id; both with a margin >= 2 * NEAR_TIE."""
    T = 40
    for base in range(21000, 21600, 30):
        try:
            prefix, P, c, logits = _fixed_point(cpu, pad, T - 35, base, T=T)
        except AssertionError:
            continue
        past = [int(x) for x in P[:, 0]]
        c_def, gap_def = rr.decide_ruled(cpu, logits, past, 30, True, DEFAULT, T)
        c_all, gap_all = rr.decide_ruled(cpu, logits, past, 30, True, SlotRules(rep_window=0), T)
        c_one, gap_one = rr.decide_ruled(cpu, logits, past, 30, True, SlotRules(rep_window=0, rep_penalty=1.0), T)
        assert (c_def, gap_def) == pr.decide(cpu, logits, past, 30, True) and c_one == c
        if c_def == c and c_all != c and min(gap_def, gap_all, gap_one) >= 2 * NEAR_TIE:
            return prefix, P, c, c_all
    return None


def _frame0(eng, prefix, P, rules, slot=1):
    eng.open(4, ignore_eos=True)
    eng.admit([slot], [prefix], [30], [SlotParams(max_frames=4)], prompts=[P], rules=[rules])
    assert eng.run(1) == 1
    codes, per = eng.codes()
    assert int(per[slot]) == 1
    return int(codes[0, slot, 0])


def test_window_0_penalises_an_id_older_than_the_ring(world, engines):
    cpu = world[3]
    ruled, _, pad = engines
    found = find_history_case(cpu, pad)
    assert found is not None, "no prompt whose whole history changes a clear frame-0 decision"
    prefix, P, c, c_all = found
    assert int(P[5, 0]) == c and (np.delete(P[:, 0], 5) != c).all()
    assert _frame0(ruled, prefix, P, DEFAULT) == c
    assert _frame0(ruled, prefix, P, SlotRules(rep_window=0)) == c_all
    assert _frame0(ruled, prefix, P, SlotRules(rep_window=0, rep_penalty=1.0)) == c       # seen, but not penalised


# ---- 3. no penalty ----------------------------------------------------------------------------------------------------------
def find_penalty_case(cpu, pad):
    T = 33
    for base in range(22000, 22600, 30):
        try:
            prefix, P, c, logits = _fixed_point(cpu, pad, T - 30, base, T=T)
        except AssertionError:
            continue
        past = [int(x) for x in P[:, 0]]
        c_def, gap_def = rr.decide_ruled(cpu, logits, past, 30, True, DEFAULT, T)
        c_one, gap_one = rr.decide_ruled(cpu, logits, past, 30, True, SlotRules(rep_penalty=1.0), T)
        if c_one == c and c_def != c and min(gap_def, gap_one) >= 2 * NEAR_TIE:
            return prefix, P, c, c_def
    return None


def test_penalty_1_lets_an_id_inside_the_window_win_again(world, engines):
    cpu = world[3]
    ruled, _, pad = engines
    found = find_penalty_case(cpu, pad)
    assert found is not None
    prefix, P, c, c_def = found
    assert _frame0(ruled, prefix, P, DEFAULT) == c_def != c
    assert _frame0(ruled, prefix, P, SlotRules(rep_penalty=1.0)) == c


# ---- 4. / 5. minimum length and the EOS rules ---------------------------------------------------------------------------------
def _run_counted(eng, prefix, P, n_text, budget, rules):
    eng.open(4)
    eng.admit([1], [prefix], [n_text], [SlotParams(max_frames=budget)], prompts=None if P is None else [P], rules=[rules])
    _finish(eng)
    done, per = eng.done()
    assert done[1]
    return _column(eng, 1)


MIN_CASE = (10, 4, 24)     # prompt frames, n_text, budget: in the style of test_eos_progress_counts_the_prompt


def find_min_frames_case(cpu, pad):
    """An input that ends by EOS at g frames under the default rules, without a near-tie anywhere, and without one under
    min_frames = g + 3 either."""
    T, n_text, budget = MIN_CASE
    for seed in range(23081, 23141):
        rng = np.random.default_rng(seed)
        (prefix,) = _prefixes(rng, [13])
        P = pr.random_prompt(rng, T)
        ref, margins = rr.generate_ruled(cpu, prefix, P, n_text, pad, budget, DEFAULT, want_margins=True)
        if min(min(m) for m in margins) < 2 * NEAR_TIE or not 1 <= len(ref) <= budget - 4:
            continue
        assert ref == pr.generate_prompted(cpu, prefix, P, n_text, pad, budget)
        ref2, margins2 = rr.generate_ruled(cpu, prefix, P, n_text, pad, budget, SlotRules(min_frames=len(ref) + 3), want_margins=True)
        if min(min(m) for m in margins2) >= 2 * NEAR_TIE:
            return prefix, P, ref, ref2
    return None


def test_min_frames_holds_eos_back(world, engines):
    cpu = world[3]
    ruled, _, pad = engines
    found = find_min_frames_case(cpu, pad)
    assert found is not None
    prefix, P, ref, ref2 = found
    T, n_text, budget = MIN_CASE
    g = len(ref)
    longer = SlotRules(min_frames=g + 3)
    print("frames by EOS:", g, "with min_frames", g + 3, ":", len(ref2))
    assert len(ref2) >= g + 3
    got = _run_counted(ruled, prefix, P, n_text, budget, DEFAULT)
    np.testing.assert_array_equal(got, np.asarray(ref).reshape(-1, 16))
    got2 = _run_counted(ruled, prefix, P, n_text, budget, longer)
    np.testing.assert_array_equal(got2, np.asarray(ref2).reshape(-1, 16))
    np.testing.assert_array_equal(got2[:g], got)             # the same stream until EOS would have come


def test_eos_rules_per_slot(world, engines):
    """progress = n_past / 6 here.  The default's boost and force end the utterance early (the force alone by n_past 13);
    with eos_boost 0 and eos_force 0 nothing length-based is left and it runs to its budget; with eos_force 1.0 (and no
    boost) EOS is forced at the first n_past above 6: 7 frames, an integer rule.  Counts are exact; the codes are graded as
    tests/test_gpu_engine.py grades a free-running stream (exact up to the first oracle near-tie)."""
    cpu = world[3]
    ruled, _, pad = engines
    n_text, budget = 2, 16
    (prefix,) = _prefixes(np.random.default_rng(907), [13])
    variants = {"default": (DEFAULT, lambda n: n <= 13), "off": (SlotRules(eos_boost=0.0, eos_force=0.0), lambda n: n == budget),
                "force 1.0": (SlotRules(eos_boost=0.0, eos_force=1.0), lambda n: n == 7)}
    for name, (ru, want) in variants.items():
        ref, margins = rr.generate_ruled(cpu, prefix, None, n_text, pad, budget, ru, want_margins=True)
        assert want(len(ref)), (name, len(ref))
        got = _run_counted(ruled, prefix, None, n_text, budget, ru)
        print(name, "frames", len(got), _compare(got[:, None, :], np.array([len(got)]), [ref], [margins]))
        assert len(got) == len(ref), name


# ---- 6. isolation, the seed contract, recycled slots --------------------------------------------------------------------------
RULE_SETS = [SlotRules(rep_penalty=1.05, rep_window=0, eos_boost=0.0, eos_force=0.0, min_frames=2),
             SlotRules(rep_penalty=3.0, rep_window=2, cp_top_p=0.5),
             SlotRules(rep_window=0, cp_top_p=0.9, min_frames=20),
             DEFAULT]


def test_slots_with_different_rules_equal_their_solo_runs(engines):
    ruled, _, pad = engines
    rng = np.random.default_rng(903)
    prefixes = _prefixes(rng, [12, 9, 17, 8])
    prompts = [None, pr.random_prompt(rng, 35), None, pr.random_prompt(rng, 3)]
    sps = [SlotParams(max_frames=F, seed=40 + b, utt=b, **SAMPLED) for b in range(4)]
    nt = [3, 30, 3, 3]                                       # (the 35 prompt frames of slot 1 are progress 35 / 90)
    solo = [_solo(ruled, prefixes[b], nt[b], sps[b], prompts[b], RULE_SETS[b], slot=(b + 1) % 4, ignore_eos=False) for b in range(4)]
    assert all(len(c) >= 1 for c in solo) and len(solo[2]) == F          # min_frames 20 > the budget: it runs to it
    ruled.open(4)
    ruled.admit([0, 1], prefixes[:2], nt[:2], sps[:2], prompts=prompts[:2], rules=RULE_SETS[:2])
    assert ruled.run(3) == 3
    ruled.admit([2, 3], prefixes[2:], nt[2:], sps[2:], prompts=prompts[2:], rules=RULE_SETS[2:])
    _finish(ruled)
    for b in range(4):
        np.testing.assert_array_equal(_column(ruled, b), solo[b], err_msg=f"slot {b}")
    assert len({c.tobytes() for c in solo}) == 4
    # the same seed, utt and rules in two slots: the same codes (cp_top_p under the seed contract)
    ruled.open(4)
    ruled.admit([0, 3], [prefixes[1]] * 2, [30, 30], [sps[1]] * 2, prompts=[prompts[1]] * 2, rules=[RULE_SETS[1]] * 2)
    _finish(ruled)
    np.testing.assert_array_equal(_column(ruled, 0), solo[1])
    np.testing.assert_array_equal(_column(ruled, 3), solo[1])
    # and the cut is part of what is drawn from
    other = _solo(ruled, prefixes[1], 30, sps[1], prompts[1], SlotRules(rep_penalty=3.0, rep_window=2), ignore_eos=False)
    assert not np.array_equal(other, solo[1])


def test_a_recycled_slot_inherits_neither_history_nor_rules(engines):
    ruled, plain, pad = engines
    rng = np.random.default_rng(904)
    a, b = _prefixes(rng, [12, 15])
    harsh = SlotRules(rep_penalty=3.0, rep_window=0, eos_boost=0.0, eos_force=0.0, cp_top_p=0.3)
    whole = SlotRules(rep_penalty=3.0, rep_window=0)
    sa, sb = SlotParams(max_frames=F, seed=1, **SAMPLED), SlotParams(max_frames=F, seed=2, **SAMPLED)
    fresh_whole = _solo(ruled, b, 30, sb, None, whole, slot=2)
    fresh_plain = _solo(plain, b, 30, sb, None, None, slot=2)
    # the first utterance's history is full of the id the second one starts with: an inherited set would divide its logit
    # by 3; inherited rules would cut the second one's code-predictor draws at 0.3
    PA = pr.random_prompt(rng, 40)
    PA[:, 0] = fresh_whole[0, 0]
    for rules, want in ((whole, fresh_whole), (None, fresh_plain)):
        ruled.open(4, ignore_eos=True)
        ruled.admit([2], [a], [30], [sa], prompts=[PA], rules=[harsh])
        _finish(ruled)
        assert _column(ruled, 2).shape == (F, 16)
        kw = {} if rules is None else dict(rules=[rules])
        ruled.admit([2], [b], [30], [sb], **kw)               # the same slot, no open() in between
        _finish(ruled)
        np.testing.assert_array_equal(_column(ruled, 2), want)


# ---- 7. the prefix cache --------------------------------------------------------------------------------------------------------
def test_a_cache_hit_gives_the_codes_of_the_miss_under_the_same_rules(world, engines):
    ruled, _, pad = engines
    rng = np.random.default_rng(905)
    (p,) = _prefixes(rng, [14])
    P = pr.random_prompt(rng, 40)
    ru = SlotRules(rep_penalty=1.5, rep_window=0, cp_top_p=0.7, min_frames=3)
    sp = SlotParams(max_frames=F, seed=9, **SAMPLED)
    key = bytes(range(16))
    ruled.prefix_cache(2, 64)
    try:
        out = []
        for want_hit in (False, True):
            ruled.open(4, ignore_eos=True)
            hit = ruled.admit([1], [p], [30], [sp], keys=[key], prompts=[P], rules=[ru])
            assert bool(hit[0]) == want_hit
            _finish(ruled)
            out.append(_column(ruled, 1))
        np.testing.assert_array_equal(out[0], out[1])
        assert out[0].shape == (F, 16)
    finally:
        ruled.prefix_cache(0)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def _raw_ruled(eng, slots, prefixes, n_text, params, rules):
    """q3e_admit_ruled without FrameEngine.admit's own checks; rules as (rep_penalty, rep_window, eos_boost, eos_force,
    min_frames, cp_top_p, reserved0, reserved1) per utterance."""
    slots = np.asarray(slots, np.int32)
    cat = np.ascontiguousarray(np.concatenate(prefixes, axis=0), dtype=np.float32)
    n_rows = np.array([p.shape[0] for p in prefixes], np.int32)
    nt = np.asarray(n_text, np.int32)
    arr = (hiplib.SlotParamsC * len(params))(*[hiplib.SlotParamsC(*p) for p in params])
    rarr = (hiplib.SlotRulesC * len(rules))(*[hiplib.SlotRulesC(*r[:6], (ctypes.c_int32 * 2)(*r[6:])) for r in rules])
    return eng._lib.q3e_admit_ruled(eng.h, len(slots), hiplib.iptr(slots), hiplib.fptr(cat), hiplib.iptr(n_rows), hiplib.iptr(nt),
                                    arr, None, None, None, None, rarr)


def test_refused_rules_change_nothing(engines):
    ruled, plain, pad = engines
    rng = np.random.default_rng(906)
    p, q = _prefixes(rng, [14, 11])
    g = (F, 0.0, 50, 1.0, 0.0, 50, 0, 0, 0)
    s = (F, 1.0, 50, 0.95, 1.0, 50, 99, 0, 0)
    ok = (1.05, 0, 0.0, 0.0, 2, 0.9, 0, 0)
    dflt = (1.2, 30, 15.0, 2.0, 0, 1.0, 0, 0)
    nan, inf = float("nan"), float("inf")
    ruled.open(4, ignore_eos=True)
    assert _raw_ruled(ruled, [0, 1], [p, p], [30, 30], [g, s], [ok, dflt]) == 0
    _finish(ruled)
    alone = [_column(ruled, 0), _column(ruled, 1)]
    ruled.open(4, ignore_eos=True)
    assert _raw_ruled(ruled, [0, 1], [p, p], [30, 30], [g, s], [ok, dflt]) == 0
    assert ruled.run(3) == 3
    bad = [(0.99, 30, 15.0, 2.0, 0, 1.0, 0, 0), (nan, 30, 15.0, 2.0, 0, 1.0, 0, 0), (inf, 30, 15.0, 2.0, 0, 1.0, 0, 0),
           (1.2, -1, 15.0, 2.0, 0, 1.0, 0, 0), (1.2, 31, 15.0, 2.0, 0, 1.0, 0, 0),
           (1.2, 30, -0.5, 2.0, 0, 1.0, 0, 0), (1.2, 30, nan, 2.0, 0, 1.0, 0, 0), (1.2, 30, inf, 2.0, 0, 1.0, 0, 0),
           (1.2, 30, 15.0, -1.0, 0, 1.0, 0, 0), (1.2, 30, 15.0, nan, 0, 1.0, 0, 0),
           (1.2, 30, 15.0, 2.0, -1, 1.0, 0, 0),
           (1.2, 30, 15.0, 2.0, 0, 0.0, 0, 0), (1.2, 30, 15.0, 2.0, 0, 1.5, 0, 0), (1.2, 30, 15.0, 2.0, 0, nan, 0, 0),
           (1.2, 30, 15.0, 2.0, 0, 1.0, 1, 0), (1.2, 30, 15.0, 2.0, 0, 1.0, 0, 7)]
    for r in bad:
        for rules in ([ok, r], [r, ok]):                     # whichever utterance carries it, neither is admitted
            assert _raw_ruled(ruled, [2, 3], [q, q], [30, 30], [g, g], rules) < 0, r
        done, per = ruled.done()
        assert [int(x) for x in per[:2]] == [3, 3] and not done[:2].any() and done[2:].all()
    with pytest.raises(ValueError):
        ruled.rules(False)                                    # a per-slot batch is open
    with pytest.raises(ValueError):
        ruled.rules(True)
    _finish(ruled)
    np.testing.assert_array_equal(_column(ruled, 0), alone[0])
    np.testing.assert_array_equal(_column(ruled, 1), alone[1])
    # rules without a reservation: refused, also default ones; the engine goes on as it was
    plain.open(4, ignore_eos=True)
    plain.admit([0], [p], [30], [SlotParams(max_frames=F)])
    assert plain.run(3) == 3
    assert _raw_ruled(plain, [2], [q], [30], [g], [dflt]) < 0
    done, per = plain.done()
    assert int(per[0]) == 3 and done[1:].all()
    _finish(plain)
    np.testing.assert_array_equal(_column(plain, 0), _solo(plain, p, 30, SlotParams(max_frames=F)))
    # FrameEngine.admit checks first
    ruled.open(4, ignore_eos=True)
    for kw in (dict(rep_penalty=0.5), dict(rep_window=31), dict(rep_window=1.5), dict(eos_boost=-1), dict(eos_force=nan),
               dict(min_frames=-1), dict(cp_top_p=0.0), dict(cp_top_p=True)):
        with pytest.raises(ValueError):
            ruled.admit([0], [p], [30], [SlotParams(max_frames=F)], rules=[SlotRules(**kw)])
    done, per = ruled.done()
    assert done.all()
