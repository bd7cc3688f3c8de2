"""One engine walked through every kind of change to what its captured frame has baked in (include/qwen3tts_engine.h:
q3e_set_sampling, q3e_scores_reserve, q3e_set_forced_codes, q3e_text_reserve, q3e_text_hold, q3e_rules_reserve, fixed batch
<-> per-slot batch), with a run after each.  q3e_run captures again exactly when the state it would launch with differs
from the one its graphs hold (csrc/q3_engine.hip: FrameState); a change that is missed replays kernels with the old
arguments.  At every step the walked engine's codes -- and scores, where reserved -- are the bits of a FRESH engine that
only ever saw that step's configuration.  Tiny synthetic pack, B = 3, n_ctx 96, 12 frames; every comparison is exact."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams, SlotRules
from tests.test_gpu_engine import _prefixes
from tests.util import synthetic_pack

pytestmark = pytest.mark.gpu

B, F = 3, 12
GREEDY = dict()
STOCHASTIC = dict(talker_temperature=0.9, talker_top_k=40, talker_top_p=0.9, cp_temperature=0.8, cp_top_k=30, seed=1234)
SAMPLED = dict(temperature=1.0, top_k=50, top_p=0.95, cp_temperature=1.0, cp_top_k=50)
RULED = SlotRules(rep_penalty=1.5, rep_window=0, eos_boost=5.0, eos_force=1.5, min_frames=3, cp_top_p=0.8)

_rng = np.random.default_rng(500)
PREFIXES = _prefixes(_rng, [8, 13, 10])
N_TEXT = [30, 30, 30]
PAD = (0.05 * _rng.standard_normal(1024)).astype(np.float32)
TEXT_ROWS = (0.05 * _rng.standard_normal((8, 1024))).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _configure(eng, scores=False, text=0, hold=False, rules=False):
    """The whole reservation state of a step, from whatever the engine had; leaves a per-slot batch first (q3e_start does),
    since every reservation refuses an open one."""
    eng.start(PREFIXES, N_TEXT, ignore_eos=True, max_frames=F)
    eng.scores_reserve(scores)
    eng.reserve_text(text)
    if text:
        eng.hold_text(hold)
    eng.rules(rules)


def _fixed(eng, sampling, **reserved):
    """A fixed batch of F frames under set_sampling(**sampling) -> codes."""
    _configure(eng, **reserved)
    eng.set_sampling(**sampling)
    eng.start(PREFIXES, N_TEXT, ignore_eos=True, max_frames=F)
    assert eng.run(F) == F
    codes, per = eng.codes()
    assert codes.shape == (F, B, 16) and list(per) == [F] * B
    return codes


def _fixed_twice(eng, sampling):
    """... and the same set_sampling call again with identical values: the same request, the same codes."""
    first = _fixed(eng, sampling)
    nodes = eng.graph_nodes
    again = _fixed(eng, sampling)
    np.testing.assert_array_equal(again, first)
    assert eng.graph_nodes == nodes > 0
    return first


def _forced(eng, forced):
    """scores_reserve(True) and a teacher-forced run of `forced` -> (the decisions recorded, the scores)."""
    _configure(eng, scores=True)
    eng.set_sampling(**STOCHASTIC)
    scores = eng.score(PREFIXES, N_TEXT, forced)
    codes, per = eng.codes()
    assert scores.shape == codes.shape == (F, B, 16)
    return codes, scores


def _slots(eng, text, hold=False, rules=False, starve=0):
    """A per-slot batch under a reservation of `text` rows: a text slot (with rules: a ruled one) and two plain slots, the
    text slot given `text` rows; with starve, only 2 of them before `starve` steps of the others -> (codes, frames per slot)."""
    _configure(eng, text=text, hold=hold, rules=rules)
    eng.open(B, ignore_eos=True)
    params = [SlotParams(max_frames=F, text_stream=True, seed=11, **SAMPLED), SlotParams(max_frames=F, seed=12, utt=1, **SAMPLED),
              SlotParams(max_frames=F - 3)]
    eng.admit([0, 1, 2], PREFIXES, [0, 30, 30], params, rules=[RULED, None, None] if rules else None)
    rows = TEXT_ROWS[:text]
    if starve:
        eng.push_text(0, rows[:2])
        assert eng.run(2 + starve) == 2 + starve             # slot 0 is held after its 2 rows, the others step on
        assert int(eng.held_steps()[0]) == starve
        eng.push_text(0, rows[2:], final=True, n_text=text)
    else:
        eng.push_text(0, rows, final=True, n_text=text)
    while eng.run(8) > 0:
        pass
    codes, per = eng.codes()
    assert list(per) == [F, F, F - 3]
    eng.release([0, 1, 2])
    return codes, per


def _engine(path):
    eng = FrameEngine(path, max_batch=B, n_ctx=96, max_frames=F)
    eng.set_pad_embed(PAD)
    return eng


STEPS = ["1 fixed batch, greedy", "2 set_sampling, stochastic, twice", "3 scores_reserve(True), teacher-forced",
         "4 scores_reserve(False)", "5 reserve_text(4), per-slot batch", "6 reserve_text(8), per-slot batch",
         "7 hold_text(True), a starved slot", "8 rules(True), a ruled slot", "9 back to the fixed batch, greedy"]


@pytest.fixture(scope="module")
def walk(gpu_lib):
    """{step: (what the walked engine gave, what a fresh engine gave)}, each a tuple of arrays."""
    path, cfg, tensors = synthetic_pack(2, 2)
    greedy = {}

    def forced(eng):
        return _forced(eng, greedy["codes"])

    steps = [lambda e: (_fixed(e, GREEDY),), lambda e: (_fixed_twice(e, STOCHASTIC),), forced, lambda e: (_fixed(e, STOCHASTIC),),
             lambda e: _slots(e, 4), lambda e: _slots(e, 8), lambda e: _slots(e, 8, hold=True, starve=3),
             lambda e: _slots(e, 8, rules=True), lambda e: (_fixed(e, GREEDY),)]
    out = {}
    eng = _engine(path)
    for name, step in zip(STEPS, steps):
        got = step(eng)
        if not greedy:
            greedy["codes"] = got[0]
        fresh = _engine(path)
        out[name] = (got, step(fresh))
        fresh.destroy()
    with pytest.raises(RuntimeError):
        eng.scores()                                         # (released in step 4, and since)
    eng.destroy()
    return out


@pytest.mark.parametrize("step", STEPS)
def test_a_reconfigured_engine_gives_a_fresh_engines_bits(walk, step):
    got, want = walk[step]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=step)


def test_the_steps_differ_from_each_other(walk):
    """(the settings took effect: a walk whose steps all gave one answer would pass the comparison above for nothing)"""
    c = {k: walk[k][0][0] for k in STEPS}
    assert not np.array_equal(c[STEPS[0]], c[STEPS[1]])      # greedy / stochastic
    assert not np.array_equal(c[STEPS[4]], c[STEPS[5]])      # 4 text rows / 8
    assert not np.array_equal(c[STEPS[5]][:, 0], c[STEPS[7]][:, 0])   # the text slot without / with its rules
    np.testing.assert_array_equal(c[STEPS[5]], c[STEPS[6]])  # a held step changes nothing: hold on = hold off
    np.testing.assert_array_equal(c[STEPS[8]], c[STEPS[0]])
    assert np.isfinite(walk[STEPS[2]][0][1]).all() and (walk[STEPS[2]][0][1] < 0).any()
