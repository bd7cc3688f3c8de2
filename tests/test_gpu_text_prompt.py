"""Text slots that continue a codec prompt (q3e_slot_params.reserved == 3), on the tiny synthetic pack: the prompt is an
ordinary prompted slot's, pushed row i rides on GENERATED frame i, and hold, stall and EOS count generated frames.

References: an ordinary prompted slot (pad rows: array equality), the CPU helper tests/text_prompt_ref.py
(tests/test_gpu_engine.py's _compare and NEAR_TIE; the first two frames of a case chosen clear on the CPU exactly), the
same utterance alone, and a hold-off engine given every row at admission (array equality)."""
import numpy as np
import pytest

from oracle.pipeline import CpuPipeline
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from tests import prompt_ref as pr
from tests import text_prompt_ref as tpr
from tests.test_gpu_codec_prompt import _raw
from tests.test_gpu_concurrent import SAMPLED
from tests.test_gpu_engine import NEAR_TIE, _compare, _prefixes
from tests.util import synthetic_pack

pytestmark = pytest.mark.gpu

N_CTX = 128
B17 = 17
CAP = 24            # frames and text rows per slot


def _rows(rng, n):
    return (0.05 * rng.standard_normal((n, 1024))).astype(np.float32)


def _text(max_frames, **kw):
    return SlotParams(max_frames=max_frames, text_stream=True, text_after_prompt=True, **kw)


def _column(eng, b):
    codes, per = eng.codes()
    return np.ascontiguousarray(codes[:int(per[b]), b, :])


def _finish(eng):
    while eng.run(8) > 0:
        pass


def _frames(eng, slots):
    done, per = eng.done()
    return [int(per[b]) for b in slots], [bool(done[b]) for b in slots]


@pytest.fixture(scope="module")
def tworld():
    path, cfg, tensors = synthetic_pack(2, 2)
    return path, cfg, tensors, CpuPipeline(cfg, tensors, n_ctx=N_CTX)


@pytest.fixture(scope="module")
def tengines(gpu_lib, tworld):
    """(hold on, hold off with a prefix cache, no reservation with a prefix cache): 17 slots, one pad row for all."""
    path = tworld[0]
    pad = _rows(np.random.default_rng(800), 1)[0]
    out = []
    for reserve, hold, cache in ((CAP, True, False), (CAP, False, True), (0, False, True)):
        eng = FrameEngine(path, max_batch=B17, n_ctx=N_CTX, max_frames=CAP)
        eng.set_pad_embed(pad)
        if reserve:
            eng.reserve_text(reserve)
        if hold:
            eng.hold_text()
        if cache:
            eng.prefix_cache(4, N_CTX)
        out.append(eng)
    yield out[0], out[1], out[2], pad
    for eng in out:
        eng.destroy()


def _admit(eng, B, utts, ignore_eos=True):
    """utts: {slot: (prefix, SlotParams, text rows or None, prompt or None)} -> an open batch, nothing pushed."""
    eng.open(B, ignore_eos=ignore_eos)
    for b, (p, sp, rows, P) in utts.items():
        eng.admit([b], [p], [0 if rows is not None else 30], [sp], prompts=[P])


def _reference(off, B, utts):
    """Hold off, every row at admission -> {slot: codes}."""
    _admit(off, B, utts)
    for b, (p, sp, rows, P) in utts.items():
        if rows is not None:
            off.push_text(b, rows, final=True, n_text=len(rows))
    _finish(off)
    return {b: _column(off, b) for b in utts}


# ---- 1. pad rows: the ordinary prompted slot's bits ---------------------------------------------------------------------------

@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("slot", [0, 16])
@pytest.mark.parametrize("n_rows,T", [(8, 1), (8, 33), (9, 60)])
def test_pad_rows_give_the_ordinary_prompted_slots_bits(tengines, n_rows, T, slot, sampled):
    _, eng, _, pad = tengines
    rng = np.random.default_rng(8100 + 100 * n_rows + T)
    (prefix,) = _prefixes(rng, [n_rows])
    q0, q1 = _prefixes(rng, [11, 16])
    P = pr.random_prompt(rng, T)
    F = 10
    kw = dict(seed=41, **SAMPLED) if sampled else {}
    other = [SlotParams(max_frames=CAP, seed=s, **SAMPLED) for s in (1, 2)]

    def run(text):
        eng.open(B17, ignore_eos=True)
        if slot == 16:                                       # the second 16-row tile, beside running neighbours
            eng.admit([3, 15], [q0, q1], [30, 30], other)
            assert eng.run(2) == 2
        S = _text(F, **kw) if text else SlotParams(max_frames=F, **kw)
        eng.admit([slot], [prefix], [30], [S], prompts=[P])
        if text:
            eng.push_text(slot, np.repeat(pad[None], F, axis=0))
        _finish(eng)
        return _column(eng, slot)

    want, got = run(False), run(True)
    assert want.shape == (F, 16) and (want >= 0).all()
    np.testing.assert_array_equal(got, want)


# ---- 2. trajectory against the CPU helper, with real text rows -----------------------------------------------------------------

F2 = 8
CASES = [(8, 9, 8), (8, 33, 5), (9, 60, 8)]     # (n_rows, T, text rows): the middle one has pad rows behind its text


def _clear_text_case(cpu, n_rows, T, n_text_rows, pad, base_seed, tries=40):
    """As tests/test_gpu_codec_prompt.py's _clear_case, with text rows: inputs, drawn on the CPU, whose first two generated
    frames hold no oracle decision closer than 2 * NEAR_TIE; those 32 decisions are then compared exactly."""
    for seed in range(base_seed, base_seed + tries):
        rng = np.random.default_rng(seed)
        (prefix,) = _prefixes(rng, [n_rows])
        P = pr.random_prompt(rng, T)
        rows = _rows(rng, n_text_rows)
        ref, margins = tpr.generate_text_prompted(cpu, prefix, P, rows, 30, pad, F2, ignore_eos=True, want_margins=True)
        if len(ref) == F2 and min(min(m) for m in margins[:2]) >= 2 * NEAR_TIE:
            return prefix, P, rows, ref, margins
    raise AssertionError(f"no seed in {base_seed}..{base_seed + tries} gives two clear first frames")


@pytest.mark.parametrize("n_rows,T,n_text_rows", CASES)
def test_generated_frames_match_the_cpu_helper(tworld, tengines, n_rows, T, n_text_rows):
    path, cfg, tensors, cpu = tworld
    _, eng, _, pad = tengines
    prefix, P, rows, ref, margins = _clear_text_case(cpu, n_rows, T, n_text_rows, pad, 8200 + 100 * n_rows + T)
    assert min(min(m) for m in margins[:2]) >= 2 * NEAR_TIE            # (on CPU values)
    # the check has something to see: with pad rows for the text the CPU's own frames differ
    assert pr.generate_prompted(cpu, prefix, P, 30, pad, F2, ignore_eos=True) != ref
    eng.open(4, ignore_eos=True)
    eng.admit([2], [prefix], [0], [_text(F2)], prompts=[P])
    eng.push_text(2, rows, final=True, n_text=30)
    assert eng.run(F2) == F2
    codes, per = eng.codes()
    assert int(per[2]) == F2
    stats = _compare(codes[:, 2:3], per[2:3], [ref], [margins])
    print(f"({n_rows}, {T}, {n_text_rows}):", stats)
    np.testing.assert_array_equal(codes[:2, 2], np.asarray(ref[:2]))   # the 32 clear decisions, exactly


# ---- 3. every slot its own T ---------------------------------------------------------------------------------------------------

def test_every_slot_counts_its_own_prompt(tengines):
    _, eng, _, pad = tengines
    rng = np.random.default_rng(8301)
    pa, pb, pc, pd = _prefixes(rng, [8, 8, 11, 13])
    PA, PC = pr.random_prompt(rng, 9), pr.random_prompt(rng, 33)
    F = 12
    utts = {0: (pa, _text(F, seed=3, **SAMPLED), _rows(rng, 10), PA),
            1: (pb, SlotParams(max_frames=F, text_stream=True), _rows(rng, 7), None),
            2: (pc, SlotParams(max_frames=F, seed=4, **SAMPLED), None, PC),
            3: (pd, SlotParams(max_frames=F), None, None)}
    together = _reference(eng, 4, utts)
    for b, u in utts.items():
        alone = _reference(eng, 4, {b: u})[b]
        assert alone.shape == (F, 16)
        np.testing.assert_array_equal(together[b], alone, err_msg=f"slot {b}")
    # (the prompt and the text are part of what is decoded: without either the prompted text slot gives other codes)
    assert not np.array_equal(_reference(eng, 4, {0: (pa, utts[0][1], utts[0][2], None)})[0], together[0])
    assert not np.array_equal(_reference(eng, 4, {0: (pa, utts[0][1], utts[0][2][:0], PA)})[0], together[0])


# ---- 4. hold ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slot,beside,T", [(0, 16, 33), (16, 3, 9)])
def test_hold_counts_generated_frames(tengines, slot, beside, T):
    on, off, _, pad = tengines
    rng = np.random.default_rng(8400 + T)
    p, q = _prefixes(rng, [8, 14])
    P = pr.random_prompt(rng, T)
    rows = _rows(rng, 9)
    F = 14
    utts = {slot: (p, _text(F, seed=77, **SAMPLED), rows, P),
            beside: (q, SlotParams(max_frames=CAP, seed=5, **SAMPLED), None, None)}
    ref = _reference(off, B17, utts)
    assert ref[slot].shape == (F, 16)
    # held after its first generated frame (g = 1) for 1 step, in the middle for 2, just before its last row for 9
    _admit(on, B17, utts)
    on.push_text(slot, rows[:1])
    for k, (n_steps, push) in enumerate([(1, None), (1, rows[1:4]), (3, None), (2, rows[4:8]), (4, None), (9, None)]):
        for _ in range(n_steps):
            assert on.run(1) == 1, k
        if k == 0:
            assert _frames(on, [slot, beside])[0] == [1, 1] and int(on.held_steps()[slot]) == 0
        if push is not None:
            on.push_text(slot, push)
    assert _frames(on, [slot, beside])[0] == [8, 20]
    assert int(on.held_steps()[slot]) == 12 and int(on.held_steps()[beside]) == 0
    on.push_text(slot, rows[8:], final=True, n_text=9)
    _finish(on)
    for b in utts:
        np.testing.assert_array_equal(_column(on, b), ref[b], err_msg=f"slot {b}")
    # one run over unheld and held steps
    _admit(on, B17, utts)
    on.push_text(slot, rows[:3])
    assert on.run(8) == 8
    assert _frames(on, [slot, beside])[0] == [3, 8]
    assert int(on.held_steps()[slot]) == 5
    on.push_text(slot, rows[3:], final=True, n_text=9)
    _finish(on)
    for b in utts:
        np.testing.assert_array_equal(_column(on, b), ref[b], err_msg=f"slot {b}")


@pytest.mark.parametrize("k", [1, 5])
def test_a_held_step_is_a_no_op_for_the_prompted_row(tengines, k):
    on, off, _, pad = tengines
    rng = np.random.default_rng(8450)
    p, q = _prefixes(rng, [9, 12])
    P = pr.random_prompt(rng, 33)
    rows = _rows(rng, 8)
    utts = {0: (q, SlotParams(max_frames=CAP), None, None), 1: (p, _text(14, seed=9, **SAMPLED), rows, P)}
    _admit(on, 4, utts)
    on.push_text(1, rows[:4])
    assert on.run(4) == 4
    hid, col, other = on.hidden()[1].copy(), _column(on, 1), on.hidden()[0].copy()
    assert col.shape == (4, 16) and int(on.held_steps()[1]) == 0
    assert on.run(k) == k
    np.testing.assert_array_equal(on.hidden()[1], hid)       # bit for bit
    assert not np.array_equal(on.hidden()[0], other)         # (the ordinary row did step)
    np.testing.assert_array_equal(_column(on, 1), col)
    codes, per = on.codes()
    assert int(per[1]) == 4 and int(per[0]) == 4 + k
    assert (codes[4:, 1, :] == -1).all()                     # nothing recorded past the row's last frame
    assert int(on.held_steps()[1]) == k
    on.push_text(1, rows[4:], final=True, n_text=8)
    _finish(on)
    ref = _reference(off, 4, utts)
    np.testing.assert_array_equal(_column(on, 1), ref[1])
    np.testing.assert_array_equal(_column(on, 0), ref[0])


def test_a_prompted_slot_without_a_frame_and_a_row_stalls_the_batch(tengines):
    on, off, _, pad = tengines
    rng = np.random.default_rng(8460)
    p, q = _prefixes(rng, [8, 11])
    P = pr.random_prompt(rng, 9)
    rows = _rows(rng, 6)
    F = 12
    T, O = _text(F), SlotParams(max_frames=F)
    # alone: its T prompt frames are no frame of its own to repeat
    _admit(on, 4, {1: (p, T, rows, P)})
    assert on.run(8) == 0
    assert list(on.text_state()[1]) == [False, True, False, False]
    assert not on.held_steps().any()
    # beside a live ordinary slot
    utts = {0: (q, O, None, None), 1: (p, T, rows, P)}
    ref = _reference(off, 4, utts)
    _admit(on, 4, utts)
    assert on.run(8) == 0
    assert list(on.text_state()[1]) == [False, True, False, False]
    assert _frames(on, [0, 1])[0] == [0, 0]
    on.push_text(1, rows[:1])                                # one row releases it: a step of its own, then it is held
    assert on.run(8) == 8
    assert _frames(on, [0, 1])[0] == [8, 1]
    assert int(on.held_steps()[1]) == 7
    on.push_text(1, rows[1:], final=True, n_text=6)
    _finish(on)
    np.testing.assert_array_equal(_column(on, 0), ref[0])
    np.testing.assert_array_equal(_column(on, 1), ref[1])
    # hold off: the same slot stalls the batch at every frame it has no row for
    _admit(off, 4, utts)
    assert off.run(8) == 0
    off.push_text(1, rows[:2])
    assert off.run(8) == 2
    assert list(off.text_state()[1]) == [False, True, False, False]
    off.push_text(1, rows[2:], final=True, n_text=6)
    _finish(off)
    np.testing.assert_array_equal(_column(off, 1), ref[1])


# ---- 5. EOS ------------------------------------------------------------------------------------------------------------------

T5, NTEXT5, BUDGET5 = 10, 4, 24


def _eos_case(cpu, pad, base_seed, open_frames, tries=40):
    """Inputs without a near-tie anywhere, so that the frame count itself is graded.  Progress is (T + g) / (3 * n_text) =
    (10 + g) / 12: above 2 -- g >= 15 -- EOS is forced, inside the budget of 24."""
    for seed in range(base_seed, base_seed + tries):
        rng = np.random.default_rng(seed)
        (prefix,) = _prefixes(rng, [13])
        P = pr.random_prompt(rng, T5)
        rows = _rows(rng, NTEXT5)
        ref, margins = tpr.generate_text_prompted(cpu, prefix, P, rows, NTEXT5, pad, BUDGET5, want_margins=True,
                                                  mask_eos_until=open_frames)
        if min(min(m) for m in margins) >= 2 * NEAR_TIE:
            return prefix, P, rows, ref, margins
    raise AssertionError("no input without a near-tie")


@pytest.mark.parametrize("open_frames", [0, 3])
def test_eos_rules_see_the_prompt_after_the_final_push(tworld, tengines, open_frames):
    path, cfg, tensors, cpu = tworld
    _, eng, _, pad = tengines
    prefix, P, rows, ref, margins = _eos_case(cpu, pad, {0: 8500, 3: 8685}[open_frames], open_frames)
    assert open_frames <= len(ref) <= BUDGET5 - T5 + 1 and len(margins) == len(ref) + 1      # it ended by EOS, inside the budget
    # the rules count the prompt: the same rows under a progress that starts at 0 run longer
    blind = tpr.generate_text_prompted(cpu, prefix, P, rows, NTEXT5, pad, BUDGET5, past=[], mask_eos_until=open_frames)
    print("frames with / without the prompt in the progress:", len(ref), len(blind))
    assert len(ref) < len(blind)
    eng.open(4)
    eng.admit([1], [prefix], [0], [_text(BUDGET5)], prompts=[P])
    if open_frames:                                           # its text stays open for the first frames: EOS masked, n_text 0
        eng.push_text(1, rows[:open_frames])
        assert eng.run(8) == open_frames
        eng.push_text(1, rows[open_frames:], final=True, n_text=NTEXT5)
    else:
        eng.push_text(1, rows, final=True, n_text=NTEXT5)
    _finish(eng)
    done, _ = eng.done()
    assert done[1]
    codes, per = eng.codes()
    print(_compare(codes[:, 1:2], per[1:2], [ref], [margins]))
    assert int(per[1]) == len(ref)
    np.testing.assert_array_equal(codes[:len(ref), 1], np.asarray(ref).reshape(-1, 16))


# ---- 6. prefix cache -----------------------------------------------------------------------------------------------------------

def test_a_keyed_admission_is_a_miss_then_a_hit_with_the_same_codes(tengines):
    _, eng, _, pad = tengines
    rng = np.random.default_rng(8601)
    (p,) = _prefixes(rng, [9])
    P = pr.random_prompt(rng, 33)
    rows = _rows(rng, 8)
    F = 10
    S = _text(F, seed=6, **SAMPLED)
    key = bytes(range(100, 116))
    eng.prefix_cache(4, N_CTX)                               # (drops every entry; the counters run on)
    before = eng.prefix_stats()
    out = []
    for want_hit in (False, True):
        eng.open(4, ignore_eos=True)
        hit = eng.admit([2], [p if not want_hit else np.zeros_like(p)], [0], [S], keys=[key], prompts=[P])
        assert bool(hit[0]) == want_hit
        eng.push_text(2, rows, final=True, n_text=8)
        _finish(eng)
        out.append(_column(eng, 2))
    assert out[0].shape == (F, 16)
    np.testing.assert_array_equal(out[1], out[0])
    after = eng.prefix_stats()
    assert [after[k] - before[k] for k in ("misses", "stores", "hits")] == [1, 1, 1]


# ---- 7. T = 0 and refusals -----------------------------------------------------------------------------------------------------

def test_without_prompt_frames_it_is_a_text_slot(tengines):
    _, eng, _, pad = tengines
    rng = np.random.default_rng(8701)
    p, q = _prefixes(rng, [8, 12])
    rows = _rows(rng, 7)
    F = 10
    out = []
    for S, P in ((SlotParams(max_frames=F, text_stream=True, seed=8, **SAMPLED), None), (_text(F, seed=8, **SAMPLED), None),
                 (_text(F, seed=8, **SAMPLED), np.zeros((0, 16), np.int32))):
        utts = {0: (q, SlotParams(max_frames=F), None, None), 1: (p, S, rows, P)}
        out.append(_reference(eng, 4, utts))
    assert out[0][1].shape == (F, 16)
    for other in out[1:]:
        np.testing.assert_array_equal(other[0], out[0][0])
        np.testing.assert_array_equal(other[1], out[0][1])


def test_refusals_change_nothing(tengines):
    _, eng, plain, pad = tengines
    rng = np.random.default_rng(8702)
    p, q = _prefixes(rng, [14, 11])
    ok = pr.random_prompt(rng, 20)
    Fr = 12
    g = (Fr, 0.0, 50, 1.0, 0.0, 50, 0, 0, 0)
    key = [bytes(range(16)), bytes(range(16, 32))]
    with pytest.raises(ValueError):
        SlotParams(max_frames=Fr, text_after_prompt=True).check(CAP)       # the bit needs a text slot
    for e, bad_calls in ((eng, [g[:8] + (2,)]), (plain, [g[:8] + (2,), g[:8] + (3,)])):
        e.open(4, ignore_eos=True)
        assert _raw(e, [0], [p], [30], [g], prompts=[ok], keys=key[:1]) == 0
        _finish(e)
        alone = _column(e, 0)
        assert alone.shape == (Fr, 16)
        e.open(4, ignore_eos=True)
        assert _raw(e, [0], [p], [30], [g], prompts=[ok], keys=key[:1]) == 0
        assert e.run(3) == 3
        stats = e.prefix_stats()
        for bad in bad_calls:
            for prompts in ([ok[:0], ok], [ok[:0], ok[:0]]):                # with a prompt and without
                assert _raw(e, [2, 3], [q, q], [30, 30], [g, bad], prompts=prompts, keys=key) < 0
                done, per = e.done()
                assert [int(x) for x in per[:1]] == [3] and not done[0] and done[1:].all()
                assert e.prefix_stats() == stats
        _finish(e)
        np.testing.assert_array_equal(_column(e, 0), alone)
    # reserved == 1 with a prompt stays refused on an engine with a reservation, == 3 is taken
    eng.open(4, ignore_eos=True)
    assert _raw(eng, [1], [q], [0], [g[:8] + (1,)], prompts=[ok]) < 0
    assert _raw(eng, [1], [q], [0], [g[:8] + (3,)], prompts=[ok]) == 0
    eng.push_text(1, _rows(rng, 3), final=True, n_text=3)
    assert eng.run(100) == Fr
    assert _column(eng, 1).shape == (Fr, 16)
