"""Codec prompts of the per-slot admissions (q3e_admit_prompted) on the tiny synthetic pack: the prompt's rows and the slot
state against q3e_admit given the same rows from the host (array equality, no tolerance), the generated frames against
the CPU reference of tests/prompt_ref.py (tests/test_gpu_engine.py's _compare and its NEAR_TIE), the sampler's view of the
prompt (ring, window, progress), budgets, draw keys and the validation.

Shapes (n_rows, T): one prompt row; the 30-entry window; the 32-entry ring wrapping; 64 and 65 rows in all (the prefill's
GEMV-to-GEMM switch); more than four 16-row attention tiles."""
import ctypes

import numpy as np
import pytest

from oracle.pipeline import CpuPipeline
from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from tests import prompt_ref as pr
from tests.test_gpu_concurrent import SAMPLED
from tests.test_gpu_engine import NEAR_TIE, _compare, _prefixes
from tests.util import synthetic_pack

pytestmark = pytest.mark.gpu

SHAPES = [(12, 1), (9, 30), (9, 33), (31, 33), (32, 33), (20, 60)]
N_CTX = 128
F = 8


@pytest.fixture(scope="module")
def world():
    path, cfg, tensors = synthetic_pack(2, 2)
    return path, cfg, tensors, CpuPipeline(cfg, tensors, n_ctx=N_CTX)


def _engine(path, pad, cache=None):
    eng = FrameEngine(path, max_batch=4, n_ctx=N_CTX, max_frames=24)
    eng.set_pad_embed(pad)
    if cache:
        eng.prefix_cache(*cache)
    return eng


def _pad(rng):
    return (0.05 * rng.standard_normal(1024)).astype(np.float32)


def _finish(eng):
    while eng.run(8) > 0:
        pass


def _column(eng, b):
    codes, per = eng.codes()
    return np.ascontiguousarray(codes[:int(per[b]), b, :])


@pytest.fixture(scope="module")
def engines(gpu_lib, world):
    """Two engines with one pad row, shared by the tests that only need `an engine`: every test opens its own batch."""
    path = world[0]
    pad = _pad(np.random.default_rng(700))
    a, b = _engine(path, pad), _engine(path, pad)
    yield a, b, pad
    a.destroy()
    b.destroy()


# ---- 1. rows and state, exact ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rows,T", SHAPES)
def test_prompt_rows_and_frame0_state_are_those_of_a_plain_prefix(world, engines, n_rows, T):
    path, cfg, tensors, cpu = world
    eng, plain, pad = engines
    rng = np.random.default_rng(7000 + 100 * n_rows + T)
    (prefix,) = _prefixes(rng, [n_rows])
    n0, n1, n2 = _prefixes(rng, [11, 16, 21])
    P = pr.random_prompt(rng, T)
    G = SlotParams(max_frames=F)
    full = pr.prompted_prefix(cpu, prefix, P, pad)
    assert full.shape == (n_rows + T, 1024)
    plain.open(4, ignore_eos=True)
    plain.admit([0], [full], [30], [G])
    want = plain.hidden()[0].copy()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    # alone in slot 0
    eng.open(4, ignore_eos=True)
    eng.admit([0], [prefix], [30], [G], prompts=[P])
    np.testing.assert_array_equal(eng.hidden()[0], want)
    # in slot 3 beside three running neighbours
    eng.open(4, ignore_eos=True)
    eng.admit([0, 1, 2], [n0, n1, n2], [30] * 3, [SlotParams(max_frames=20)] * 3)
    assert eng.run(3) == 3
    eng.admit([3], [prefix], [30], [G], prompts=[P])
    np.testing.assert_array_equal(eng.hidden()[3], want)
    done, per = eng.done()
    assert int(per[3]) == 0 and not done[3]              # nothing generated yet: the prompt is not counted


# ---- 2. trajectory against the oracle ---------------------------------------------------------------------------------------

def _clear_case(cpu, n_rows, T, pad, base_seed, n_text=30, tries=40):
    """Inputs, drawn on the CPU, whose first two generated frames hold no oracle decision closer than 2 * NEAR_TIE: those
    32 decisions are then compared exactly, the near-tie allowance of _compare cannot cover them."""
    for seed in range(base_seed, base_seed + tries):
        rng = np.random.default_rng(seed)
        (prefix,) = _prefixes(rng, [n_rows])
        P = pr.random_prompt(rng, T)
        ref, margins = pr.generate_prompted(cpu, prefix, P, n_text, pad, F, ignore_eos=True, want_margins=True)
        if len(ref) == F and min(min(m) for m in margins[:2]) >= 2 * NEAR_TIE:
            return prefix, P, ref, margins
    raise AssertionError(f"no seed in {base_seed}..{base_seed + tries} gives two clear first frames")


@pytest.mark.parametrize("n_rows,T", SHAPES)
def test_generated_frames_match_the_cpu_reference(world, engines, n_rows, T):
    path, cfg, tensors, cpu = world
    eng, _, pad = engines
    prefix, P, ref, margins = _clear_case(cpu, n_rows, T, pad, 9000 + 100 * n_rows + T)
    assert min(min(m) for m in margins[:2]) >= 2 * NEAR_TIE            # (on CPU values)
    eng.open(4, ignore_eos=True)
    eng.admit([2], [prefix], [30], [SlotParams(max_frames=F)], prompts=[P])
    assert eng.run(F) == F
    codes, per = eng.codes()
    assert int(per[2]) == F
    stats = _compare(codes[:, 2:3], per[2:3], [ref], [margins])
    print(f"({n_rows}, {T}):", stats)
    np.testing.assert_array_equal(codes[:2, 2], np.asarray(ref[:2]))   # the 32 clear decisions, exactly


# ---- 3. the ring is what the sampler reads ----------------------------------------------------------------------------------

def _fixed_point(cpu, pad, at, base_seed, n_rows=9, T=33, tries=30):
    """A prompt whose frame-0 arg-max under an EMPTY history, c, stands at P[at][0] (and nowhere else in column 0):
    iterate prefill -> c -> P[at][0] = c until c is stable.  -> (prefix, P, c, raw frame-0 logits)."""
    for seed in range(base_seed, base_seed + tries):
        rng = np.random.default_rng(seed)
        (prefix,) = _prefixes(rng, [n_rows])
        P = pr.random_prompt(rng, T)
        for _ in range(6):
            logits = pr.frame0_logits(cpu, prefix, P, pad)
            c, _ = pr.decide(cpu, logits, [], 30, True)
            if int(P[at, 0]) == c:
                if (np.delete(P[:, 0], at) != c).all():
                    return prefix, P, c, logits
                break
            P[at, 0] = c
    raise AssertionError("no stable prompt found")


def _device_frame0(eng, prefix, P, slot=1):
    eng.open(4, ignore_eos=True)
    eng.admit([slot], [prefix], [30], [SlotParams(max_frames=F)], prompts=[P])
    assert eng.run(1) == 1
    codes, per = eng.codes()
    assert int(per[slot]) == 1
    return int(codes[0, slot, 0])


def test_an_id_inside_the_window_is_penalised(world, engines):
    path, cfg, tensors, cpu = world
    eng, _, pad = engines
    T = 33
    found = None
    for base in range(11000, 11400, 30):
        prefix, P, c, logits = _fixed_point(cpu, pad, T - 30, base)
        c_empty, gap_empty = pr.decide(cpu, logits, [], 30, True)
        c_seeded, gap_seeded = pr.decide(cpu, logits, [int(x) for x in P[:, 0]], 30, True)
        if c_seeded != c_empty and gap_empty >= 2 * NEAR_TIE and gap_seeded >= 2 * NEAR_TIE:
            found = (prefix, P, c_empty, c_seeded)
            break
    assert found is not None, "no prompt whose history changes a clear frame-0 decision"
    prefix, P, c_empty, c_seeded = found
    assert c_empty == int(P[T - 30, 0]) and c_seeded != c_empty
    assert _device_frame0(eng, prefix, P) == c_seeded


def test_an_id_just_outside_the_window_is_not(world, engines):
    path, cfg, tensors, cpu = world
    eng, _, pad = engines
    T = 33
    found = None
    for base in range(12000, 12400, 30):
        prefix, P, c, logits = _fixed_point(cpu, pad, T - 31, base)     # in the ring of 32, not among the last 30
        c_seeded, gap_seeded = pr.decide(cpu, logits, [int(x) for x in P[:, 0]], 30, True)
        c_pen, _ = pr.decide(cpu, logits, [c], 30, True)                 # what a sampler that penalised it would pick
        if c_seeded == c and c_pen != c and gap_seeded >= 2 * NEAR_TIE:
            found = (prefix, P, c)
            break
    assert found is not None
    prefix, P, c = found
    assert _device_frame0(eng, prefix, P) == c


# ---- 4. progress counts the prompt ------------------------------------------------------------------------------------------

def test_eos_progress_counts_the_prompt(world, engines):
    path, cfg, tensors, cpu = world
    eng, _, pad = engines
    T, n_text, budget = 10, 4, 24
    for seed in range(13001, 13041):   # inputs without a near-tie anywhere, so that the frame count itself is graded
        rng = np.random.default_rng(seed)
        (prefix,) = _prefixes(rng, [13])
        P = pr.random_prompt(rng, T)
        ref, margins = pr.generate_prompted(cpu, prefix, P, n_text, pad, budget, want_margins=True)
        if min(min(m) for m in margins) >= 2 * NEAR_TIE:
            break
    assert min(min(m) for m in margins) >= 2 * NEAR_TIE
    # the boost rises with progress = n_past / 12 from the first generated frame on, and above 2 -- n_past = T + generated
    # > 24 -- EOS is forced: at most 15 frames.  The same rows with an empty history run longer.
    assert len(ref) <= 24 - T + 1 and len(margins) == len(ref) + 1
    unprompted = cpu.generate(pr.prompted_prefix(cpu, prefix, P, pad), n_text, pad, budget)
    print("frames with / without the prompt in the progress:", len(ref), len(unprompted))
    assert len(ref) < len(unprompted)
    eng.open(4)
    eng.admit([1], [prefix], [n_text], [SlotParams(max_frames=budget)], prompts=[P])
    _finish(eng)
    done, _ = eng.done()
    assert done[1]
    codes, per = eng.codes()
    print(_compare(codes[:, 1:2], per[1:2], [ref], [margins]))
    assert int(per[1]) == len(ref)


# ---- 5. budget, positions, independence -------------------------------------------------------------------------------------

def test_the_budget_counts_generated_frames(world, engines):
    path, cfg, tensors, cpu = world
    eng, _, pad = engines
    rng = np.random.default_rng(14001)
    (prefix,) = _prefixes(rng, [10])
    P = pr.random_prompt(rng, 33)
    eng.open(4, ignore_eos=True)
    eng.admit([2], [prefix], [30], [SlotParams(max_frames=5)], prompts=[P])
    for k in range(1, 6):
        assert eng.run(1) == 1
        done, per = eng.done()
        assert int(per[2]) == k and bool(done[2]) == (k >= 5)
    assert eng.run(8) == 0
    # a longer-lived neighbour makes the codes array longer than the prompted column
    eng.open(4, ignore_eos=True)
    eng.admit([0, 2], [prefix, prefix], [30, 30], [SlotParams(max_frames=9), SlotParams(max_frames=5)], prompts=[None, P])
    _finish(eng)
    codes, per = eng.codes()
    done, per2 = eng.done()
    assert done.all() and [int(per[0]), int(per[2])] == [9, 5] and int(per2[2]) == 5
    assert codes.shape[0] == 9
    assert ((codes[:5, 2] >= 0) & (codes[:5, 2] < 2048)).all()
    assert (codes[5:, 2, 0] == -1).all() and int(codes[5, 2, 0]) == -1
    ref, margins = pr.generate_prompted(cpu, prefix, P, 30, pad, 5, ignore_eos=True, want_margins=True)
    print(_compare(codes[:, 2:3], per[2:3], [ref], [margins]))


def test_draws_and_neighbours_are_independent_of_a_prompted_admission(world, engines):
    path, cfg, tensors, cpu = world
    eng, _, pad = engines
    rng = np.random.default_rng(15001)
    p, q0, q1 = _prefixes(rng, [14, 11, 16])
    P, Q = pr.random_prompt(rng, 33), pr.random_prompt(rng, 7)
    Fs = 12
    S = SlotParams(max_frames=Fs, seed=1234, **SAMPLED)
    other = [SlotParams(max_frames=Fs, seed=s, **SAMPLED) for s in (1, 2, 3)]
    # alone in slot 0
    eng.open(4, ignore_eos=True)
    eng.admit([0], [p], [30], [S], prompts=[P])
    _finish(eng)
    alone = _column(eng, 0)
    assert alone.shape == (Fs, 16)
    # the unprompted neighbour without any prompted admission
    eng.open(4, ignore_eos=True)
    eng.admit([1], [q0], [30], [other[0]])
    _finish(eng)
    neighbour = _column(eng, 1)
    # slot 3, after earlier admissions, beside a prompted and an unprompted utterance
    eng.open(4, ignore_eos=True)
    eng.admit([1, 2], [q0, q1], [30, 30], [other[0], other[1]], prompts=[None, Q])
    assert eng.run(4) == 4
    eng.admit([3], [p], [30], [S], prompts=[P])
    _finish(eng)
    np.testing.assert_array_equal(_column(eng, 3), alone)
    np.testing.assert_array_equal(_column(eng, 1), neighbour)
    # the prompt is part of what is drawn from: the same seed without it gives other codes
    eng.open(4, ignore_eos=True)
    eng.admit([0], [p], [30], [S])
    _finish(eng)
    assert not np.array_equal(_column(eng, 0), alone)


# ---- 6. validation ----------------------------------------------------------------------------------------------------------

def _raw(eng, slots, prefixes, n_text, params, prompts=None, frames=None, keys=None):
    """q3e_admit_prompted / q3e_admit_keyed without FrameEngine.admit's own checks; params as (max_frames, temperature,
    top_k, top_p, cp_temperature, cp_top_k, seed, utt, reserved).  prompts: one [T][16] array per utterance or None =
    q3e_admit_keyed; frames: the prompt_frames array (default: the prompts' lengths; "null": NULL)."""
    slots = np.asarray(slots, np.int32)
    cat = np.ascontiguousarray(np.concatenate(prefixes, axis=0), dtype=np.float32)
    n_rows = np.array([p.shape[0] for p in prefixes], np.int32)
    nt = np.asarray(n_text, np.int32)
    arr = (hiplib.SlotParamsC * len(params))(*[hiplib.SlotParamsC(*p) for p in params])
    kptr = None
    if keys is not None:
        kk = np.stack([np.frombuffer(k, "<u8") for k in keys]).astype(np.uint64)
        kptr = kk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    head = (eng.h, len(slots), hiplib.iptr(slots), hiplib.fptr(cat), hiplib.iptr(n_rows), hiplib.iptr(nt), arr, kptr, None)
    if prompts is None:
        return eng._lib.q3e_admit_keyed(*head)
    pcat = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32).reshape(-1, 16) for x in prompts] +
                                               [np.zeros((1, 16), np.int32)], axis=0))
    if isinstance(frames, str):
        return eng._lib.q3e_admit_prompted(*head, hiplib.iptr(pcat), None)
    fr = np.asarray([len(x) for x in prompts] if frames is None else frames, np.int32)
    return eng._lib.q3e_admit_prompted(*head, hiplib.iptr(pcat), hiplib.iptr(fr))


def test_refused_prompts_change_nothing(world, engines):
    path, cfg, tensors, cpu = world
    eng, _, pad = engines
    rng = np.random.default_rng(16001)
    p, q = _prefixes(rng, [14, 11])
    Fr = 12
    g = (Fr, 0.0, 50, 1.0, 0.0, 50, 0, 0, 0)
    s = (Fr, 1.0, 50, 0.95, 1.0, 50, 99, 0, 0)
    ok = pr.random_prompt(rng, 20)
    eng.reserve_text(16)                                 # so that the text-slot case is refused for its prompt alone
    try:
        eng.open(4, ignore_eos=True)                     # what the two running utterances decode undisturbed
        assert _raw(eng, [0, 1], [p, p], [30, 30], [g, s], prompts=[ok, ok[:0]]) == 0
        _finish(eng)
        alone = [_column(eng, 0), _column(eng, 1)]
        assert alone[0].shape == (Fr, 16)
        eng.open(4, ignore_eos=True)
        assert _raw(eng, [0, 1], [p, p], [30, 30], [g, s], prompts=[ok, ok[:0]]) == 0
        assert eng.run(3) == 3
        too_long = pr.random_prompt(rng, N_CTX - 11 - Fr + 1)            # 11 + T + 12 = n_ctx + 1
        fits = pr.random_prompt(rng, N_CTX - 11 - Fr)
        bad0, bad7 = ok.copy(), ok.copy()
        bad0[13, 0] = 2048
        bad7[19, 7] = -1
        bad_calls = [
            ([2, 3], [q, q], [g, g], [ok, too_long]),
            ([2, 3], [q, q], [g, g], [ok, bad0]),
            ([2, 3], [q, q], [g, g], [bad7, ok]),
            ([2, 3], [q, q], [g, g[:8] + (1,)], [ok[:0], ok]),           # a prompt on a text slot
        ]
        for slots, prefixes, params, prompts in bad_calls:
            assert _raw(eng, slots, prefixes, [30, 30], params, prompts=prompts) < 0
            done, per = eng.done()
            assert [int(x) for x in per[:2]] == [3, 3] and not done[:2].any() and done[2:].all()
        _finish(eng)
        np.testing.assert_array_equal(_column(eng, 0), alone[0])
        np.testing.assert_array_equal(_column(eng, 1), alone[1])
        # the longest prompt that fits is taken
        eng.open(4, ignore_eos=True)
        assert _raw(eng, [2], [q], [30], [g], prompts=[fits]) == 0
        assert eng.run(100) == Fr
        assert _column(eng, 2).shape == (Fr, 16)
    finally:
        eng.reserve_text(0)


def test_without_prompt_frames_it_is_admit_keyed(world, engines):
    path, cfg, tensors, cpu = world
    eng, _, pad = engines
    rng = np.random.default_rng(17001)
    p, q = _prefixes(rng, [14, 19])
    Fr = 10
    params = [(Fr, 0.0, 50, 1.0, 0.0, 50, 0, 0, 0), (Fr, 1.0, 50, 0.95, 1.0, 50, 5, 1, 0)]
    junk = [pr.random_prompt(rng, 3), pr.random_prompt(rng, 4)]          # never read: no frames say so
    out = []
    for kw in (dict(prompts=None), dict(prompts=junk, frames="null"), dict(prompts=junk, frames=[0, 0])):
        eng.open(4, ignore_eos=True)
        assert _raw(eng, [1, 3], [p, q], [30, 30], params, **kw) == 0
        hid0 = eng.hidden().copy()
        _finish(eng)
        codes, per = eng.codes()
        out.append((hid0, codes.copy(), per.copy(), eng.hidden().copy()))
    assert [int(x) for x in out[0][2][[1, 3]]] == [Fr, Fr]
    for other in out[1:]:
        for a, b in zip(out[0], other):
            np.testing.assert_array_equal(a, b)
