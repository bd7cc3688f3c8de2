"""Per-decision log-probabilities in the engine (q3e_scores_reserve / q3e_get_scores, FrameEngine.scores / score) on the tiny
synthetic pack: B = 3, n_ctx 96, 12 frames.

  * the codes of an engine with the reservation are bit for bit those of one without, in every mode;
  * teacher-forced with the oracle's ids, every one of the 12 x 3 x 16 scores is within NEAR_TIE of the float64 log-softmax
    of the oracle's own logits.  Why that bound: |d lp| <= |d z_u| + |d lse| <= 2 * max|d z|, and tests/test_gpu_engine.py
    asserts max|d z| < 2.5e-3 = NEAR_TIE / 2 -- measured there on the full-depth talker head only; the observed maximum per
    group is printed here;
  * score() is the manual start / force / run sequence; the per-slot seed contract and the prefix cache hold for the scores
    as they do for the codes; ended rows and frames past an utterance's count read 0.0; no reservation, no scores."""
import numpy as np
import pytest

from oracle import frontend as fe
from oracle import oracle as orc
from oracle.pipeline import CpuPipeline
from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams, SlotRules
from tests import prompt_ref as pr
from tests import score_ref as R
from tests.test_gpu_concurrent import SAMPLED
from tests.test_gpu_engine import NEAR_TIE, _prefixes
from tests.util import synthetic_pack

pytestmark = pytest.mark.gpu

B, N_CTX, F = 3, 96, 12


@pytest.fixture(scope="module")
def world():
    path, cfg, tensors = synthetic_pack(2, 2)
    return path, cfg, tensors, CpuPipeline(cfg, tensors, n_ctx=N_CTX)


def _engine(path, pad, scores, rules=True, text=F, cache=0):
    eng = FrameEngine(path, max_batch=B, n_ctx=N_CTX, max_frames=F)
    eng.set_pad_embed(pad)
    if text:
        eng.reserve_text(text)
    if rules:
        eng.rules()
    if cache:
        eng.prefix_cache(cache, 32)
    if scores:
        eng.scores_reserve()
    return eng


@pytest.fixture(scope="module")
def engines(gpu_lib, world):
    """(an engine with the scores reserved, one without), one pad row for both."""
    pad = (0.05 * np.random.default_rng(1200).standard_normal(1024)).astype(np.float32)
    scored, plain = _engine(world[0], pad, True), _engine(world[0], pad, False)
    yield scored, plain, pad
    scored.destroy()
    plain.destroy()


def _finish(eng):
    while eng.run(8) > 0:
        pass


# ---- the codes do not change ------------------------------------------------------------------------------------------------
def _start_run(eng, sampled):
    rng = np.random.default_rng(1201)
    prefixes = _prefixes(rng, [12, 21, 17])
    eng.set_sampling(seed=77, **({"talker_temperature": 0.9, "talker_top_k": 50, "talker_top_p": 0.95, "cp_temperature": 0.9,
                                  "cp_top_k": 50} if sampled else {}))
    eng.start(prefixes, [30, 2, 8], ignore_eos=False, max_frames=F)
    eng.run(F)
    return eng.codes()


def _slot_scenario(eng):
    """One ruled, one prompted and one text slot in a per-slot batch -> (codes, per)."""
    rng = np.random.default_rng(1202)
    p0, p1, p2 = _prefixes(rng, [12, 9, 8])
    P = pr.random_prompt(rng, 9)
    rows = (0.05 * rng.standard_normal((10, 1024))).astype(np.float32)
    sps = [SlotParams(max_frames=F, seed=5, **SAMPLED), SlotParams(max_frames=F, seed=6, utt=1, **SAMPLED),
           SlotParams(max_frames=10, text_stream=True, seed=7, **SAMPLED)]
    eng.open(B)
    eng.admit([0, 1, 2], [p0, p1, p2], [30, 30, 0], sps, prompts=[None, P, None],
              rules=[SlotRules(rep_penalty=1.05, rep_window=0, cp_top_p=0.8), None, None])
    eng.push_text(2, rows[:3])
    eng.run(6)
    eng.push_text(2, rows[3:], final=True, n_text=10)
    _finish(eng)
    return eng.codes()


@pytest.mark.parametrize("mode", ["start_greedy", "start_sampled", "slots"])
def test_codes_are_identical_with_and_without_the_reservation(engines, mode):
    scored, plain, pad = engines
    run = _slot_scenario if mode == "slots" else (lambda e: _start_run(e, mode == "start_sampled"))
    want, per = run(plain)
    got, per2 = run(scored)
    assert want.shape[0] > 0 and (per > 0).all()
    np.testing.assert_array_equal(per2, per)
    np.testing.assert_array_equal(got, want)
    sc, per3 = scored.scores()
    np.testing.assert_array_equal(per3, per)
    assert sc.shape == got.shape and sc.dtype == np.float32
    # every recorded decision has a finite log-probability <= 0 on this model; everything else reads 0.0
    live = (got[:, :, 0] >= 0) & (np.arange(got.shape[0])[:, None] < per[None, :])
    assert live.any() and np.isfinite(sc).all()
    assert (sc[live] < 0).all() and (sc[~live] == 0.0).all()
    if mode != "slots":   # the EOS boost ended utterance 1 early: its later frames are the masked ones
        assert per[1] < F and not live[int(per[1]):, 1].any()
    for e in (scored, plain):
        e.set_sampling()


# ---- teacher-forced against the oracle ----------------------------------------------------------------------------------------
def oracle_scores(cpu, cfg, prefix, n_text, pad, n_frames):
    """The oracle's greedy ids under ignore_eos (CpuPipeline.generate's loop) and the float64 log-softmax of the oracle's own
    logits at each of them -> (frames [n][16] int, lp [n][16] float64)."""
    audio_vocab, eos = cfg.cp_vocab, cfg.codec_eos
    cpu.talker.clear()
    hidden = cpu.talker.forward(prefix, 0)
    pos, past, frames, lps = prefix.shape[0], [], [], []
    for _ in range(n_frames):
        logits = cpu.talker.logits(hidden)
        lg, _ = fe.process_talker_logits(logits, past, n_text, eos)
        lg[eos] = -1e10
        code0 = int(np.argmax(lg))
        codes, _, hid = cpu.cp.predict(hidden, code0, want_hidden=True)
        lp = [R.talker_log_prob(logits, code0, audio_vocab, eos)]
        for g in range(cfg.cp_groups):
            lp.append(R.log_prob(orc.head_logits(cpu.cp.heads[g], hid[g]), int(codes[g])))
        frames.append([code0] + [int(c) for c in codes])
        lps.append(lp)
        past.append(code0)
        hidden = cpu.talker.forward(fe.feedback_embedding(code0, codes, cpu.codec_embedding, cpu.cp_emb, pad), pos)
        pos += 1
    return np.array(frames, np.int32), np.array(lps, np.float64)


@pytest.fixture(scope="module")
def forced_case(world, engines):
    path, cfg, tensors, cpu = world
    pad = engines[2]
    rng = np.random.default_rng(1203)
    prefixes = _prefixes(rng, [12, 21, 17])
    n_text = [30, 12, 40]
    ids, lps = zip(*[oracle_scores(cpu, cfg, prefixes[b], n_text[b], pad, F) for b in range(B)])
    for b in range(B):
        ref = cpu.generate(prefixes[b], n_text[b], pad, F, ignore_eos=True)
        assert ids[b].tolist() == ref
    forced = np.ascontiguousarray(np.stack(ids, axis=1))      # [F][B][16]
    return prefixes, n_text, forced, np.stack(lps, axis=1)


def _manual(eng, prefixes, n_text, forced):
    eng.start(prefixes, n_text, ignore_eos=True, max_frames=F)
    eng.set_forced_codes(forced)
    assert eng.run(F) == F
    return eng.scores()


def test_teacher_forced_scores_match_the_oracle(engines, forced_case):
    scored, plain, pad = engines
    prefixes, n_text, forced, want = forced_case
    got, per = _manual(scored, prefixes, n_text, forced)
    assert got.shape == (F, B, 16) and (per == F).all()
    err = np.abs(got.astype(np.float64) - want)
    print("teacher-forced |device - oracle| log-probability, maximum per group:",
          " ".join(f"{g}:{err[:, :, g].max():.2e}" for g in range(16)))
    print(f"overall {err.max():.3e} (bound NEAR_TIE = {NEAR_TIE}); log-probabilities span {want.min():.2f} .. {want.max():.2f}")
    assert np.isfinite(got).all()
    assert (err < NEAR_TIE).all(), f"{(err >= NEAR_TIE).sum()} of {err.size} scores differ by NEAR_TIE or more, worst {err.max():.3e}"
    # the same run is the same bits
    again, _ = _manual(scored, prefixes, n_text, forced)
    assert again.tobytes() == got.tobytes()


def test_score_is_the_manual_sequence(engines, forced_case):
    scored, plain, pad = engines
    prefixes, n_text, forced, _ = forced_case
    want, _ = _manual(scored, prefixes, n_text, forced)
    got = scored.score(prefixes, n_text, forced)
    assert got.shape == (F, B, 16) and got.tobytes() == want.tobytes()
    # a shorter list of frames scores its own frames the same
    short = scored.score(prefixes, n_text, forced[:5])
    assert short.shape == (5, B, 16) and short.tobytes() == want[:5].tobytes()
    with pytest.raises(RuntimeError):
        plain.score(prefixes, n_text, forced)


# ---- per-slot contracts -------------------------------------------------------------------------------------------------------
def test_per_slot_seed_contract_holds_for_scores(engines):
    """One sampled utterance alone in slot 0, and in slot 2 beside two others after an earlier admission: the same codes
    and the same scores."""
    scored, plain, pad = engines
    rng = np.random.default_rng(1204)
    p, q, r = _prefixes(rng, [14, 9, 19])
    sp = SlotParams(max_frames=F, seed=41, utt=2, **SAMPLED)
    scored.open(B, ignore_eos=True)
    scored.admit([0], [p], [30], [sp])
    _finish(scored)
    codes, per = scored.codes()
    sc, _ = scored.scores()
    n = int(per[0])
    assert n == F
    scored.open(B, ignore_eos=True)
    scored.admit([0, 1], [q, r], [30, 30], [SlotParams(max_frames=F, seed=1, **SAMPLED), SlotParams(max_frames=5, seed=2, **SAMPLED)])
    scored.run(3)
    scored.admit([2], [p], [30], [sp])
    _finish(scored)
    codes2, per2 = scored.codes()
    sc2, _ = scored.scores()
    assert int(per2[2]) == n
    np.testing.assert_array_equal(codes2[:n, 2], codes[:n, 0])
    assert sc2[:n, 2].tobytes() == sc[:n, 0].tobytes() and (sc[:n, 0] < 0).all()
    # slot 1 used its budget of 5: the frames past its count read 0.0 although the batch went on
    assert int(per2[1]) == 5 and (sc2[5:, 1] == 0.0).all() and (sc2[:5, 1] < 0).all()


def test_prefix_cache_hit_gives_the_scores_of_the_miss(gpu_lib, world):
    pad = (0.05 * np.random.default_rng(1205).standard_normal(1024)).astype(np.float32)
    eng = _engine(world[0], pad, True, cache=2)
    try:
        rng = np.random.default_rng(1206)
        p, = _prefixes(rng, [15])
        sp = SlotParams(max_frames=F, seed=9, **SAMPLED)
        out = []
        for slot, want_hit in ((1, False), (2, True)):
            eng.open(B, ignore_eos=True)
            hit = eng.admit([slot], [p if not want_hit else np.zeros_like(p)], [30], [sp], keys=[bytes([7]) * 16])
            assert bool(hit[0]) == want_hit
            _finish(eng)
            codes, per = eng.codes()
            sc, _ = eng.scores()
            assert int(per[slot]) == F
            out.append((codes[:, slot].copy(), sc[:, slot].copy()))
        np.testing.assert_array_equal(out[1][0], out[0][0])
        assert out[1][1].tobytes() == out[0][1].tobytes() and (out[0][1] < 0).all()
    finally:
        eng.destroy()


# ---- the reservation ----------------------------------------------------------------------------------------------------------
def test_no_reservation_no_scores(engines):
    scored, plain, pad = engines
    rng = np.random.default_rng(1207)
    prefixes = _prefixes(rng, [10, 11, 12])
    plain.start(prefixes, [30] * 3, ignore_eos=True, max_frames=4)
    plain.run(4)
    out = np.zeros((F, B, 16), np.float32)
    per = np.zeros(B, np.int32)
    assert plain._lib.q3e_get_scores(plain.h, hiplib.fptr(out), F, hiplib.iptr(per)) < 0
    with pytest.raises(RuntimeError):
        plain.scores()
    # refused while a per-slot batch is open, like q3e_rules_reserve; nothing changes
    scored.open(B)
    with pytest.raises(ValueError):
        scored.scores_reserve(False)
    with pytest.raises(ValueError):
        scored.scores_reserve(True)
    scored.start(prefixes, [30] * 3, ignore_eos=True, max_frames=4)
    scored.run(4)
    assert scored.scores()[0].shape == (4, B, 16)
    # releasing and reserving again between batches works, and the frame is captured again
    scored.scores_reserve(False)
    with pytest.raises(RuntimeError):
        scored.scores()
    scored.scores_reserve(True)
    scored.start(prefixes, [30] * 3, ignore_eos=True, max_frames=4)
    scored.run(4)
    sc, per = scored.scores()
    assert (per == 4).all() and (sc < 0).all()
