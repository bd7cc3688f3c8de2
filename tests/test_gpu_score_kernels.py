"""The score of an emitted id, at the kernels: talker_sample_kernel*_scores and cp_argmax_kernel*_scores through the hooks
q3t_talker_score_case / q3t_cp_score_case against tests/score_ref.py (float64).

Inputs are the seeded launches of tests/sample_cases.py -- every family, the degenerate ones included; scalar, per-slot and
per-slot-with-rules launches; greedy and stochastic rows side by side; rows before and after the launch -- plus the held rows
of its text cases.  Every launch runs twice on the device, through the non-score hook and through the score hook, with the
same draw, and:

  1. every piece of state (codes, ring, counters, seen-sets, held flags, gathered rows) is bit for bit the same;
  2. a score is written exactly where a code is written (the buffer starts as a sentinel), so never for a row outside the
     launch, an ended or held talker row, a held code-predictor row or a frame beyond the codes array;
  3. each written score matches the reference within 1e-5 + 1e-6 * |ref|, NaN and +-inf exactly;
  4. a teacher-forced id scores the forced id (one >= audio_vocab / >= V among them: -inf);
  5. a held code-predictor row keeps the score its frame recorded.

The bound of 3, for the reductions as built (fp32, u = 2^-24 ~ 6e-8):
  talker  per thread an online (max, sum) pair over <= 12 logits: each step is one expf (<= 2 ulp), one multiply or add and
          one add, <= 12 * 4 u serial; the wave merge rescales once (expf, multiply) and adds in 6 butterfly stages; the 4
          waves rescale once more and add serially: <= (48 + 9 + 7) u < 4e-6 relative on the sum, the same absolute on its
          log.  logf adds <= 2 ulp of log s <= ln 3072 ~ 8 (1e-6), z_u - m and the final subtraction one rounding each of
          a value of the size of |ref| (6e-8 * |ref| each).  Total < 5.2e-6 + 1.2e-7 * |ref|.
  cp      per thread <= 8 (16 at V = 4096) expf + add, 6 stages, 3 adds: <= (16 * 3 + 9) u < 3.5e-6, then as above.
Both are inside 1e-5 + 1e-6 * |ref|; the largest observed error is printed per vocabulary."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import sample_cases as SC
from tests import sample_ref as SR
from tests import score_ref as R
from tests.test_gpu_sample_decisions import U64P, _opt, _slots_array
from tests.test_gpu_sample_rules import U32P, _rules_array

pytestmark = pytest.mark.gpu

SENT = np.float32(-12345.5)     # "no score was written here"
RECORDED = np.float32(-0.625)   # the score a held row's frame holds from the step that recorded its id
MODES = ("scalar", "slots", "rules")
RULES = (dict(rep_penalty=1.2, rep_window=30, eos_boost=15.0, eos_force=2.0, min_past=0, cp_top_p=1.0),
         dict(rep_penalty=1.05, rep_window=0, eos_boost=0.0, eos_force=0.0, min_past=2, cp_top_p=0.8),
         dict(rep_penalty=1.0, rep_window=7, eos_boost=4.0, eos_force=1.5, min_past=0, cp_top_p=0.5))


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), f"{what}: the score launch left other bits than the launch without scores"


def _check_scores(scores, written, ref_of, worst):
    """scores [F][RT][16] after the launch; written: {(f, r, col): id used}; every other entry must be the sentinel."""
    mask = np.zeros(scores.shape, bool)
    for (f, r, c), u in written.items():
        mask[f, r, c] = True
        got, ref = scores[f, r, c], ref_of(r, u)
        assert got.tobytes() != SENT.tobytes(), f"no score at frame {f} row {r} column {c} where a code was written"
        ok, err = R.matches(got, ref)
        assert ok, f"frame {f} row {r} column {c} id {u}: device {got!r}, reference {ref!r} (error {err:.3e})"
        worst[0] = max(worst[0], err)
        worst[1] += 1
    keep = scores[~mask]
    assert (keep.view(np.uint32) == SENT.view(np.uint32)).all(), "a score was written where no code was"


# ---- talker ---------------------------------------------------------------------------------------------------------
def run_talker(lib, logits, st, cfg, scores):
    """One launch through q3t_talker_sample_rules_case (scores None) or q3t_talker_score_case -> (rc, state after)."""
    out = SR.copy_state(st)
    RT = logits.shape[0]
    logits = np.ascontiguousarray(logits, np.float32)
    forced, ta, seed_ptr = cfg.get("forced"), cfg.get("text_avail"), cfg.get("seed_ptr")
    ta = None if ta is None else np.ascontiguousarray(ta, np.int32)
    keep, slots = _slots_array(cfg.get("slots"))
    keep2, rules = _rules_array(cfg.get("rules"))
    seen = out.get("seen")
    args = [hiplib.fptr(logits), logits.shape[1], RT, cfg["row0"], cfg["R"], hiplib.iptr(out["past"]), hiplib.iptr(out["n_past"]),
            hiplib.iptr(out["n_text"]), hiplib.iptr(out["done"]), hiplib.iptr(out["n_frames"]), hiplib.iptr(out["pos0"]),
            hiplib.iptr(out["pos"]), hiplib.iptr(out["codes"]), cfg["frame_cap"], _opt(forced, hiplib.iptr),
            cfg["audio_vocab"], cfg["eos"], int(cfg.get("ignore_eos", False)), cfg.get("max_frames", 0),
            cfg.get("rep_penalty", 1.2), cfg.get("temperature", 0.0), cfg.get("top_k", 50), cfg.get("top_p", 0.95),
            cfg.get("seed", 0), None if seed_ptr is None else seed_ptr.ctypes.data_as(U64P), slots, _opt(ta, hiplib.iptr),
            _opt(out.get("held"), hiplib.iptr), rules, None if seen is None else seen.ctypes.data_as(U32P)]
    if scores is None:
        return lib.q3t_talker_sample_rules_case(*args), out
    return lib.q3t_talker_score_case(*args, hiplib.fptr(scores)), out


def _talker_cases(V, mode):
    audio_vocab, eos = SC.TALKER_VOCABS[V]
    cases = SC.talker_decision_cases(V, mode != "scalar")
    if mode != "scalar" and V in SC.TEXT_TALKER_VOCABS:
        cases += SC.text_talker_cases(V)          # held rows, masked EOS
    out = []
    for ci, case in enumerate(cases):
        cfg, st = dict(case["cfg"]), SR.copy_state(case["st"])
        RT, row0, Rn = cfg["R_total"], cfg["row0"], cfg["R"]
        rng = SC.rng_for("score_talker", V, mode, ci)
        if mode == "rules":
            cfg["rules"] = [RULES[int(rng.integers(3))] for _ in range(RT)]
            words = (audio_vocab + 31) // 32
            st["seen"] = rng.integers(0, 2 ** 32, (RT, words), dtype=np.uint64).astype(np.uint32) & np.uint32(0x11111111)
        # teacher forcing on every third row of the launch: an audio id, EOS, or an id outside the allowed set; one row
        # outside the launch too (nothing may come of it)
        forced = np.full((cfg["frame_cap"], RT, 16), -1, np.int32)
        for i in range(0, Rn, 3):
            pick = (int(rng.integers(audio_vocab)), eos, audio_vocab + (1 if audio_vocab + 1 != eos else 2), int(rng.integers(audio_vocab)))
            forced[:, row0 + i, 0] = pick[(i // 3) % 4]
        forced[:, 0, 0] = 1
        cfg["forced"] = forced
        out.append(dict(logits=case["logits"], st=st, cfg=cfg))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V", [64, 3072])
def test_talker_scores(test_lib, V, mode):
    audio_vocab, eos = SC.TALKER_VOCABS[V]
    worst, kinds = [0.0, 0], dict(nan=0, ninf=0, forced=0, outside=0)
    for case in _talker_cases(V, mode):
        logits, st, cfg = case["logits"], case["st"], case["cfg"]
        rc0, plain = run_talker(test_lib, logits, st, cfg, None)
        scores = np.full((cfg["frame_cap"], cfg["R_total"], 16), SENT, np.float32)
        rc1, dev = run_talker(test_lib, logits, st, cfg, scores)
        assert rc0 == 0 and rc1 == 0, (rc0, rc1)
        for k in plain:                                                              # 1
            _same_bits(dev[k], plain[k], k)
        written = {}
        for r in range(cfg["row0"], cfg["row0"] + cfg["R"]):
            f = int(st["n_frames"][r])
            if f >= cfg["frame_cap"] or dev["n_past"][r] == st["n_past"][r]:        # not recorded / ended or held: no id
                continue
            code = int(dev["codes"][f, r, 0])
            assert code >= 0
            fz = int(cfg["forced"][f, r, 0])
            written[(f, r, 0)] = fz if fz >= 0 else code                            # 4
            kinds["forced"] += fz >= 0
            kinds["outside"] += fz >= audio_vocab and fz != eos
            assert int(dev["past"][r, st["n_past"][r] & 31]) == written[(f, r, 0)]   # the id the stream continues with
        _check_scores(scores, written, lambda r, u: R.talker_log_prob(logits[r], u, audio_vocab, eos), worst)   # 2, 3
        vals = np.array([scores[k] for k in written])
        kinds["nan"] += int(np.isnan(vals).sum())
        kinds["ninf"] += int(np.isneginf(vals).sum())
    print(f"talker V={V} {mode}: {worst[1]} scores, largest error {worst[0]:.3e}; {kinds}")
    assert worst[1] > 100 and all(v > 0 for v in kinds.values()), kinds


def test_talker_score_ignores_the_sampler(test_lib):
    """One row of logits under sampler settings that change the decision -- temperature, top-k / top-p, the repetition
    penalty, ignore_eos, the EOS boost of a long utterance, per-slot rules: the forced id scores the same bits."""
    V, (audio_vocab, eos) = 3072, SC.TALKER_VOCABS[3072]
    rng = SC.rng_for("score_invariance")
    RT = 4
    logits = (6.0 * rng.standard_normal((RT, V))).astype(np.float32)
    base = SC.talker_state(rng, RT, V, audio_vocab)
    base["n_frames"][:] = 0
    forced = np.full((SC.FRAME_CAP, RT, 16), -1, np.int32)
    forced[0, :, 0] = [5, 2047, eos, 900]
    seen = []
    for v in (dict(), dict(temperature=0.9, top_k=50, top_p=0.95, seed=3), dict(temperature=5.0, top_k=0, top_p=1.0, seed=9),
              dict(rep_penalty=3.0), dict(ignore_eos=True), dict(n_text=2, n_past=5), dict(slots=0.8), dict(slots=0.0, rules=1)):
        st = SR.copy_state(base)
        cfg = dict(V=V, audio_vocab=audio_vocab, eos=eos, frame_cap=SC.FRAME_CAP, row0=0, R=RT, R_total=RT, forced=forced)
        cfg.update({k: x for k, x in v.items() if k not in ("n_text", "n_past", "slots", "rules")})
        if "n_text" in v:
            st["n_text"][:], st["n_past"][:] = v["n_text"], v["n_past"]          # progress 5/6: the EOS boost is on, a forced EOS is not
        if "slots" in v:
            cfg["slots"] = [SC.slot(t_temp=v["slots"], t_top_k=20, t_top_p=0.9, seed=11 + r) for r in range(RT)]
        if "rules" in v:
            cfg["rules"] = [RULES[1]] * RT
            st["seen"] = np.full((RT, (audio_vocab + 31) // 32), 0xFFFFFFFF, np.uint32)
        scores = np.full((SC.FRAME_CAP, RT, 16), SENT, np.float32)
        rc, dev = run_talker(test_lib, logits, st, cfg, scores)
        assert rc == 0
        live = dev["n_past"] > st["n_past"]
        assert live.any()
        seen.append((live, scores[0, :, 0].copy()))
    all_live = np.logical_and.reduce([l for l, _ in seen])
    assert all_live.sum() >= 2
    for live, s in seen[1:]:
        assert s[all_live].tobytes() == seen[0][1][all_live].tobytes()
    for r in np.nonzero(all_live)[0]:
        assert R.matches(seen[0][1][r], R.talker_log_prob(logits[r], int(forced[0, r, 0]), audio_vocab, eos))[0]


# ---- code predictor -------------------------------------------------------------------------------------------------
def run_cp(lib, logits, codes, n_frames, cfg, table, scores):
    """One launch with the gather epilogue through q3t_cp_sample_rules_case (scores None) or q3t_cp_score_case
    -> (rc, codes after, gathered rows, ssq)."""
    RT, V = logits.shape
    H = table.shape[1]
    logits = np.ascontiguousarray(logits, np.float32)
    codes = np.array(codes, np.int32, copy=True)
    n_frames = np.ascontiguousarray(n_frames, np.int32)
    forced, seed_ptr, held = cfg.get("forced"), cfg.get("seed_ptr"), cfg.get("held")
    held = None if held is None else np.ascontiguousarray(held, np.int32)
    keep, slots = _slots_array(cfg.get("slots"))
    keep2, rules = _rules_array(cfg.get("rules"))
    h = np.full((RT, H), 777.0, np.float32)
    ssq = np.full((RT, H // 16), 777.0, np.float32)
    args = [hiplib.fptr(logits), V, RT, cfg["row0"], cfg["R"], cfg["group"], hiplib.iptr(codes), hiplib.iptr(n_frames),
            cfg["frame_cap"], _opt(forced, hiplib.iptr), cfg.get("temperature", 0.0), cfg.get("top_k", 50), cfg.get("seed", 0),
            None if seed_ptr is None else seed_ptr.ctypes.data_as(U64P), slots, 1, H, hiplib.fptr(table), None, 0, None, None, 0,
            None, 0, None, hiplib.fptr(h), hiplib.fptr(ssq), None, None, None, None, 0, _opt(held, hiplib.iptr),
            rules]
    if scores is None:
        return lib.q3t_cp_sample_rules_case(*args), codes, h, ssq
    return lib.q3t_cp_score_case(*args, hiplib.fptr(scores)), codes, h, ssq


def _cp_cases(V, mode):
    cases = SC.cp_decision_cases(V, mode != "scalar")
    if mode != "scalar":
        cases += SC.cp_held_cases(V)
    out = []
    for ci, case in enumerate(cases):
        cfg = dict(case["cfg"])
        RT, row0, Rn = cfg["R_total"], cfg["row0"], cfg["R"]
        rng = SC.rng_for("score_cp", V, mode, ci)
        if mode == "rules":
            cfg["rules"] = [RULES[int(rng.integers(3))] for _ in range(RT)]
        if "forced" not in cfg:   # every third row of the launch: an id of the vocabulary, or one beyond it
            forced = np.full((cfg["frame_cap"], RT, 16), -1, np.int32)
            for i in range(0, Rn, 3):
                forced[:, row0 + i, 1 + cfg["group"]] = V + 3 if (i // 3) % 3 == 1 else int(rng.integers(V))
            forced[:, 0, :] = 2
            cfg["forced"] = forced
        out.append(dict(logits=case["logits"], codes=case["codes"], n_frames=case["n_frames"], cfg=cfg))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V", SC.CP_VOCABS)
def test_cp_scores(test_lib, V, mode):
    assert SC.CP_VOCABS == (64, 2048, 2052, 4096)
    worst, kinds = [0.0, 0], dict(nan=0, ninf=0, forced=0, outside=0, held=0, unrecorded=0)
    table = SC.rng_for("score_cp_table", V).standard_normal((V, 64)).astype(np.float32)
    for case in _cp_cases(V, mode):
        logits, codes, n_frames, cfg = case["logits"], case["codes"], case["n_frames"], case["cfg"]
        g = cfg["group"]
        rc0, c0, h0, q0 = run_cp(test_lib, logits, codes, n_frames, cfg, table, None)
        scores = np.full((cfg["frame_cap"], cfg["R_total"], 16), SENT, np.float32)
        rows = range(cfg["row0"], cfg["row0"] + cfg["R"])
        for r in rows:            # a held row's frame already holds the score recorded with its id
            if SR.cp_held(cfg, r):
                scores[SR.cp_frame(n_frames[r], cfg["frame_cap"])[0], r, 1 + g] = RECORDED
        rc1, c1, h1, q1 = run_cp(test_lib, logits, codes, n_frames, cfg, table, scores)
        assert rc0 == 0 and rc1 == 0, (rc0, rc1)
        _same_bits(c1, c0, "codes")                                                  # 1
        _same_bits(h1, h0, "gathered rows")
        _same_bits(q1, q0, "ssq")
        written = {}
        for r in rows:
            f, keep = SR.cp_frame(n_frames[r], cfg["frame_cap"])
            if SR.cp_held(cfg, r):                                                   # 5
                assert scores[f, r, 1 + g].tobytes() == RECORDED.tobytes(), f"held row {r} lost its recorded score"
                scores[f, r, 1 + g] = SENT
                kinds["held"] += 1
                continue
            if not keep:
                kinds["unrecorded"] += 1
                continue
            fz = int(cfg["forced"][f, r, 1 + g])
            written[(f, r, 1 + g)] = fz if fz >= 0 else int(c1[f, r, 1 + g])         # 4
            kinds["forced"] += fz >= 0
            kinds["outside"] += fz >= V
        _check_scores(scores, written, lambda r, u: R.log_prob(logits[r], u), worst)  # 2, 3
        vals = np.array([scores[k] for k in written])
        kinds["nan"] += int(np.isnan(vals).sum())
        kinds["ninf"] += int(np.isneginf(vals).sum())
    print(f"cp V={V} {mode}: {worst[1]} scores, largest error {worst[0]:.3e}; {kinds}")
    need = ("nan", "ninf", "forced", "outside") + (("held",) if mode != "scalar" else ())
    assert worst[1] > 100 and all(kinds[k] > 0 for k in need), kinds

