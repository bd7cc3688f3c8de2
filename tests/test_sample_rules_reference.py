"""tests/sample_rules_ref.py (the reference tests/test_gpu_sample_rules.py grades the device with) pinned: against
tests/sample_ref.py at default rules, against transformers' RepetitionPenaltyLogitsProcessor for the whole-history window,
against hand-worked values at every rule's boundary -- and, from the reference alone, the share of ambiguous stochastic rows
of every family of tests/sample_rules_cases.py (at most 5 %, the cap tests/sample_cases.py states).  CPU only."""
import numpy as np
import pytest

from tests import sample_cases as SC
from tests import sample_ref as SR
from tests import sample_rules_cases as RC
from tests import sample_rules_ref as RR


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- default rules are the reference's constants ---------------------------------------------------------------------
@pytest.mark.parametrize("V", [64, 2152])
def test_default_rules_equal_sample_ref_talker(V):
    n = 0
    for slots_mode in (0, 1):
        for case in SC.talker_decision_cases(V, slots_mode, per_family=1):
            logits, st, cfg = case["logits"], case["st"], case["cfg"]
            want = SR.talker_sets(logits, st, cfg)
            ruled = dict(cfg, rules=[RR.rules() for _ in range(cfg["R_total"])]) if slots_mode else cfg
            got = RR.talker_sets_rules(logits, dict(st, seen=np.zeros((cfg["R_total"], RR.seen_words(cfg["audio_vocab"])), np.uint32)), ruled)
            assert got.keys() == want.keys()
            for r in want:
                assert got[r][0] == want[r][0]
                np.testing.assert_array_equal(_bits(got[r][1]), _bits(want[r][1]))
                ign = bool(cfg["ignore_eos"])
                l, forced = SR.process_talker(logits[r], st["past"][r], int(st["n_past"][r]), int(st["n_text"][r]),
                                              cfg["audio_vocab"], cfg["eos"], ign, 1.2)
                l2, forced2, masked = RR.process_talker_rules(logits[r], st["past"][r], int(st["n_past"][r]), int(st["n_text"][r]),
                                                              RR.rules(), None, cfg["audio_vocab"], cfg["eos"], ign)
                np.testing.assert_array_equal(_bits(l), _bits(l2))
                assert forced == forced2 and masked == ign
                n += 1
    assert n > 100


@pytest.mark.parametrize("V", [64, 2048])
def test_default_rules_equal_sample_ref_cp(V):
    for case in SC.cp_decision_cases(V, 1, per_family=1):
        cfg = case["cfg"]
        # (cp_top_p 1 is "no cut", as the top_p 0 sample_ref passes)
        assert RR.cp_sets_rules(case["logits"], case["n_frames"], dict(cfg, rules=[RR.rules()] * cfg["R_total"])) == \
            SR.cp_sets(case["logits"], case["n_frames"], cfg) == RR.cp_sets_rules(case["logits"], case["n_frames"], cfg)


def test_default_values_in_f32():
    """The doubles the EOS rules are computed with are exact in f32, so a default entry gives the constants' bits; the
    penalty is used as an f32 on both sides (1.2f, which is not 1.2)."""
    for k, v in RR.DEFAULT.items():
        if k != "rep_penalty":
            assert float(np.float32(v)) == float(v), k
    assert np.float32(RR.DEFAULT["rep_penalty"]) == np.float32(1.2)


# ---- the whole-history window is transformers' repetition penalty ----------------------------------------------------
@pytest.mark.parametrize("p", [1.0, 1.05, 1.2, 3.0])
def test_window_0_is_the_transformers_repetition_penalty(p):
    torch = pytest.importorskip("torch")
    from transformers import RepetitionPenaltyLogitsProcessor
    rng = np.random.default_rng(int(p * 100))
    V, audio_vocab, eos = 2152, 2048, 2150
    proc = RepetitionPenaltyLogitsProcessor(float(p))
    for n in (1, 5, 33, 100):
        hist = [int(t) for t in rng.integers(0, audio_vocab, n)]
        logits = (4.0 * rng.standard_normal(V)).astype(np.float32)
        logits[hist[0]] = 0.0                                             # a zero logit among the penalised ones
        st = dict(past=np.zeros((1, 32), np.int32), n_past=np.zeros(1, np.int32), seen=np.zeros((1, RR.seen_words(audio_vocab)), np.uint32))
        RC_hist = hist
        for i, t in enumerate(RC_hist):
            st["past"][0, i % 32] = t
            RR.seen_add(st["seen"][0], t, audio_vocab)
        got, _, _ = RR.process_talker_rules(logits, st["past"][0], n, 0, RR.rules(rep_penalty=p, rep_window=0), st["seen"][0], audio_vocab, eos)
        masked = SR.nan_as_inf(logits)
        ids = np.arange(V)
        masked[(ids >= audio_vocab) & (ids != eos)] = np.float32(-1e10)
        want = proc(torch.tensor([hist], dtype=torch.long), torch.tensor(masked[None], dtype=torch.float32))[0].numpy()
        np.testing.assert_array_equal(_bits(got), _bits(want))


# ---- hand-worked values ----------------------------------------------------------------------------------------------
def _ring(chron):
    ring = np.full(32, -5, np.int32)
    for i in range(max(0, len(chron) - 32), len(chron)):
        ring[i % 32] = chron[i]
    return ring


def test_window_boundaries_by_hand():
    hist = list(range(100, 140))                       # 40 ids, the newest 139; the ring holds 108 .. 139
    ring = _ring(hist)
    seen = RR.seen_of(hist, 2048)
    assert RR.penalised_ids(ring, 40, RR.rules(rep_window=1), seen, 2048) == {139}
    assert RR.penalised_ids(ring, 40, RR.rules(rep_window=2), seen, 2048) == {138, 139}
    assert RR.penalised_ids(ring, 40, RR.rules(rep_window=30), seen, 2048) == set(range(110, 140))
    assert RR.penalised_ids(ring, 40, RR.rules(rep_window=0), seen, 2048) == set(range(100, 140))    # older than the ring
    assert RR.penalised_ids(ring, 1, RR.rules(rep_window=30), seen, 2048) == {ring[0]}
    assert RR.penalised_ids(ring, 0, RR.rules(rep_window=30), np.zeros(64, np.uint32), 2048) == set()
    assert RR.penalised_ids(ring, 40, RR.rules(), seen, 2048) == set(SR.window_ids(ring, 40))


def test_seen_set_transition_by_hand():
    row = np.zeros(RR.seen_words(2048), np.uint32)
    assert len(row) == 64 and RR.seen_words(48) == 2 and RR.seen_words(33) == 2 and RR.seen_words(32) == 1
    for t in (0, 31, 32, 63, 2047, 31):
        RR.seen_add(row, t, 2048)
    assert row[0] == 0x80000001 and row[1] == 0x80000001 and row[63] == 0x80000000 and row[2:63].sum() == 0
    before = row.copy()
    for t in (2048, 2150, -1, 5000):                   # no bit outside the audio vocabulary
        RR.seen_add(row, t, 2048)
    np.testing.assert_array_equal(row, before)
    assert RR.seen_has(row, 31) and not RR.seen_has(row, 30) and not RR.seen_has(row, 2048) and not RR.seen_has(row, -1)
    codes = np.zeros((5, 16), np.int32)
    codes[:, 0] = (3, 3, 35, 34, 3)
    np.testing.assert_array_equal(RR.prompt_seen(codes, 48), np.array([8, 12], np.uint32))


def test_penalty_arithmetic_by_hand():
    l = np.full(64, -50.0, np.float32)
    l[3], l[4], l[5] = 6.0, -6.0, 0.0
    ring = _ring([3, 4, 5])
    out, _, _ = RR.process_talker_rules(l, ring, 3, 0, RR.rules(rep_penalty=3.0), None, 48, 50)
    assert out[3] == np.float32(2.0) and out[4] == np.float32(-18.0) and out[5] == 0.0
    out, _, _ = RR.process_talker_rules(l, ring, 3, 0, RR.rules(rep_penalty=1.0), None, 48, 50)
    np.testing.assert_array_equal(_bits(out[:48]), _bits(l[:48]))                       # 1 is "no penalty", exactly
    out, _, _ = RR.process_talker_rules(l, ring, 3, 0, RR.rules(rep_penalty=1.05), None, 48, 50)
    assert out[3] == np.float32(6.0) / np.float32(1.05) and out[4] == np.float32(-6.0) * np.float32(1.05)


def test_eos_rules_by_hand():
    l = np.zeros(64, np.float32)
    ring = _ring([])
    def eos_after(n_past, n_text, ign=False, **kw):
        out, forced, masked = RR.process_talker_rules(l, _ring(list(range(40, 40 + min(n_past, 5)))), n_past, n_text, RR.rules(**kw), None, 48, 50, ign)
        return out[50], forced, masked
    # progress 30 / 15 = 2.0 exactly: the boost is at its ceiling, the force (strictly above) is not reached
    assert eos_after(30, 5) == (np.float32(15.0), False, False)
    assert eos_after(31, 5) == (np.float32(15.0), True, False)
    assert eos_after(30, 5, eos_boost=7.5) == (np.float32(7.5), False, False)
    assert eos_after(30, 5, eos_boost=0.0) == (np.float32(0.0), False, False)
    # progress 12 / 15 = 0.8 exactly: no boost yet; 13 / 15: (13/15 - 0.8) / 0.7 of the ceiling, rounded to f32 once
    assert eos_after(12, 5)[0] == 0.0
    assert eos_after(13, 5)[0] == np.float32((13 / 15 - 0.8) / 0.7 * 15.0)
    assert eos_after(13, 5, eos_boost=7.5)[0] == np.float32((13 / 15 - 0.8) / 0.7 * 7.5)
    # eos_force: strictly above; 0 never
    assert eos_after(15, 5, eos_force=1.0)[1] is False and eos_after(16, 5, eos_force=1.0)[1] is True
    assert eos_after(1000, 5, eos_force=0.0)[1] is False
    assert eos_after(1000, 0)[1] is False                                              # no text length, no progress
    # min_past: n_past below it masks EOS as ignore_eos does (no boost); at it the rules are back
    assert eos_after(30, 5, min_past=31) == (np.float32(-1e10), False, True)
    assert eos_after(31, 5, min_past=32) == (np.float32(-1e10), True, True)           # (the caller drops a masked force)
    assert eos_after(31, 5, min_past=31) == (np.float32(15.0), True, False)
    assert eos_after(31, 5, ign=True) == (np.float32(-1e10), True, True)
    assert ring is not None


def test_talker_sets_honour_the_mask_on_a_forced_eos():
    V, (av, eos) = 64, SC.TALKER_VOCABS[64]
    logits = np.zeros((1, V), np.float32)
    logits[0, 7] = 5.0
    st = dict(past=np.full((1, 32), 9, np.int32), n_past=np.array([40], np.int32), n_text=np.array([5], np.int32),
              done=np.zeros(1, np.int32), n_frames=np.zeros(1, np.int32), seen=np.zeros((1, 2), np.uint32))
    cfg = dict(V=V, audio_vocab=av, eos=eos, row0=0, R=1, frame_cap=8, slots=[SC.slot()], rules=[RR.rules()])
    assert RR.talker_sets_rules(logits, st, cfg)[0][0] == {eos}
    cfg["rules"] = [RR.rules(min_past=41)]
    assert RR.talker_sets_rules(logits, st, cfg)[0][0] == {7}
    cfg["rules"] = [RR.rules(eos_force=0.0, eos_boost=0.0)]
    assert RR.talker_sets_rules(logits, st, cfg)[0][0] == {7}


def test_seen_follows_the_ring():
    V, (av, eos) = 64, SC.TALKER_VOCABS[64]
    st = dict(past=np.zeros((2, 32), np.int32), n_past=np.array([33, 2], np.int32), n_text=np.zeros(2, np.int32),
              done=np.zeros(2, np.int32), n_frames=np.zeros(2, np.int32), pos0=np.zeros(2, np.int32), pos=np.zeros(2, np.int32),
              codes=np.full((8, 2, 16), -7, np.int32), seen=np.zeros((2, 2), np.uint32))
    cfg = dict(V=V, audio_vocab=av, eos=eos, row0=0, R=2, frame_cap=8, slots=[SC.slot(), SC.slot()],
               forced=np.full((8, 2, 16), -1, np.int32))
    cfg["forced"][0, 1, 0] = 47
    RR.talker_apply_row_rules(st, cfg, 0, 33)
    RR.talker_apply_row_rules(st, cfg, 1, 5)            # teacher forcing: the set takes the forced id, as the ring does
    assert st["past"][0, 1] == 33 and st["seen"][0].tolist() == [0, 2]
    assert st["past"][1, 2] == 47 and st["codes"][0, 1, 0] == 5 and st["seen"][1].tolist() == [0, 1 << 15]
    before = SR.copy_state(st)
    RR.talker_apply_row_rules(st, cfg, 0, eos)          # an ending row writes nothing
    np.testing.assert_array_equal(st["seen"], before["seen"])


def test_cp_top_p_by_hand():
    l = np.full(64, -np.inf, np.float32)
    l[[3, 9, 20, 40]] = 0.0                              # four equal weights: cumulative 1/4, 1/2, 3/4, 1
    cfg = dict(V=64, row0=0, R=1, group=2, frame_cap=8, slots=[SC.slot(c_temp=1.0, c_top_k=0, seed=11)])
    nf = np.array([1], np.int32)
    u = SR.uniform01(11, 0, 1, 3)
    def picks(tp):
        return RR.cp_sets_rules(l[None], nf, dict(cfg, rules=[RR.rules(cp_top_p=tp)]))[0]
    assert picks(1.0) == {(3, 9, 20, 40)[int(u * 4)]} == RR.cp_sets_rules(l[None], nf, cfg)[0]
    assert picks(0.3) == {(3, 9)[int(u * 2)]}           # searchsorted(cumsum, 0.3) + 1 = 2 entries
    assert picks(0.6) == {(3, 9, 20)[int(u * 3)]}
    assert picks(1e-6) == {3}
    cfg["slots"][0]["c_temp"] = 0.0
    assert picks(0.5) == {3}                             # the arg-max ignores it


# ---- the cap on ambiguous rows, from the reference alone -------------------------------------------------------------
def _share(cases, sets_of, talker):
    out = {}
    for c in cases:
        sets = sets_of(c)
        for i, fam in enumerate(c["families"]):
            r = c["cfg"]["row0"] + i
            if SR.is_greedy(SR._row_params(c["cfg"], r, talker)["temperature"]) or r not in sets:
                continue
            a, n = out.get(fam, (0, 0))
            out[fam] = (a + (len(sets[r]) > 1), n + 1)
    return out


def test_ambiguity_cap_rule_cases():
    """At most 5 % of the stochastic rows of every family are ambiguous (a condition on the inputs, not a measurement)."""
    total = {}
    for V in SC.TEXT_TALKER_VOCABS:
        cases = RC.talker_rule_cases(V) + RC.talker_family_cases(V)
        sh = _share(cases, lambda c: {r: s for r, (s, _) in RR.talker_sets_rules(c["logits"], c["st"], c["cfg"]).items()}, True)
        SC.share_report(f"talker rules V={V}", sh)
        for f, (a, n) in sh.items():
            total["talker " + f] = tuple(np.add(total.get("talker " + f, (0, 0)), (a, n)))
    for V in SC.TEXT_CP_VOCABS:
        sh = _share(RC.cp_rule_cases(V), lambda c: RR.cp_sets_rules(c["logits"], c["n_frames"], c["cfg"]), False)
        SC.share_report(f"cp rules V={V}", sh)
        for f, (a, n) in sh.items():
            total["cp " + f] = tuple(np.add(total.get("cp " + f, (0, 0)), (a, n)))
    assert len(total) >= 10
    for f, (a, n) in total.items():
        assert n > 0 and a <= 0.05 * n, (f, a, n)


# ---- the engine tests' reference (tests/rules_ref.py) ------------------------------------------------------------------
def test_rules_ref_decision_at_default_rules_is_prompt_ref_and_follows_sample_rules_ref():
    from types import SimpleNamespace
    from qwen3_tts_axera_russian_amd.engine import SlotRules
    from tests import prompt_ref as pr
    from tests import rules_ref as rr
    cpu = SimpleNamespace(cfg=SimpleNamespace(codec_eos=2150))
    rng = np.random.default_rng(5)
    variants = [SlotRules(), SlotRules(rep_penalty=1.05, rep_window=0, eos_boost=0.0, eos_force=0.0, min_frames=2),
                SlotRules(rep_penalty=3.0, rep_window=2, eos_boost=7.5, eos_force=1.0, min_frames=9)]
    for n_past, n_text, n_prompt in ((0, 5, 0), (3, 5, 0), (13, 5, 10), (16, 5, 10), (31, 5, 0), (40, 5, 33), (40, 0, 40), (100, 30, 40)):
        past = [int(t) for t in rng.integers(0, 2048, n_past)]
        logits = (0.64 * rng.standard_normal(3072)).astype(np.float32)
        for ign in (False, True):
            assert rr.decide_ruled(cpu, logits, past, n_text, ign, variants[0], n_prompt) == pr.decide(cpu, logits, past, n_text, ign)
            for ru in variants:
                ring = np.zeros(32, np.int32)
                for i in range(max(0, n_past - 32), n_past):
                    ring[i % 32] = past[i]
                entry = RR.rules(rep_penalty=ru.rep_penalty, rep_window=ru.rep_window, eos_boost=ru.eos_boost, eos_force=ru.eos_force,
                                 min_past=n_prompt + ru.min_frames)
                l, forced, masked = RR.process_talker_rules(logits, ring, n_past, n_text, entry, RR.seen_of(past, 2048), 2048, 2150, ign)
                want = 2150 if forced and not masked else SR.first_argmax(l)
                assert rr.decide_ruled(cpu, logits, past, n_text, ign, ru, n_prompt)[0] == want
