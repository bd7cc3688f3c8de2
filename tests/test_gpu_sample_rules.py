"""The per-slot sampler rules on the device, single launches, graded exactly against tests/sample_rules_ref.py.

talker_sample_kernel_rules / cp_argmax_kernel_rules through q3t_talker_sample_rules_case / q3t_cp_sample_rules_case, and
prompt_rows_kernel's seen-set through q3t_prompt_rows_seen_case: 16 rows per launch at row 3 of 21, so rows outside the
launch are checked to be untouched.  Graded as tests/test_gpu_sample_decisions.py grades: the device's pick is in the
reference's acceptable set and every piece of state the launch owns -- codes, ring, counters, held flags and the seen-sets --
equals the reference's bit for bit.  The hand cases put a competitor one float32 step below / above the processed value
under test, so the arg-max resolves a single bit of the device's arithmetic (tests/sample_rules_cases.py).  The share of
ambiguous stochastic rows of every family is capped by tests/test_sample_rules_reference.py::test_ambiguity_cap_rule_cases."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import sample_cases as SC
from tests import sample_ref as SR
from tests import sample_rules_cases as RC
from tests import sample_rules_ref as RR
from tests.test_gpu_sample_decisions import _opt, _slots_array, check_cp, check_talker

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
U32P = ctypes.POINTER(ctypes.c_uint32)
ROW_KEYS = ("past", "n_past", "done", "n_frames", "pos", "seen")


def _rules_array(rules):
    if rules is None:
        return None, None
    arr = (hiplib.KernelSlotRulesC * len(rules))()
    for a, r in zip(arr, rules):
        a.rep_penalty, a.rep_window, a.eos_boost, a.eos_force = r["rep_penalty"], r["rep_window"], r["eos_boost"], r["eos_force"]
        a.min_past, a.cp_top_p = r["min_past"], r["cp_top_p"]
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def run_talker_rules(lib, logits, st, cfg):
    """-> (return code, state after the launch) through q3t_talker_sample_rules_case; st["seen"] / st["held"] /
    cfg["rules"] / cfg["text_avail"] may each be missing (null)."""
    out = SR.copy_state(st)
    RT = logits.shape[0]
    logits = np.ascontiguousarray(logits, np.float32)
    forced, ta = cfg.get("forced"), cfg.get("text_avail")
    ta = None if ta is None else np.ascontiguousarray(ta, np.int32)
    keep, slots = _slots_array(cfg.get("slots"))
    keep2, rules = _rules_array(cfg.get("rules"))
    seen = out.get("seen")
    rc = lib.q3t_talker_sample_rules_case(
        hiplib.fptr(logits), logits.shape[1], RT, cfg["row0"], cfg["R"], hiplib.iptr(out["past"]), hiplib.iptr(out["n_past"]),
        hiplib.iptr(out["n_text"]), hiplib.iptr(out["done"]), hiplib.iptr(out["n_frames"]), hiplib.iptr(out["pos0"]),
        hiplib.iptr(out["pos"]), hiplib.iptr(out["codes"]), cfg["frame_cap"], _opt(forced, hiplib.iptr),
        cfg["audio_vocab"], cfg["eos"], int(cfg.get("ignore_eos", False)), cfg.get("max_frames", 0),
        cfg.get("rep_penalty", 1.2), cfg.get("temperature", 0.0), cfg.get("top_k", 50), cfg.get("top_p", 0.95),
        cfg.get("seed", 0), None, slots, _opt(ta, hiplib.iptr), _opt(out.get("held"), hiplib.iptr), rules,
        None if seen is None else seen.ctypes.data_as(U32P))
    return rc, out


def check_talker_rules(lib, case):
    """One launch: every row's decision is in its acceptable set, and the whole state -- the seen-sets and the rows outside
    the launch included -- equals the reference's."""
    logits, st, cfg = case["logits"], case["st"], case["cfg"]
    rc, dev = run_talker_rules(lib, logits, st, cfg)
    assert rc == 0, f"launch refused: {rc}"
    sets = RR.talker_sets_rules(logits, st, cfg)
    exp = SR.copy_state(st)
    if "held" in st:
        exp["held"] = SR.talker_held_after(st, cfg)
    for r, (picks, _) in sets.items():
        for code in sorted(picks):
            trial = SR.copy_state(st)
            RR.talker_apply_row_rules(trial, cfg, r, code)
            if all(np.array_equal(trial[k][r], dev[k][r]) for k in ROW_KEYS if k in st) and \
                    np.array_equal(trial["codes"][:, r], dev["codes"][:, r]):
                RR.talker_apply_row_rules(exp, cfg, r, code)
                break
        else:
            trial = SR.copy_state(st)
            RR.talker_apply_row_rules(trial, cfg, r, min(picks))
            diff = {k: (trial[k][r].tolist(), dev[k][r].tolist()) for k in ROW_KEYS if k in st and not np.array_equal(trial[k][r], dev[k][r])}
            f = int(st["n_frames"][r])
            raise AssertionError(
                f"row {r} ({case['families'][r - cfg['row0']]}): acceptable decisions {sorted(picks)[:8]}, device recorded code_0 "
                f"{dev['codes'][min(f, cfg['frame_cap'] - 1), r, 0]}; rules {RR.row_rules(cfg, r)}, params "
                f"{SR._row_params(cfg, r, True)}, n_past {st['n_past'][r]}, n_text {st['n_text'][r]}, flags {SR.slot_flags(cfg, r)}; "
                f"(expected, device) {diff}")
    for k in exp:
        np.testing.assert_array_equal(dev[k], exp[k], err_msg=k)
    return dev


# ---- talker -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["window", "penalty", "eos", "eos_ignored", "forced", "held", "families"])
@pytest.mark.parametrize("V", SC.TEXT_TALKER_VOCABS)
def test_talker_rules(test_lib, V, group):
    cases = {"window": RC.window_cases, "penalty": RC.penalty_cases, "eos": RC.eos_cases,
             "eos_ignored": lambda v: RC.eos_cases(v, ignore_eos=True), "forced": RC.forced_cases, "held": RC.held_cases,
             "families": RC.talker_family_cases}[group](V)
    assert cases
    held = ended = went_on = 0
    for case in cases:
        dev = check_talker_rules(test_lib, case)
        rows = slice(case["cfg"]["row0"], case["cfg"]["row0"] + case["cfg"]["R"])
        held += int((dev.get("held", np.zeros(1))[rows] == 1).sum())
        ended += int((dev["done"][rows] != case["st"]["done"][rows]).sum())
        went_on += int((dev["n_past"][rows] != case["st"]["n_past"][rows]).sum())
    # the cases exercise what they are named for
    assert went_on > 0
    if group in ("eos", "held"):
        assert ended > 0
    if group == "held":
        assert held > 0


@pytest.mark.parametrize("V", SC.TEXT_TALKER_VOCABS)
def test_window_cases_separate_the_windows(V):
    """(reference only) the probes decide differently under another window: a device that ignored rep_window could not
    pass."""
    flipped = 0
    for case in RC.window_cases(V):
        cfg = case["cfg"]
        for r, (picks, _) in RR.talker_sets_rules(case["logits"], case["st"], cfg).items():
            other = RR.talker_sets_rules(case["logits"], case["st"], dict(cfg, rules=[RR.rules(rep_window=30 if cfg["rules"][r]["rep_window"] != 30 else 1)] * cfg["R_total"]))
            flipped += SR.is_greedy(cfg["slots"][r]["t_temp"]) and other[r][0] != picks
    assert flipped >= 10


@pytest.mark.parametrize("V", SC.TEXT_TALKER_VOCABS)
def test_null_rules_and_default_rules_are_the_launch_without_them(test_lib, V):
    """rules = NULL / seen = NULL through the new hook is the existing per-slot launch (graded by the existing reference);
    default rules with a seen-set give the same codes, ring and counters bit for bit."""
    audio_vocab, _ = SC.TALKER_VOCABS[V]
    cases = SC.talker_decision_cases(V, 1, per_family=1)[:6] + SC.text_talker_cases(V)
    for case in cases:
        st, cfg = case["st"], case["cfg"]
        plain = check_talker(test_lib, case)                              # q3t_talker_sample(_text)_case
        rc, null = run_talker_rules(test_lib, case["logits"], st, cfg)    # the rules hook, both null
        assert rc == 0
        ruled_st = dict(st, seen=np.zeros((cfg["R_total"], RR.seen_words(audio_vocab)), np.uint32))
        ruled_cfg = dict(cfg, rules=[RR.rules() for _ in range(cfg["R_total"])])
        rc, ruled = run_talker_rules(test_lib, case["logits"], ruled_st, ruled_cfg)
        assert rc == 0
        for k in plain:
            np.testing.assert_array_equal(null[k], plain[k], err_msg=k)
            np.testing.assert_array_equal(ruled[k], plain[k], err_msg=k)
        # and the set took exactly the ids the ring took
        for r in range(cfg["R_total"]):
            want = np.zeros(RR.seen_words(audio_vocab), np.uint32)
            if plain["n_past"][r] != st["n_past"][r]:
                RR.seen_add(want, int(plain["past"][r, int(st["n_past"][r]) % 32]), audio_vocab)
            np.testing.assert_array_equal(ruled["seen"][r], want)


def test_launcher_refuses_rules_without_their_company(test_lib):
    case = RC.window_cases(64)[0]
    st, cfg = case["st"], case["cfg"]
    no_seen = {k: v for k, v in st.items() if k != "seen"}
    assert run_talker_rules(test_lib, case["logits"], no_seen, cfg)[0] == -1              # rules without a seen-set
    scalar = {k: v for k, v in cfg.items() if k != "slots"}
    assert run_talker_rules(test_lib, case["logits"], st, scalar)[0] == -1               # rules outside per-slot mode
    assert run_talker_rules(test_lib, case["logits"], st, dict(scalar, rules=None))[0] == -1   # a seen-set outside it
    cp = RC.cp_rule_cases(64)[0]
    assert _run_cp_rules(test_lib, cp, {k: v for k, v in cp["cfg"].items() if k != "slots"})[0] == -1


# ---- code predictor -----------------------------------------------------------------------------------------------------
def _run_cp_rules(lib, case, cfg):
    logits = np.ascontiguousarray(case["logits"], np.float32)
    RT, V = logits.shape
    codes = np.array(case["codes"], np.int32, copy=True)
    n_frames = np.ascontiguousarray(case["n_frames"], np.int32)
    keep, slots = _slots_array(cfg.get("slots"))
    keep2, rules = _rules_array(cfg.get("rules"))
    rc = lib.q3t_cp_sample_rules_case(
        hiplib.fptr(logits), V, RT, cfg["row0"], cfg["R"], cfg["group"], hiplib.iptr(codes), hiplib.iptr(n_frames),
        cfg["frame_cap"], None, cfg.get("temperature", 0.0), cfg.get("top_k", 50), cfg.get("seed", 0), None, slots, 0, 0,
        None, None, 0, None, None, 0, None, 0, None, None, None, None, None, None, None, 0, None, rules)
    return rc, codes


@pytest.mark.parametrize("V", SC.TEXT_CP_VOCABS)
def test_cp_top_p(test_lib, V):
    cases = RC.cp_rule_cases(V)
    assert {c["cfg"]["group"] for c in cases} == {0, 14}
    cut = 0
    for case in cases:
        cfg = case["cfg"]
        rc, dev = _run_cp_rules(test_lib, case, cfg)
        assert rc == 0
        sets = RR.cp_sets_rules(case["logits"], case["n_frames"], cfg)
        uncut = SR.cp_sets(case["logits"], case["n_frames"], cfg)
        exp = np.array(case["codes"], copy=True)
        for r, picks in sets.items():
            f, keep = SR.cp_frame(case["n_frames"][r], cfg["frame_cap"])
            got = int(dev[f, r, 1 + cfg["group"]])
            assert got in picks, (f"row {r} ({case['families'][r - cfg['row0']]}): device {got}, acceptable {sorted(picks)[:8]}; "
                                  f"cp_top_p {cfg['rules'][r]['cp_top_p']}, params {SR._row_params(cfg, r, False)}")
            exp[f, r, 1 + cfg["group"]] = got
            cut += picks != uncut[r]
        np.testing.assert_array_equal(dev, exp)                           # nothing else written, no row outside the launch
        # default rules and no rules: the existing launch
        plain, _ = check_cp(test_lib, dict(case, cfg={k: v for k, v in cfg.items() if k != "rules"}))
        rc, dflt = _run_cp_rules(test_lib, case, dict(cfg, rules=[RR.rules()] * cfg["R_total"]))
        assert rc == 0
        np.testing.assert_array_equal(dflt, plain)
    assert cut >= 2, "the cut must move some picks, or the cases show nothing"


# ---- the prompt's seen-set ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", RC.PROMPT_TS)
def test_prompt_rows_seed_the_seen_set(test_lib, T):
    """Column 0 of ALL T frames, not of the last 32; duplicates and ids sharing a word (the workgroups' atomic OR); bits
    already in the set stay; the ring and the counter as without a set."""
    H, audio_vocab, cp_vocab = 32, 48, 64
    rng = SC.rng_for("rules", "prompt", T)
    codes = RC.prompt_codes(T, audio_vocab, rng)
    temb = rng.standard_normal((64, H)).astype(np.float32)
    tabs = rng.standard_normal((15, cp_vocab, H)).astype(np.float32)
    words = RR.seen_words(audio_vocab)

    def run(seen, vocab=audio_vocab):
        past, n_past = np.full(32, -9, np.int32), np.array([-9], np.int32)
        args = [hiplib.iptr(codes), T, hiplib.iptr(past), hiplib.iptr(n_past), hiplib.fptr(temb), temb.shape[0], hiplib.fptr(tabs),
                15, cp_vocab, 15, None, H, 0, T, T, 0, None, None, None, None, 0]
        if seen is None:
            rc = test_lib.q3t_prompt_rows_case(*args)
        else:
            assert len(seen) == RR.seen_words(vocab)
            rc = test_lib.q3t_prompt_rows_seen_case(*args, seen.ctypes.data_as(U32P), vocab)
        assert rc == 0, rc
        return past, n_past

    seen = np.zeros(words, np.uint32)
    past, n_past = run(seen)
    np.testing.assert_array_equal(seen, RR.prompt_seen(codes, audio_vocab))
    assert {t for t in range(audio_vocab) if RR.seen_has(seen, t)} == set(int(c) for c in codes[:, 0])
    past0, n_past0 = run(None)
    np.testing.assert_array_equal(past, past0)
    assert n_past[0] == n_past0[0] == T
    pre = np.array([1 << 5, 1 << 9], np.uint32)                          # the launch ORs into what is there
    seen2 = pre.copy()
    run(seen2)
    np.testing.assert_array_equal(seen2, RR.prompt_seen(codes, audio_vocab) | pre)
    # ids outside [0, audio_vocab) have no bit: neither beyond the set's words (a vocabulary of 32: one word) nor in the
    # padding of its last word (a vocabulary of 40: ids 40 .. 47 of the prompt share word 1 with 32 .. 39)
    for vocab in (32, 40):
        small = np.zeros(RR.seen_words(vocab), np.uint32)
        run(small, vocab)
        np.testing.assert_array_equal(small, RR.prompt_seen(codes, vocab), err_msg=f"audio vocabulary {vocab}")
    if T >= 31:
        assert (codes[:, 0] >= 40).any() and ((codes[:, 0] >= 32) & (codes[:, 0] < 40)).any()
