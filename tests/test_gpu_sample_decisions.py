"""Every device sampling decision against tests/sample_ref.py, exactly.

talker_sample_kernel / talker_sample_kernel_slots and cp_argmax_kernel / cp_argmax_kernel_slots run through the hooks
q3t_talker_sample_case / q3t_cp_sample_case: one case per row, many rows per launch.  The draw is a counter-based hash,
so u is known; the device's pick must be in sample_ref.acceptable_picks (one element, except where a comparison falls
inside the fp32 error bound gamma -- at most 5 % of the stochastic cases of a family, printed by every test), and
every piece of state the launch owns (codes, ring, counters, gathered rows) must equal the reference bit for bit,
rows outside the launch included.

Ambiguous shares (computed from the reference alone, so the same on every machine; worst family over all vocabularies
and both modes): talker 3 of 75 (4.0 %), code predictor 1 of 47 (2.1 %); most families 0 -- printed per family by
tests/test_sample_reference.py::test_ambiguity_cap and by the decision tests here.

Text slots (q3t_talker_sample_text_case / q3t_cp_sample_text_case, 16 rows per launch at row 3 of 21, greedy and stochastic
rows side by side): the hold rule over its hand grid, the EOS mask of flags & 2, held rows of the code predictor under every
epilogue, and the text row the feedback adds last.  None of their stochastic rows is ambiguous (talker 0 of 58 + 0 of 16,
code predictor 0 of 8 + 0 of 48 over both vocabularies; held rows make no draw and are not counted) --
tests/test_sample_reference.py::test_ambiguity_cap_text_cases."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import sample_cases as SC
from tests import sample_ref as SR

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
U16P = ctypes.POINTER(ctypes.c_uint16)


def _slots_array(slots):
    if slots is None:
        return None, None
    arr = (hiplib.KernelSlotParamsC * len(slots))()
    for a, s in zip(arr, slots):
        a.max_frames, a.t_temp, a.t_top_k, a.t_top_p = s["max_frames"], s["t_temp"], s["t_top_k"], s["t_top_p"]
        a.c_temp, a.c_top_k, a.seed, a.no_row = s["c_temp"], s["c_top_k"], s["seed"], s["no_row"]
        a.flags = s.get("flags", 0)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _opt(a, ptr):
    return None if a is None else ptr(a)


def run_talker(lib, logits, st, cfg):
    """-> (return code, state after the launch); `st` itself stays as it is.  A state with `held` (and cfg["text_avail"],
    which may be None) goes through q3t_talker_sample_text_case."""
    out = SR.copy_state(st)
    RT = logits.shape[0]
    assert cfg.get("R_total", RT) == RT
    logits = np.ascontiguousarray(logits, np.float32)
    forced = cfg.get("forced")
    seed_ptr = cfg.get("seed_ptr")
    keep, slots = _slots_array(cfg.get("slots"))
    text = "held" in st or cfg.get("text_avail") is not None
    ta = cfg.get("text_avail")
    ta = None if ta is None else np.ascontiguousarray(ta, np.int32)
    extra = (_opt(ta, hiplib.iptr), _opt(out.get("held"), hiplib.iptr)) if text else ()
    rc = (lib.q3t_talker_sample_text_case if text else lib.q3t_talker_sample_case)(
        hiplib.fptr(logits), logits.shape[1], RT, cfg["row0"], cfg["R"], hiplib.iptr(out["past"]), hiplib.iptr(out["n_past"]),
        hiplib.iptr(out["n_text"]), hiplib.iptr(out["done"]), hiplib.iptr(out["n_frames"]), hiplib.iptr(out["pos0"]),
        hiplib.iptr(out["pos"]), hiplib.iptr(out["codes"]), cfg["frame_cap"], _opt(forced, hiplib.iptr),
        cfg["audio_vocab"], cfg["eos"], int(cfg.get("ignore_eos", False)), cfg.get("max_frames", 0),
        cfg.get("rep_penalty", 1.2), cfg.get("temperature", 0.0), cfg.get("top_k", 50), cfg.get("top_p", 0.95),
        cfg.get("seed", 0), None if seed_ptr is None else seed_ptr.ctypes.data_as(U64P), slots, *extra)
    return rc, out


ROW_KEYS = ("past", "n_past", "done", "n_frames", "pos")


def check_talker(lib, case, counts=None):
    """One launch: the decision of every row is in its acceptable set and the whole state equals the reference's.  A
    held row has no decision: it is missing from the sets, so the reference's state keeps its input bit for bit in
    past, n_past, done, n_frames, pos and codes, and the comparison of the whole state below demands the same of the
    device; held[] is compared over every row of the batch."""
    logits, st, cfg = case["logits"], case["st"], case["cfg"]
    rc, dev = run_talker(lib, logits, st, cfg)
    assert rc == 0, f"launch refused: {rc}"
    sets = SR.talker_sets(logits, st, cfg)
    exp = SR.copy_state(st)
    if "held" in st:
        exp["held"] = SR.talker_held_after(st, cfg)
    for r, (picks, _) in sets.items():
        ok = False
        for code in sorted(picks):
            trial = SR.copy_state(st)
            SR.talker_apply_row(trial, cfg, r, code)
            if all(np.array_equal(trial[k][r], dev[k][r]) for k in ROW_KEYS) and np.array_equal(trial["codes"][:, r], dev["codes"][:, r]):
                SR.talker_apply_row(exp, cfg, r, code)
                ok = True
                break
        if not ok:
            trial = SR.copy_state(st)
            SR.talker_apply_row(trial, cfg, r, min(picks))
            diff = {k: (trial[k][r].tolist(), dev[k][r].tolist()) for k in ROW_KEYS if not np.array_equal(trial[k][r], dev[k][r])}
            f = int(st["n_frames"][r])
            fam = case.get("families", [None] * cfg["R"])[r - cfg["row0"]]
            raise AssertionError(
                f"row {r} ({fam}): acceptable decisions {sorted(picks)[:8]}, device recorded code_0 "
                f"{dev['codes'][min(f, cfg['frame_cap'] - 1), r, 0]}; params {SR._row_params(cfg, r, True)}, n_past "
                f"{st['n_past'][r]}, n_text {st['n_text'][r]}, n_frames {f}, done {st['done'][r]}; (expected, device) {diff}")
        if counts is not None and not SR.is_greedy(SR._row_params(cfg, r, True)["temperature"]):
            counts[0] += len(picks) > 1
            counts[1] += 1
    for k in exp:   # rows the launch does not own included
        np.testing.assert_array_equal(dev[k], exp[k], err_msg=k)
    return dev


def run_cp(lib, logits, codes, n_frames, cfg, epi=None):
    """epi: None, or dict(kind=1, H, next_table, next_qkv=None, gamma=None) / dict(kind=2, H, talker_emb, cp_tables [G][V][H],
    pad, gamma=None, text_rows [RT][text_cap][H] = None).  cfg["held"] / cfg["text_avail"] + cfg["text_cap"] / text_rows send
    the launch through q3t_cp_sample_text_case.  -> (rc, codes, outputs dict); outputs start as sentinels so untouched rows show."""
    RT, V = logits.shape
    logits = np.ascontiguousarray(logits, np.float32)
    codes = np.array(codes, np.int32, copy=True)
    n_frames = np.ascontiguousarray(n_frames, np.int32)
    forced, seed_ptr = cfg.get("forced"), cfg.get("seed_ptr")
    keep, slots = _slots_array(cfg.get("slots"))
    out = {}
    kind, H, qkv_ld = 0, 0, 0
    tab = qkv = gamma = temb = cpt = pad = None
    if epi:
        kind, H = epi["kind"], epi["H"]
        out["h"] = np.full((RT, H), 777.0, np.float32)
        out["ssq"] = np.full((RT, H // 16), 777.0, np.float32)
        gamma = epi.get("gamma")
        if gamma is not None:
            out["xh"] = np.full((RT, H), 0x1234, np.uint16)
        if kind == 1:
            tab, qkv = epi["next_table"], epi.get("next_qkv")
            if qkv is not None:
                qkv_ld = qkv.shape[1]
                out["qkv"] = np.full((RT, qkv_ld), 777.0, np.float32)
        else:
            temb, cpt, pad = epi["talker_emb"], np.ascontiguousarray(epi["cp_tables"], np.float32), epi.get("pad")
    trows = epi.get("text_rows") if epi else None
    ta, held = cfg.get("text_avail"), cfg.get("held")
    text = trows is not None or ta is not None or held is not None
    ta = None if ta is None else np.ascontiguousarray(ta, np.int32)
    held = None if held is None else np.ascontiguousarray(held, np.int32)
    extra = (_opt(trows, hiplib.fptr), _opt(ta, hiplib.iptr), cfg.get("text_cap", 0), _opt(held, hiplib.iptr)) if text else ()
    rc = (lib.q3t_cp_sample_text_case if text else lib.q3t_cp_sample_case)(
        hiplib.fptr(logits), V, RT, cfg["row0"], cfg["R"], cfg["group"], hiplib.iptr(codes), hiplib.iptr(n_frames),
        cfg["frame_cap"], _opt(forced, hiplib.iptr), cfg.get("temperature", 0.0), cfg.get("top_k", 50), cfg.get("seed", 0),
        None if seed_ptr is None else seed_ptr.ctypes.data_as(U64P), slots, kind, H, _opt(tab, hiplib.fptr),
        _opt(qkv, hiplib.fptr), qkv_ld, _opt(gamma, hiplib.fptr), _opt(temb, hiplib.fptr), 0 if temb is None else temb.shape[0],
        _opt(cpt, hiplib.fptr), 0 if cpt is None else cpt.shape[0], _opt(pad, hiplib.fptr), _opt(out.get("h"), hiplib.fptr),
        _opt(out.get("ssq"), hiplib.fptr), None if "xh" not in out else out["xh"].ctypes.data_as(U16P),
        _opt(out.get("qkv"), hiplib.fptr), *extra)
    return rc, codes, out


def check_cp(lib, case, epi=None, counts=None):
    logits, codes, n_frames, cfg = case["logits"], case["codes"], case["n_frames"], case["cfg"]
    rc, dcodes, out = run_cp(lib, logits, codes, n_frames, cfg, epi)
    assert rc == 0, f"launch refused: {rc}"
    sets = SR.cp_sets(logits, n_frames, cfg)
    exp = np.array(codes, copy=True)
    g = cfg["group"]
    rows = range(cfg["row0"], cfg["row0"] + cfg["R"])
    used = {}
    for r in rows:
        if SR.cp_held(cfg, r):   # no decision: the row continues with the id its frame records, and stores nothing
            used[r] = SR.cp_apply_row(exp, n_frames, cfg, r, None)
            continue
        picks = sets[r]
        f, keep = SR.cp_frame(n_frames[r], cfg["frame_cap"])
        got = int(dcodes[f, r, 1 + g]) if keep else None
        fam = case.get("families", [None] * cfg["R"])[r - cfg["row0"]]
        if keep:
            assert got in picks, (f"row {r} ({fam}): device {got}, acceptable {sorted(picks)[:8]}; params "
                                  f"{SR._row_params(cfg, r, False)}, group {g}, n_frames {n_frames[r]}")
        elif epi is None or len(picks) == 1:
            got = min(picks)
        else:   # not recorded: the decision shows only in the gathered row
            got = next((c for c in sorted(picks) if _epi_matches(out, epi, exp, n_frames, cfg, r, c)), min(picks))
        used[r] = SR.cp_apply_row(exp, n_frames, cfg, r, got)
        if counts is not None and not SR.is_greedy(SR._row_params(cfg, r, False)["temperature"]):
            counts[0] += len(picks) > 1
            counts[1] += 1
    np.testing.assert_array_equal(dcodes, exp)
    if epi:
        H = epi["H"]
        for r in range(logits.shape[0]):
            if r not in used:   # sentinels: untouched
                assert (out["h"][r] == 777.0).all() and (out["ssq"][r] == 777.0).all(), f"row {r} written"
                assert "xh" not in out or (out["xh"][r] == 0x1234).all()
                assert "qkv" not in out or (out["qkv"][r] == 777.0).all()
                continue
            want = _epi_row(epi, exp, n_frames, cfg, r, used[r])
            np.testing.assert_array_equal(out["h"][r].view(np.uint32), want.view(np.uint32), err_msg=f"h_out row {r}")
            ssq = SR.ssq_parts(want)
            tol = (H + 4) * 2.0 ** -23 * ssq
            assert (np.abs(out["ssq"][r].astype(np.float64) - ssq) <= tol).all(), f"ssq_out row {r}"
            if "xh" in out:
                xw = SR.xh_row(want, epi["gamma"])
                err = np.abs(out["xh"][r].view(np.float16).astype(np.float64) - xw)
                assert (err <= SR.fp16_ulp(xw)).all(), f"xh_out row {r}: {err.max()}"
            if "qkv" in out:
                qw = SR.gather_row(epi["next_qkv"], used[r])
                np.testing.assert_array_equal(out["qkv"][r].view(np.uint32), qw.view(np.uint32), err_msg=f"qkv_out row {r}")
    return dcodes, out


def _epi_row(epi, codes_after, n_frames, cfg, r, used):
    if epi["kind"] == 1:
        return SR.gather_row(epi["next_table"], used)
    ids = SR.cp_feedback_codes(codes_after, n_frames, cfg, r, used)
    last = epi.get("pad")
    if epi.get("text_rows") is not None and cfg.get("slots") is not None:
        last = SR.feedback_last(last, epi["text_rows"][r], cfg["text_avail"][r], n_frames[r])
    return SR.feedback_row(ids, epi["talker_emb"], list(epi["cp_tables"]), last)


def _epi_matches(out, epi, codes, n_frames, cfg, r, code):
    trial = np.array(codes, copy=True)
    used = SR.cp_apply_row(trial, n_frames, cfg, r, code)
    return np.array_equal(out["h"][r], _epi_row(epi, trial, n_frames, cfg, r, used))


def _report(name, counts):
    a, n = counts
    print(f"{name}: {a} of {n} stochastic cases have more than one acceptable pick")
    assert n > 0 and a <= 0.05 * n


# ---- decisions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots_mode", [0, 1], ids=["scalar", "slots"])
@pytest.mark.parametrize("V", sorted(SC.TALKER_VOCABS))
def test_talker_decisions(test_lib, V, slots_mode):
    counts = [0, 0]
    cases = SC.talker_decision_cases(V, slots_mode)
    for case in cases:
        check_talker(test_lib, case, counts)
    shares = SC.ambiguous_share(cases, lambda c: {r: s for r, (s, _) in SR.talker_sets(c["logits"], c["st"], c["cfg"]).items()})
    SC.share_report(f"talker V={V} {'slots' if slots_mode else 'scalar'}", shares)
    assert all(a <= 0.05 * n for a, n in shares.values())
    _report("talker decisions", counts)


@pytest.mark.parametrize("slots_mode", [0, 1], ids=["scalar", "slots"])
@pytest.mark.parametrize("V", SC.CP_VOCABS)
def test_cp_decisions(test_lib, V, slots_mode):
    counts = [0, 0]
    cases = SC.cp_decision_cases(V, slots_mode)
    assert {c["cfg"]["group"] for c in cases} == set(range(15))
    for case in cases:
        check_cp(test_lib, case, counts=counts)
    shares = SC.ambiguous_share(cases, lambda c: SR.cp_sets(c["logits"], c["n_frames"], c["cfg"]))
    SC.share_report(f"cp V={V} {'slots' if slots_mode else 'scalar'}", shares)
    assert all(a <= 0.05 * n for a, n in shares.values())
    _report("cp decisions", counts)


@pytest.mark.parametrize("kernel", ["talker", "cp"])
def test_selection_and_sort_paths_agree_at_64_65(test_lib, kernel):
    """top_k = 64 takes the selection rounds, 65 the bitonic sort: on rows whose 65th entry weighs less than gamma the
    two must draw the same id."""
    V, R = (2152, 24) if kernel == "talker" else (2048, 24)
    rng = SC.rng_for("64/65", kernel)
    n_live = SC.TALKER_VOCABS[V][0] if kernel == "talker" else V
    # twice the spread of the decision tests (sampled at T = 1): the 65th of ~2000 normal entries then weighs ~e^-25
    logits = np.stack([SC.make_logits(("normal", "ties")[i % 2], rng, V, n_live, 64, 2.0) for i in range(R)])
    picks = {}
    same = 0
    for tk in (64, 65):
        if kernel == "talker":
            st = SC.talker_state(SC.rng_for("64/65 state"), R, V, n_live)
            st["n_text"][:] = 0
            cfg = dict(V=V, audio_vocab=n_live, eos=SC.TALKER_VOCABS[V][1], frame_cap=SC.FRAME_CAP, row0=0, R=R, temperature=1.0,
                       top_k=tk, top_p=1.0, seed=11)
            dev = check_talker(test_lib, dict(logits=logits, st=st, cfg=cfg))
            sets = {r: s for r, (s, _) in SR.talker_sets(logits, st, cfg).items()}
            picks[tk] = [int(dev["codes"][min(int(st["n_frames"][r]), SC.FRAME_CAP - 1), r, 0]) for r in range(R)]
            proc = [SR.talker_sets(logits, st, cfg)[r][1] for r in range(R)]
        else:
            nf = np.ones(R, np.int32)
            cfg = dict(V=V, frame_cap=SC.FRAME_CAP, row0=0, R=R, group=3, temperature=1.0, top_k=tk, seed=11)
            codes, _ = check_cp(test_lib, dict(logits=logits, codes=np.full((SC.FRAME_CAP, R, 16), -7, np.int32), n_frames=nf, cfg=cfg))
            sets = SR.cp_sets(logits, nf, cfg)
            picks[tk] = [int(codes[0, r, 4]) for r in range(R)]
            proc = list(logits)
        picks[tk, "sets"] = sets
    for r in range(R):
        order, key = SR.kept_order(proc[r], 65)
        w = np.exp(key[order] - key[order[0]])
        assert w[64] / w.sum() < (65 + 4) * 2.0 ** -23, "the 65th entry must weigh less than gamma"
        if len(picks[64, "sets"][r]) == 1 and len(picks[65, "sets"][r]) == 1:
            assert picks[64][r] == picks[65][r], f"row {r}: top_k 64 drew {picks[64][r]}, top_k 65 drew {picks[65][r]}"
            same += 1
    print(f"{kernel}: {same} of {R} rows unambiguous under both")
    assert same >= R - 2


def test_top_p_cut_on_exact_equality(test_lib):
    """Inputs on which the device's fp32 arithmetic is exact: m tied finite entries (weights exactly 1, sums small
    integers), nothing else above -1e10, top_p = 0.5.  The kept prefix is searchsorted(cumsum, 0.5) + 1 = m / 2 entries
    (cumsum reaches 0.5 exactly there, and >= keeps it) -- one entry fewer than a strict comparison would keep, so draws
    with u in the upper part land on another id.  No error band applies; the pick is the reference's with gamma = 0."""
    V, (av, eos) = 100, SC.TALKER_VOCABS[100]
    rng = SC.rng_for("top-p equality")
    rows = []
    for m in (2, 4, 8):
        for top_k in (50, 0):          # selection path and sort path
            for _ in range(6):
                ids = np.sort(rng.choice(av, size=m, replace=False))
                l = np.full(V, -np.inf, np.float32)
                l[ids] = 1.5
                rows.append((l, m, top_k, ids))
    R = len(rows)
    logits = np.stack([r[0] for r in rows])
    st = SC.talker_state(rng, R, V, av)
    st["n_past"][:] = 0
    st["n_text"][:] = 0
    slots = [SC.slot(t_temp=1.0, t_top_k=tk, t_top_p=0.5, seed=1000 + i, no_row=i % 2) for i, (_, _, tk, _) in enumerate(rows)]
    cfg = dict(V=V, audio_vocab=av, eos=eos, frame_cap=SC.FRAME_CAP, row0=0, R=R, slots=slots)
    rc, dev = run_talker(test_lib, logits, st, cfg)
    assert rc == 0
    upper = 0
    for r, (_, m, tk, ids) in enumerate(rows):
        u = SR.uniform01(slots[r]["seed"], 0 if slots[r]["no_row"] else r, int(st["n_frames"][r]), 0)
        want = int(ids[min(int(u * (m // 2)), m // 2 - 1)])      # uniform over the m / 2 lowest indices
        got = int(dev["codes"][int(st["n_frames"][r]), r, 0])
        assert got == want, f"row {r}: {m} tied entries {ids}, top_k {tk}, u {u}: device {got}, reference {want}"
        upper += u >= 0.5
    assert upper >= R // 4     # rows on which a strict comparison would have drawn from the upper half


# ---- talker pre-processing (greedy: exact) ------------------------------------------------------------------------
def _ring_from(chron):
    ring = np.zeros(32, np.int32)
    for i in range(max(0, len(chron) - 32), len(chron)):
        ring[i % 32] = chron[i]
    return ring


def _preprocessing_rows(V, av, eos):
    """-> list of (logits, chronological past, n_text, note).  a = the arg-max of the raw logits, b the runner-up:
    a penalised (or EOS boosted) changes the winner, so a wrong window or threshold shows in the recorded id."""
    rng = SC.rng_for("pre", V)
    rows = []
    a, b = 5, av - 3
    filler = [i for i in range(av) if i not in (a, b)]

    def base(va, vb, rest=-50.0):
        l = (rest + rng.random(V)).astype(np.float32)
        l[a], l[b] = va, vb
        return l
    for n_past in (0, 1, 29, 30, 31, 32, 33, 64, 100):
        # a at: the most recent slot, the oldest one inside the window, the newest one outside it, nowhere
        for where in ("recent", "inside", "outside", "absent"):
            chron = [int(x) for x in rng.choice(filler, size=n_past)]
            at = {"recent": n_past - 1, "inside": n_past - 30, "outside": n_past - 31, "absent": -1}[where]
            if where != "absent" and (at < 0 or at < n_past - 32):
                continue
            if at >= 0:
                chron[at] = a
            for va, vb in ((5.0, 4.5), (-1.0, -1.1), (0.0, -0.05)):      # positive: / 1.2, negative: * 1.2, zero: unchanged
                rows.append((base(va, vb), chron, 0, f"n_past {n_past} {where} {va}"))
    # the repeated id is EOS (its logit is penalised like any other)
    for va in (5.0, -1.0):
        l = base(va - 0.4 * abs(va), va - 0.45 * abs(va))
        l[eos] = va
        rows.append((l, [eos, 7, 9], 0, "eos repeated"))
        rows.append((l, [7, 9], 0, "eos not repeated"))
    # EOS boost: min((progress - 0.8) / 0.7, 1) * 15 once progress = n_past / (3 n_text) > 0.8; forced beyond 2
    for n_text, n_past, gap in ((5, 12, 1.0), (5, 13, 1.0), (7, 16, 0.1), (7, 17, 0.1), (5, 22, 14.6), (5, 23, 14.6), (5, 30, 20.0),
                                (5, 31, 20.0), (0, 40, 1.0), (1, 3, 16.0), (1, 7, 50.0)):
        l = base(5.0, 4.0)
        l[eos] = 5.0 - gap
        rows.append((l, [int(x) for x in rng.choice(filler, size=n_past)], n_text, f"progress {n_past}/{3 * n_text}"))
    # nothing audible: the winner is the first masked id (>= audio_vocab), which ends the row
    l = np.full(V, -np.inf, np.float32)
    rows.append((l, [], 3, "winner >= audio_vocab"))
    l = base(5.0, 4.0)
    l[av + 1] = 100.0      # masked, must not win
    l[V - 1] = np.nan      # masked as well
    rows.append((l, [], 3, "masked ids lose"))
    return rows


@pytest.mark.parametrize("slots_mode", [0, 1], ids=["scalar", "slots"])
@pytest.mark.parametrize("ignore_eos", [0, 1])
@pytest.mark.parametrize("V", [100, 2152])
def test_talker_preprocessing(test_lib, V, ignore_eos, slots_mode):
    av, eos = SC.TALKER_VOCABS[V]
    rows = _preprocessing_rows(V, av, eos)
    R = len(rows)
    st = SC.talker_state(SC.rng_for("pre state"), R, V, av, frame_cap=2)
    st["n_frames"][:] = 0
    for r, (_, chron, n_text, _) in enumerate(rows):
        st["past"][r] = _ring_from(chron)
        st["n_past"][r] = len(chron)
        st["n_text"][r] = n_text
    cfg = dict(V=V, audio_vocab=av, eos=eos, ignore_eos=bool(ignore_eos), frame_cap=2, row0=0, R=R, temperature=0.0)
    if slots_mode:
        cfg["slots"] = [SC.slot(t_temp=0.0, seed=r) for r in range(R)]
    case = dict(logits=np.stack([r[0] for r in rows]), st=st, cfg=cfg, families=[r[3] for r in rows])
    dev = check_talker(test_lib, case)
    # the cases do what they were built for: both outcomes occur
    ended = int(dev["done"].sum())
    assert 0 < ended < R
    if not ignore_eos:
        rec = {note: int(dev["codes"][0, r, 0]) for r, (_, _, _, note) in enumerate(rows)}
        assert rec["n_past 31 inside 5.0"] == av - 3 and rec["n_past 31 outside 5.0"] == 5
        assert rec["n_past 33 inside 5.0"] == av - 3 and rec["n_past 33 outside 5.0"] == 5
        assert rec["progress 12/15"] == 5 and rec["progress 13/15"] == -1
        assert rec["progress 22/15"] == 5 and rec["progress 23/15"] == -1
        assert rec["progress 30/15"] == 5 and rec["progress 31/15"] == -1


# ---- state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots_mode", [0, 1], ids=["scalar", "slots"])
@pytest.mark.parametrize("stochastic", [0, 1])
def test_talker_state_transitions(test_lib, slots_mode, stochastic):
    """frame_cap edges, rows that were done, frame budget, teacher forcing, rows outside the launch."""
    V, (av, eos) = 100, SC.TALKER_VOCABS[100]
    cap = 4
    rng = SC.rng_for("talker state", slots_mode, stochastic)
    spec = [(nf, done, ends) for nf in (0, cap - 1, cap, cap + 1, cap + 2) for done in (0, 1) for ends in (0, 1)]
    spec = [s + (budget,) for s in spec for budget in (0, 1, 2)]     # none / reached (n_past = max_frames) / one frame left
    R, row0 = len(spec), 3
    RT = R + 5
    st = SC.talker_state(rng, RT, V, av, frame_cap=cap)
    st["n_text"][:] = 0
    st["n_past"][:] = 20
    logits = (3.0 * rng.standard_normal((RT, V))).astype(np.float32)
    forced = np.full((cap, RT, 16), -1, np.int32)
    forced[:, ::2, 0] = rng.integers(0, av, (cap, (RT + 1) // 2))
    slots = [SC.slot(t_temp=0.8 * stochastic, t_top_k=5, t_top_p=0.9, seed=77 + r, no_row=r % 2) for r in range(RT)]
    for i, (nf, done, ends, budget) in enumerate(spec):
        r = row0 + i
        st["n_frames"][r], st["done"][r] = nf, done
        logits[r, eos if ends else 11] = 60.0      # the arg-max is EOS / an audio id
        slots[r]["max_frames"] = 0 if budget == 0 else 20 + budget - 1
    cfg = dict(V=V, audio_vocab=av, eos=eos, frame_cap=cap, row0=row0, R=R, R_total=RT, forced=forced,
               temperature=0.8 * stochastic, top_k=5, top_p=0.9, seed=5)
    if slots_mode:
        check_talker(test_lib, dict(logits=logits, st=st, cfg=dict(cfg, slots=slots)))
    else:   # the budget is a launch scalar: one launch per value
        for budget in (0, 1, 2):
            check_talker(test_lib, dict(logits=logits, st=st, cfg=dict(cfg, max_frames=0 if budget == 0 else 20 + budget - 1)))


def _cp_state_case(rng, V, cap, slots_mode, stochastic):
    spec = [(nf, fz) for nf in (0, 1, cap - 1, cap, cap + 1, cap + 2) for fz in (-1, 3, V + 5)]
    R, row0 = len(spec), 2
    RT = R + 3
    logits = (3.0 * rng.standard_normal((RT, V))).astype(np.float32)
    n_frames = rng.integers(0, cap, RT).astype(np.int32)
    codes = rng.integers(-1, V + 2, (cap, RT, 16)).astype(np.int32)     # ids in range, -1 and >= vocab
    forced = np.full((cap, RT, 16), -1, np.int32)
    g = int(rng.integers(0, 15))
    for i, (nf, fz) in enumerate(spec):
        n_frames[row0 + i] = nf
        forced[:, row0 + i, 1 + g] = fz
        forced[:, row0 + i, 1 + (g + 1) % 15] = (-1, 2)[i % 2]      # another group's forced id: feeds the feedback sum only
        forced[:, row0 + i, 0] = (-1, 4)[(i // 2) % 2]
    cfg = dict(V=V, frame_cap=cap, row0=row0, R=R, R_total=RT, group=g, forced=forced, temperature=0.8 * stochastic, top_k=5, seed=9)
    if slots_mode:
        cfg["slots"] = [SC.slot(c_temp=0.8 * stochastic, c_top_k=5, seed=31 + r, no_row=r % 2) for r in range(RT)]
    return dict(logits=logits, codes=codes, n_frames=n_frames, cfg=cfg)


@pytest.mark.parametrize("slots_mode", [0, 1], ids=["scalar", "slots"])
@pytest.mark.parametrize("stochastic", [0, 1])
def test_cp_state_transitions(test_lib, slots_mode, stochastic):
    """n_frames = 0 clamps to frame 0; frames at and beyond frame_cap are not recorded; a forced id continues the
    stream while codes keeps the decision; rows outside the launch are untouched."""
    rng = SC.rng_for("cp state", slots_mode, stochastic)
    case = _cp_state_case(rng, 64, 4, slots_mode, stochastic)
    check_cp(test_lib, case)
    table = rng.standard_normal((64, 64)).astype(np.float32)
    check_cp(test_lib, case, dict(kind=1, H=64, next_table=table))


# ---- gather / feedback epilogue ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("qkv_ld", [0, 192, 4096, 4608])
@pytest.mark.parametrize("H", [64, 1024, 1536])
def test_cp_gather_epilogue(test_lib, H, qkv_ld):
    """h_out / qkv_out rows bit-equal the table rows of the id the stream continues with (zeros for a forced id >= V);
    ssq_out within (H + 4) * 2^-23 of float64, xh_out within one fp16 ulp.  H = 1536 and qkv_ld = 4608 reach the
    tail loops of the next_qkv branch."""
    V = 64
    rng = SC.rng_for("gather", H, qkv_ld)
    case = _cp_state_case(rng, V, 4, slots_mode=H == 1024, stochastic=qkv_ld == 192)
    table = (rng.standard_normal((V, H)) * 10.0 ** rng.uniform(-3, 3, (V, 1))).astype(np.float32)
    epi = dict(kind=1, H=H, next_table=table, gamma=(1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32))
    if qkv_ld:
        epi["next_qkv"] = rng.standard_normal((V, qkv_ld)).astype(np.float32)
    _, out = check_cp(test_lib, case, epi)
    assert (out["h"][case["cfg"]["row0"]:case["cfg"]["row0"] + case["cfg"]["R"]] == 0).all(axis=1).any(), "no forced id >= V row"
    check_cp(test_lib, case, dict(epi, gamma=None))     # without the pre-scaled copy


@pytest.mark.parametrize("H", [64, 1024, 1536])
def test_cp_feedback_epilogue(test_lib, H):
    """The feedback sum over ids in range, -1 and >= vocab: sequential f32 adds in the documented order, bit-equal."""
    V, TV = 64, 100
    rng = SC.rng_for("feedback", H)
    for pad_on in (1, 0):
        case = _cp_state_case(rng, V, 4, slots_mode=pad_on, stochastic=1 - pad_on)
        case["codes"][:, :, 0] = rng.integers(-1, TV + 2, case["codes"].shape[:2])
        epi = dict(kind=2, H=H, talker_emb=rng.standard_normal((TV, H)).astype(np.float32),
                   cp_tables=rng.standard_normal((15, V, H)).astype(np.float32),
                   pad=rng.standard_normal(H).astype(np.float32) if pad_on else None,
                   gamma=(1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32) if pad_on else None)
        check_cp(test_lib, case, epi)


# ---- text slots: hold rule, EOS mask, held rows of the code predictor, text rows in the feedback ------------------------
def _launch_rows(case):
    return range(case["cfg"]["row0"], case["cfg"]["row0"] + case["cfg"]["R"])


@pytest.mark.parametrize("V", SC.TEXT_TALKER_VOCABS)
def test_talker_hold_grid(test_lib, V):
    """Every cell of the hold rule's hand grid (tests/test_sample_reference.py::test_hold_rule_hand_grid), 16 per launch
    of talker_sample_kernel_slots with text_avail and held.  EOS is on top of every row: a held row that decided
    anything would end.  A held row keeps its state bit for bit and held[] equals the reference on all 21 rows
    (check_talker); greedy and stochastic rows alternate."""
    counts = [0, 0]
    held_rows = free_flag3 = 0
    for case in SC.hold_grid_cases(V):
        st, cfg = case["st"], case["cfg"]
        dev = check_talker(test_lib, case, counts)
        for r in _launch_rows(case):
            if SR.talker_held(st, cfg, r):
                held_rows += 1
                assert dev["held"][r] == 1 and dev["done"][r] == 0 and dev["n_frames"][r] == st["n_frames"][r]
            else:
                assert dev["held"][r] == 0
                free_flag3 += cfg["slots"][r]["flags"] == 3
        outside = [r for r in range(cfg["R_total"]) if r not in _launch_rows(case)]
        assert (dev["held"][outside] == SC.HELD_SENTINEL).all()
    assert held_rows == 9 and free_flag3 >= 9
    _report("talker hold grid", counts)


@pytest.mark.parametrize("V", SC.TEXT_TALKER_VOCABS)
def test_talker_eos_mask(test_lib, V):
    """flags 2 and 3 with hold off: EOS on top, with and without forced EOS (progress > 2) -- the row continues with the
    best audio id; flags 0 and 1 end.  held[] (given, with text_avail null) stays untouched."""
    counts = [0, 0]
    av, eos = SC.TALKER_VOCABS[V]
    for case in SC.eos_mask_cases(V):
        st, cfg, logits = case["st"], case["cfg"], case["logits"]
        assert cfg["text_avail"] is None
        dev = check_talker(test_lib, case, counts)
        sets = SR.talker_sets(logits, st, cfg)
        kinds = set()
        for r in _launch_rows(case):
            fl, f = cfg["slots"][r]["flags"], int(st["n_frames"][r])
            forced = st["n_past"][r] / (3 * st["n_text"][r]) > 2
            assert int(np.argmax(logits[r])) == eos
            if fl & 2:
                code = int(dev["codes"][f, r, 0])
                assert dev["done"][r] == 0 and 0 <= code < av and code in sets[r][0]
                if SR.is_greedy(cfg["slots"][r]["t_temp"]):
                    assert code == SR.first_argmax(sets[r][1][:av])
            else:
                assert dev["done"][r] == 1 and dev["codes"][f, r, 0] == -1
            kinds.add((fl, bool(forced), SR.is_greedy(cfg["slots"][r]["t_temp"])))
        assert len(kinds) == 16
        assert (dev["held"] == SC.HELD_SENTINEL).all()
    _report("talker EOS mask", counts)


def _text_epilogue(name, V, H, rng):
    gamma = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)
    if name == "none":
        return None
    if name.startswith("gather"):
        epi = dict(kind=1, H=H, next_table=rng.standard_normal((V, H), dtype=np.float32), gamma=gamma)
        if name == "gather_qkv":
            epi["next_qkv"] = rng.standard_normal((V, 192), dtype=np.float32)
        return epi
    return dict(kind=2, H=H, talker_emb=rng.standard_normal((100, H), dtype=np.float32),
                cp_tables=rng.standard_normal((15, V, H), dtype=np.float32), pad=rng.standard_normal(H, dtype=np.float32), gamma=gamma)


@pytest.mark.parametrize("epilogue", ["none", "gather", "gather_qkv", "feedback"])
@pytest.mark.parametrize("V", SC.TEXT_CP_VOCABS)
def test_cp_held_rows(test_lib, V, epilogue):
    """A held row of cp_argmax_kernel_slots leaves codes untouched and continues with the id its frame records (0 for -1 and
    for an id beyond the vocabulary; the teacher-forced id where one is given), whatever its logits say: h_out bit-equal,
    ssq_out / xh_out / qkv_out as check_cp grades them, built from that id.  Free rows of the same launch decide as ever."""
    H = 1024 if V == 64 else 96
    counts = [0, 0]
    for case in SC.cp_held_cases(V):
        cfg, g = case["cfg"], case["cfg"]["group"]
        epi = _text_epilogue(epilogue, V, H, SC.rng_for("held epi", V, epilogue))
        dcodes, _ = check_cp(test_lib, case, epi, counts)
        recorded = set()
        for r in _launch_rows(case):
            f = int(case["n_frames"][r]) - 1
            if cfg["held"][r]:
                rec = int(case["codes"][f, r, 1 + g])
                recorded.add("in" if 0 <= rec < V else rec)
                assert dcodes[f, r, 1 + g] == rec
                assert SR.first_argmax(case["logits"][r]) != (rec if 0 <= rec < V else 0), "a fresh decision must differ"
            else:
                assert dcodes[f, r, 1 + g] in SR.cp_sets(case["logits"], case["n_frames"], cfg)[r]
        assert recorded == {"in", -1, V + 5}
    _report("cp held rows", counts)


@pytest.mark.parametrize("H", [96, 1024])
@pytest.mark.parametrize("V", SC.TEXT_CP_VOCABS)
def test_cp_feedback_text_rows(test_lib, V, H):
    """The feedback sum's last addend: text_rows[r][n_frames - 1] while n_frames - 1 < text_avail[r], pad otherwise (also on
    flags-0 rows, as CpArgmaxArgs documents; also where the codes' frame is clamped to frame_cap - 1).  Every text row
    and the pad are distinct random rows; h_out is bit-equal to sample_ref.feedback_row."""
    rng = SC.rng_for("text rows", V, H)
    epi = _text_epilogue("feedback", V, H, rng)
    epi["text_rows"] = rng.standard_normal((SC.TEXT_RT, SC.TEXT_CAP, H), dtype=np.float32)
    counts = [0, 0]
    seen = set()
    for case in SC.text_row_cases(V):
        cfg = case["cfg"]
        check_cp(test_lib, case, epi, counts)
        for r in _launch_rows(case):
            last = SR.feedback_last(None, epi["text_rows"][r], cfg["text_avail"][r], case["n_frames"][r])
            seen.add((last is not None, cfg["slots"][r]["flags"] & 1, int(case["n_frames"][r]) - 1 >= cfg["frame_cap"]))
    assert seen == {(t, f, c) for t in (False, True) for f in (0, 1) for c in (False, True)}
    _report("cp text rows", counts)


def test_sampler_launchers_refuse_inconsistent_text_arguments(test_lib):
    """text_avail without held, either of them without per-slot mode (talker); text_rows / text_avail / held without
    per-slot mode, text_rows without text_avail or with text_cap = 0 (code predictor): -1, and nothing changes."""
    V = 64
    case = SC.hold_grid_cases(V)[0]
    st, cfg = case["st"], case["cfg"]
    no_held = {k: v for k, v in st.items() if k != "held"}
    scalar = dict(cfg, slots=None, temperature=0.0)
    for state, c in ((no_held, cfg), (st, scalar), (no_held, scalar), (st, dict(scalar, text_avail=None))):
        rc, dev = run_talker(test_lib, case["logits"], state, c)
        assert rc == -1
        for k in state:
            np.testing.assert_array_equal(dev[k], state[k], err_msg=k)
    rc, _ = run_talker(test_lib, case["logits"], st, cfg)        # the consistent set is served
    assert rc == 0
    case = SC.text_row_cases(V)[0]
    cfg = case["cfg"]
    H = 96
    epi = _text_epilogue("feedback", V, H, SC.rng_for("refusals"))
    epi["text_rows"] = np.zeros((SC.TEXT_RT, SC.TEXT_CAP, H), np.float32)
    held = np.zeros(SC.TEXT_RT, np.int32)
    scalar = dict(cfg, slots=None, temperature=0.0)
    no_text = dict(epi, text_rows=None)
    bad = [(scalar, epi), (scalar, no_text), (dict(scalar, text_avail=None, text_cap=0, held=held), no_text),
           (dict(cfg, text_avail=None), epi), (dict(cfg, text_cap=0), epi), (dict(cfg, text_cap=-1), epi)]
    for c, e in bad:
        rc, got, out = run_cp(test_lib, case["logits"], case["codes"], case["n_frames"], c, e)
        assert rc == -1
        np.testing.assert_array_equal(got, case["codes"])
        assert (out["h"] == 777.0).all() and (out["ssq"] == 777.0).all()
    rc, _, _ = run_cp(test_lib, case["logits"], case["codes"], case["n_frames"], cfg, epi)
    assert rc == 0
    rc, _, _ = run_cp(test_lib, case["logits"], case["codes"], case["n_frames"], dict(cfg, held=held), no_text)
    assert rc == 0


# ---- what the launcher refuses ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2050, 63, 2049])
def test_cp_refuses_vocabulary_not_a_multiple_of_4(test_lib, V):
    """cp_argmax reads each row as V / 4 float4: a tail would be dropped silently (and odd rows misaligned), so the
    launcher refuses such a vocabulary.  Regression test: it used to accept it and never look at the last ids."""
    logits = np.zeros((2, V), np.float32)
    logits[:, V - 1] = 9.0       # the winner sits in the tail
    codes = np.full((1, 2, 16), -7, np.int32)
    cfg = dict(V=V, frame_cap=1, row0=0, R=2, group=0)
    rc, got, _ = run_cp(test_lib, logits, codes, np.ones(2, np.int32), cfg)
    assert rc == -1
    np.testing.assert_array_equal(got, codes)
    V4 = V // 4 * 4                # the same rows cut to a multiple of 4 are served
    rc, got, _ = run_cp(test_lib, logits[:, :V4], codes, np.ones(2, np.int32), dict(cfg, V=V4))
    assert rc == 0
    assert got[0, :, 1].tolist() == [0, 0]
