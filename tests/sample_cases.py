"""Seeded inputs of the sampling-decision tests -- shared by tests/test_sample_reference.py (which checks, from the
reference alone, that at most 5 % of the stochastic cases of every family are ambiguous) and
tests/test_gpu_sample_decisions.py (which runs the same cases on the device).  One case = one launch of many rows."""
from __future__ import annotations

import zlib

import numpy as np

from tests import sample_ref as SR

TALKER_VOCABS = {64: (48, 50), 100: (78, 90), 2152: (2048, 2150), 3072: (2048, 2150), 4096: (2048, 2150)}  # V: (audio_vocab, eos)
CP_VOCABS = (64, 2048, 2052, 4096)
JUST_ABOVE = float(np.nextafter(np.float32(1e-6), np.float32(1.0)))   # the smallest stochastic temperature
TEMPS = (1e-6, JUST_ABOVE, 0.5, 1.0, 5.0)
TOP_PS = (1e-6, 0.5, 0.95, 1.0, 0.0, 1.5)
SEEDS = (0, 2 ** 64 - 1, 0x1234567890ABCDEF, 7)
FRAMES = (0, 1, 5)
FAMILIES = ("normal", "ties", "flat_top", "few_finite", "all_ninf", "nan_top", "inf_top")
FRAME_CAP = 8
# logits = spread * T * N(0, 1): the weights are exp(spread * (z - z_max)) at every temperature.  With gamma =
# (n + 4) * 2^-23 a case is ambiguous when u lands within gamma of one of the boundaries that are further than gamma apart,
# so the share is about 2 * gamma * (entries heavier than gamma); at n = 4096 (gamma = 4.9e-4) a spread of 10 leaves about a
# dozen such entries (z > z_max - ln(1/gamma) / 10), i.e. ~1 %; a flat distribution would have all 4096.
SPREAD = 10.0


def top_ks(V):
    return (1, 2, 50, 64, 65, 500, V - 1, V, V + 1, 0, -3)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def make_logits(family, rng, V, n_live, top_k, temperature, eos_finite=0):
    """One row of float32 logits.  n_live: ids below it take part (the talker masks the others); top_k tells where the
    planted ties go; eos_finite: see talker_decision_cases."""
    scale = SPREAD * (temperature if temperature >= 0.1 else 1.0)
    l = (scale * rng.standard_normal(V)).astype(np.float32)
    live = l[:n_live]
    k_eff = n_live if (top_k <= 0 or top_k > n_live) else top_k
    order = np.argsort(-live, kind="stable")
    if family == "ties":
        # the three heaviest entries tie (inside the kept set, where most draws land), and so do the ranks around the
        # top-k boundary
        live[order[:3]] = live[order[0]]
        if 3 < k_eff < n_live - 1:
            live[order[k_eff - 1:k_eff + 2]] = live[order[k_eff]]
    elif family == "flat_top":
        # one entry on top, then m + 2 equal ones, the others far below: the kept ones are the lowest indices of the tied
        # block, drawn uniformly in index order -- any other tie rule moves most picks.  (The heavier top entry keeps
        # the cumulative masses away from top_p = 1/2 and 19/20, which a flat block of 50 or 20 would hit exactly.)
        # Each of the m boundaries (1/m apart) is ambiguous over 2 * gamma of u: m <= 65 while gamma is that of <= 65
        # kept entries, 16 once top_k keeps more (gamma up to 4.9e-4).
        m = max(1, min(k_eff, 65, n_live - 3)) if k_eff <= 65 else 16
        live[order[1:m + 3]] = live[order[1]]
        live[order[0]] = live[order[1]] + np.float32(0.03 * scale)
        live[order[m + 3:]] -= np.float32(3.0 * scale)
    elif family == "few_finite":
        keep = rng.choice(n_live, size=min(3, n_live), replace=False)
        v = live[keep].copy()
        l[:] = -np.inf
        l[keep] = v
    elif family == "all_ninf":
        l[:] = -np.inf
        if eos_finite:
            l[eos_finite] = 0.0
    elif family == "nan_top":
        l[rng.choice(n_live, size=2, replace=False)] = np.nan
    elif family == "inf_top":
        l[rng.choice(n_live, size=2, replace=False)] = np.inf
    return l


def slot(max_frames=0, t_temp=0.0, t_top_k=0, t_top_p=1.0, c_temp=0.0, c_top_k=0, seed=0, no_row=1, flags=0):
    return dict(max_frames=max_frames, t_temp=t_temp, t_top_k=t_top_k, t_top_p=t_top_p, c_temp=c_temp, c_top_k=c_top_k,
                seed=seed, no_row=no_row, flags=flags)


def talker_state(rng, RT, V, audio_vocab, frame_cap=FRAME_CAP, sentinel=True):
    """A random but valid state: rings of audio ids, counters, and sentinels (-7) where a launch must write nothing."""
    n_past = rng.choice([0, 3, 31, 40], size=RT).astype(np.int32)
    return dict(past=rng.integers(0, audio_vocab, (RT, 32)).astype(np.int32), n_past=n_past,
                n_text=rng.choice([0, 7, 30], size=RT).astype(np.int32), done=np.zeros(RT, np.int32),
                n_frames=rng.choice(FRAMES, size=RT).astype(np.int32), pos0=rng.integers(5, 50, RT).astype(np.int32),
                pos=np.full(RT, -7, np.int32), codes=np.full((frame_cap, RT, 16), -7, np.int32))


def _param_grid(V, with_top_p):
    """(temperature, top_k, top_p) of the scalar-mode launches: every top_k, every temperature, every top_p."""
    tks = top_ks(V)
    grid = [((0.5, 1.0, 5.0)[i % 3], tk, (0.95, 1.0, 0.5)[i % 3]) for i, tk in enumerate(tks)]
    grid += [(T, tk, 0.95) for T in TEMPS for tk in (50, 65)]
    if with_top_p:
        grid += [(1.0, tk, tp) for tp in TOP_PS for tk in (50, 0)]
    return grid


def _families_rows(per_family):
    return [f for f in FAMILIES for _ in range(per_family)]


def talker_decision_cases(V, slots_mode, per_family=3):
    """Launches of len(FAMILIES) * per_family rows (+ untouched rows before and after).  Scalar mode: one parameter
    combination per launch, seeds from SEEDS or a per-row seed array.  Per-slot mode: every row draws its own combination.

    The talker's mask turns an all -inf row into a flat distribution over the ids >= audio_vocab (-1e10 each), which no
    error bound resolves once top_k keeps hundreds of them.  So a talker "all_ninf" row is all -inf only where top_k <= 65;
    beyond, EOS alone is finite (it then holds all the mass), and ignore_eos launches keep to top_k <= 65."""
    audio_vocab, eos = TALKER_VOCABS[V]
    fams = _families_rows(per_family)
    R, row0 = len(fams), 2
    RT = R + 3
    grid = _param_grid(V, True)
    cases = []
    for li, (T, tk, tp) in enumerate(grid):
        rng = rng_for("talker", V, slots_mode, li)
        st = talker_state(rng, RT, V, audio_vocab)
        cfg = dict(V=V, audio_vocab=audio_vocab, eos=eos, ignore_eos=bool(li % 5 == 4 and 0 < tk <= 65), rep_penalty=1.2, frame_cap=FRAME_CAP,
                   row0=row0, R=R, R_total=RT)
        logits = np.zeros((RT, V), np.float32)
        if slots_mode:
            cfg["slots"] = []
            for r in range(RT):
                cfg["slots"].append(slot(t_temp=TEMPS[rng.integers(5)], t_top_k=top_ks(V)[rng.integers(11)],
                                         t_top_p=TOP_PS[rng.integers(6)], c_temp=0.7, c_top_k=3,
                                         seed=SEEDS[rng.integers(4)] if rng.integers(3) else int(rng.integers(0, 2 ** 63)),
                                         no_row=int(rng.integers(2))))
        else:
            cfg.update(temperature=T, top_k=tk, top_p=tp, seed=SEEDS[li % 4])
            if li % 3 == 2:
                cfg["seed_ptr"] = rng.integers(0, 2 ** 63, RT).astype(np.uint64)
                cfg["seed_ptr"][row0] = 2 ** 64 - 1
        for i, fam in enumerate(fams):
            r = row0 + i
            p = SR._row_params(cfg, r, True)
            if slots_mode and cfg["ignore_eos"] and fam == "all_ninf":
                cfg["slots"][r]["t_top_k"] = p["top_k"] = (1, 2, 50, 64, 65)[rng.integers(5)]
            wide = p["top_k"] <= 0 or p["top_k"] > 65
            logits[r] = make_logits(fam, rng, V, audio_vocab, p["top_k"], p["temperature"], eos if wide else 0)
        cases.append(dict(logits=logits, st=st, cfg=cfg, families=fams))
    return cases


def cp_decision_cases(V, slots_mode, per_family=3):
    fams = _families_rows(per_family)
    R, row0 = len(fams), 2
    RT = R + 3
    grid = _param_grid(V, False)
    cases = []
    for li, (T, tk, _) in enumerate(grid):
        rng = rng_for("cp", V, slots_mode, li)
        cfg = dict(V=V, frame_cap=FRAME_CAP, row0=row0, R=R, R_total=RT, group=li % 15)
        if slots_mode:
            cfg["slots"] = []
            for r in range(RT):
                cfg["slots"].append(slot(c_temp=TEMPS[rng.integers(5)], c_top_k=top_ks(V)[rng.integers(11)], t_temp=0.7,
                                         t_top_k=3, t_top_p=0.5,
                                         seed=SEEDS[rng.integers(4)] if rng.integers(3) else int(rng.integers(0, 2 ** 63)),
                                         no_row=int(rng.integers(2))))
        else:
            cfg.update(temperature=T, top_k=tk, seed=SEEDS[li % 4])
            if li % 3 == 2:
                cfg["seed_ptr"] = rng.integers(0, 2 ** 63, RT).astype(np.uint64)
                cfg["seed_ptr"][row0] = 2 ** 64 - 1
        logits = np.zeros((RT, V), np.float32)
        for i, fam in enumerate(fams):
            r = row0 + i
            p = SR._row_params(cfg, r, False)
            logits[r] = make_logits(fam, rng, V, V, p["top_k"], p["temperature"])
        cases.append(dict(logits=logits, cfg=cfg, families=fams, n_frames=rng.choice(FRAMES, size=RT).astype(np.int32),
                          codes=np.full((FRAME_CAP, RT, 16), -7, np.int32)))
    return cases


def ambiguous_share(cases, sets_of):
    """-> {family: (ambiguous, stochastic)} over the rows of `cases`; sets_of(case) -> {row: set}."""
    out = {}
    for c in cases:
        sets = sets_of(c)
        for i, fam in enumerate(c["families"]):
            r = c["cfg"]["row0"] + i
            p = SR._row_params(c["cfg"], r, "st" in c)
            if SR.is_greedy(p["temperature"]) or r not in sets:      # (a held row makes no draw)
                continue
            a, n = out.get(fam, (0, 0))
            out[fam] = (a + (len(sets[r]) > 1), n + 1)
    return out


def share_report(name, shares):
    txt = ", ".join(f"{f} {a}/{n}" for f, (a, n) in shares.items())
    print(f"ambiguous share {name}: {txt}")
    return txt


# ---- text slots: hold rule, EOS mask, held rows in the code predictor, text rows in the feedback ---------------------
# One case per row, TEXT_R rows per launch between untouched rows; a list longer than a launch is cut into launches
# (the last one filled up from the start of the list).  Even rows are greedy, odd rows stochastic.
TEXT_RT, TEXT_ROW0, TEXT_R = 21, 3, 16
TEXT_TALKER_VOCABS = (64, 2152)
TEXT_CP_VOCABS = (64, 2048)
HOLD_AVAIL, HOLD_BUDGET = 5, 12
HOLD_N_PAST = (0, 1, HOLD_AVAIL - 1, HOLD_AVAIL, HOLD_AVAIL + 1, HOLD_BUDGET - 1, HOLD_BUDGET)
TEXT_CAP = 6
TEXT_AVAILS = (0, 1, 3, 6)
HELD_SENTINEL = -7


def hold_grid():
    """(n_past, flags, done) of the hold rule's hand grid: every edge of 1 <= n_past, text_avail <= n_past < budget."""
    return [(n, fl, done) for n in HOLD_N_PAST for fl in (0, 1, 2, 3) for done in (0, 1)]


def _launches(specs, R=TEXT_R):
    specs = list(specs)
    specs += specs[:(-len(specs)) % R]
    return [specs[i:i + R] for i in range(0, len(specs), R)]


def _text_slots(rng, flags_of, talker):
    """SlotParams of a launch: row TEXT_ROW0 + i greedy for even i, stochastic for odd i."""
    slots = []
    for r in range(TEXT_RT):
        i = r - TEXT_ROW0
        T = 0.8 if i % 2 else 0.0
        slots.append(slot(max_frames=HOLD_BUDGET, t_temp=T if talker else 0.7, t_top_k=5, t_top_p=0.9, c_temp=0.7 if talker else T,
                          c_top_k=5, seed=int(rng.integers(0, 2 ** 63)), no_row=r % 2, flags=flags_of(i) if 0 <= i < TEXT_R else 3))
    return slots


def _talker_text_case(V, tag, li, rows, text_avail):
    """rows: TEXT_R tuples (n_past, flags, done, n_text).  EOS is on top of every row of the launch, far above the
    rest: a row that decides ends, unless its EOS is masked."""
    audio_vocab, eos = TALKER_VOCABS[V]
    rng = rng_for(tag, V, li)
    st = talker_state(rng, TEXT_RT, V, audio_vocab)
    st["n_text"][:] = 0
    st["held"] = np.full(TEXT_RT, HELD_SENTINEL, np.int32)
    logits = (SPREAD * 0.8 * rng.standard_normal((TEXT_RT, V))).astype(np.float32)
    for i, (n_past, _, done, n_text) in enumerate(rows):
        r = TEXT_ROW0 + i
        st["n_past"][r], st["done"][r], st["n_text"][r] = n_past, done, n_text
        logits[r, eos] = 200.0
    cfg = dict(V=V, audio_vocab=audio_vocab, eos=eos, rep_penalty=1.2, frame_cap=FRAME_CAP, row0=TEXT_ROW0, R=TEXT_R,
               R_total=TEXT_RT, slots=_text_slots(rng, lambda i: rows[i][1], True), text_avail=text_avail)
    return dict(logits=logits, st=st, cfg=cfg, families=[tag] * TEXT_R)


def hold_grid_cases(V):
    """The hand grid of tests/test_sample_reference.py on the device: text_avail = HOLD_AVAIL and a budget of HOLD_BUDGET
    on every row."""
    # (the grid's held cells all fall on even, greedy rows: the rows that fill the last launch repeat them on both kinds)
    grid = hold_grid() + [(n, 3, 0) for n in (5, 5, 6, 6, 11, 11, 4, 12)]
    return [_talker_text_case(V, "hold", li, [(n, fl, done, 0) for n, fl, done in rows], np.full(TEXT_RT, HOLD_AVAIL, np.int32))
            for li, rows in enumerate(_launches(grid))]


def eos_mask_cases(V):
    """flags 0 .. 3 with hold off (text_avail null), EOS on top; half of the rows beyond progress 2 (forced EOS: n_past
    31 of n_text 5), half far below (n_past 3)."""
    rows = [((31, 3)[(i // 4) % 2], i % 4, 0, 5) for i in range(TEXT_R)]
    case = _talker_text_case(V, "eos_mask", 0, rows, None)
    for s in case["cfg"]["slots"]:
        s["max_frames"] = 0
    for i in range(TEXT_R):                      # greedy and stochastic rows of every (flags, forced) pair
        case["cfg"]["slots"][TEXT_ROW0 + i]["t_temp"] = 0.8 if i >= 8 else 0.0
    return [case]


def _cp_text_case(V, tag, li, frame_cap=FRAME_CAP, group=4):
    rng = rng_for(tag, V, li)
    cfg = dict(V=V, frame_cap=frame_cap, row0=TEXT_ROW0, R=TEXT_R, R_total=TEXT_RT, group=group,
               slots=_text_slots(rng, lambda i: (1, 0, 3, 2)[i % 4], False))
    logits = (SPREAD * 0.8 * rng.standard_normal((TEXT_RT, V))).astype(np.float32)
    codes = rng.integers(0, 64, (frame_cap, TEXT_RT, 16)).astype(np.int32)      # ids of every vocabulary in use
    return rng, dict(logits=logits, cfg=cfg, families=[tag] * TEXT_R, codes=codes,
                     n_frames=rng.integers(1, frame_cap + 1, TEXT_RT).astype(np.int32))


def cp_held_cases(V):
    """Even rows of the launch held, in pairs greedy / stochastic; the id the frame records in this group's column is in
    range, -1, beyond the vocabulary, or in range under a teacher-forced id.  A held row's logits put another id on
    top, far above the rest: a fresh decision would differ from the recorded id."""
    rng, case = _cp_text_case(V, "cp_held", 0)
    cfg, g = case["cfg"], case["cfg"]["group"]
    held = np.ones(TEXT_RT, np.int32)
    forced = np.full((FRAME_CAP, TEXT_RT, 16), -1, np.int32)
    for i in range(TEXT_R):
        r = TEXT_ROW0 + i
        held[r] = int(i % 4 < 2)                 # held rows 0, 1 (greedy, stochastic), free rows 2, 3, ...
        nf = case["n_frames"][r] = 1 + (i * 3) % FRAME_CAP
        rec = (int(rng.integers(0, V)), -1, V + 5, int(rng.integers(0, V)))[(i // 4) % 4]
        case["codes"][nf - 1, r, 1 + g] = rec
        if (i // 4) % 4 == 3:
            forced[nf - 1, r, 1 + g] = 9
            forced[nf - 1, r, 1 + (g + 1) % 15] = 2
        if held[r]:
            case["logits"][r, ((rec if 0 <= rec < V else 0) + 7) % V] = 200.0
    cfg.update(held=held, forced=forced)
    return [case]


def text_row_cases(V):
    """The feedback launch (group 14) of text slots: (text_avail, n_frames) over TEXT_AVAILS x {0, 1, avail, avail + 1,
    frame_cap, frame_cap + 1}; flags 0 rows with text_avail > 0 among them.  A last launch has frame_cap = 2 below
    text_avail = 6: rows that ended past the codes array still add the text row of their own frame."""
    specs = [(av, nf, FRAME_CAP) for av in TEXT_AVAILS for nf in (0, 1, av, av + 1, FRAME_CAP, FRAME_CAP + 1)]
    cases = []
    for li, rows in enumerate(_launches(specs) + [[(TEXT_CAP, nf, 2) for nf in (1, 2, 3, 4, 5, 6, 7, 8)] * 2]):
        rng, case = _cp_text_case(V, "text_rows", li, frame_cap=rows[0][2], group=14)
        ta = np.zeros(TEXT_RT, np.int32)
        for i, (av, nf, _) in enumerate(rows):
            ta[TEXT_ROW0 + i], case["n_frames"][TEXT_ROW0 + i] = av, nf
        case["cfg"].update(text_avail=ta, text_cap=TEXT_CAP)
        cases.append(case)
    return cases


def text_talker_cases(V):
    return hold_grid_cases(V) + eos_mask_cases(V)


def text_cp_cases(V):
    return cp_held_cases(V) + text_row_cases(V)
