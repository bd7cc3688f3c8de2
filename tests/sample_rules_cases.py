"""Seeded inputs of the sampler-rules tests -- shared by tests/test_sample_rules_reference.py (reference alone: the
ambiguity cap) and tests/test_gpu_sample_rules.py (the same cases on the device).  One case = one launch of TEXT_R rows at
row TEXT_ROW0 of TEXT_RT, per-slot mode, as the text-slot cases of tests/sample_cases.py; even rows greedy, odd rows
stochastic unless a case says otherwise.

A decision is all a launch shows of its processed logits, so the hand cases put the decision ON the value under test: a
competitor id one float32 step below / above the processed value the reference computes, so that the two outcomes differ
whenever one bit of the device's value differs."""
from __future__ import annotations

import numpy as np

from tests import sample_cases as SC
from tests import sample_ref as SR
from tests import sample_rules_ref as RR

RT, ROW0, R = SC.TEXT_RT, SC.TEXT_ROW0, SC.TEXT_R
WINDOWS = (1, 2, 29, 30, 0)
PENALTIES = (1.0, 1.05, 1.2, 3.0)
BOOSTS = (0.0, 7.5, 15.0)
CP_TOP_PS = (1.0, 0.95, 0.5, 1e-6)
LOW = np.float32(-30.0)      # every id that plays no part


def n_pasts(w):
    return sorted({n for n in (0, 1, w - 1, w, w + 1, 31, 32, 33, 100) if n >= 0})


def boundary_ids(audio_vocab):
    """Ids on the seen-set's word boundaries."""
    return [t for t in (0, 31, 32, 63, audio_vocab - 1) if t < audio_vocab]


def _slots(rng, greedy_of=lambda i: i % 2 == 0, flags_of=lambda i: 0, max_frames=0):
    out = []
    for r in range(RT):
        i = r - ROW0
        T = 0.0 if greedy_of(i) else 0.8
        out.append(SC.slot(max_frames=max_frames, t_temp=T, t_top_k=5, t_top_p=0.9, c_temp=T, c_top_k=5,
                           seed=int(rng.integers(0, 2 ** 63)), no_row=r % 2, flags=flags_of(i) if 0 <= i < R else 0))
    return out


def _state(rng, V, audio_vocab):
    """A valid random state with a seen-set that matches nothing in particular (rows outside the launch keep it)."""
    st = SC.talker_state(rng, RT, V, audio_vocab)
    st["n_text"][:] = 0
    st["seen"] = rng.integers(0, 2 ** 32, (RT, RR.seen_words(audio_vocab)), dtype=np.uint64).astype(np.uint32)
    return st


def set_history(st, r, hist, audio_vocab):
    """Row r has emitted `hist` (chronological): ring, counter and seen-set as the sampler would have left them."""
    st["n_past"][r] = len(hist)
    st["past"][r] = -5                                   # entries never written are never read
    for i, t in enumerate(hist):
        if i >= len(hist) - SR.RING:
            st["past"][r, i % SR.RING] = t
    st["seen"][r] = RR.seen_of(hist, audio_vocab)


def _base(V, tag, li, **slot_kw):
    audio_vocab, eos = SC.TALKER_VOCABS[V]
    rng = SC.rng_for("rules", tag, V, li)
    st = _state(rng, V, audio_vocab)
    logits = np.full((RT, V), LOW, np.float32) + (0.5 * rng.standard_normal((RT, V))).astype(np.float32)
    cfg = dict(V=V, audio_vocab=audio_vocab, eos=eos, rep_penalty=1.2, frame_cap=SC.FRAME_CAP, row0=ROW0, R=R, R_total=RT,
               slots=_slots(rng, **slot_kw), rules=[RR.rules() for _ in range(RT)])
    return rng, dict(logits=logits, st=st, cfg=cfg, families=[tag] * R)


def _launches(specs):
    specs = list(specs)
    specs += specs[:(-len(specs)) % R]
    return [specs[i:i + R] for i in range(0, len(specs), R)]


def window_cases(V):
    """rep_window x n_past, the probe id X on top standing ONCE in the history, at age a (0 = the newest): a = w - 1 is the
    oldest id inside the window, a = w the first outside; for w = 0 the oldest id of the whole history (older than the ring
    once n_past > 32) and an id that was never emitted.  A competitor Y sits between X's penalised and unpenalised value:
    X penalised -> Y is on top.  X and Y walk over the ids on the seen-set's word boundaries."""
    audio_vocab, _ = SC.TALKER_VOCABS[V]
    bid = boundary_ids(audio_vocab)
    specs = []
    for w in WINDOWS:
        for n in n_pasts(w):
            ages = (n - 1, n) if w == 0 else (w - 1, w)   # (age n: not in the history at all)
            specs += [(w, n, a) for a in ages]
    cases = []
    for li, rows in enumerate(_launches(specs)):
        rng, case = _base(V, "window", li, greedy_of=lambda i: (i // 2) % 2 == 0)   # both ages on greedy and on stochastic rows
        for i, (w, n, age) in enumerate(rows):
            r = ROW0 + i
            x, y = bid[(li + i) % len(bid)], bid[(li + i + 1) % len(bid)]
            others = [t for t in range(audio_vocab) if t not in (x, y)]
            hist = [int(t) for t in rng.choice(others, size=n)]
            if 0 <= age < n:
                hist[n - 1 - age] = x
            set_history(case["st"], r, hist, audio_vocab)
            case["cfg"]["rules"][r] = RR.rules(rep_window=w)
            case["logits"][r, x], case["logits"][r, y] = 10.0, 9.5          # 10 / 1.2 < 9.5 < 10
        cases.append(case)
    return cases


def _on_the_value(case, r, value, y, above):
    """Competitor y one float32 step above / below `value`."""
    case["logits"][r, y] = np.nextafter(np.float32(value), np.float32(np.inf if above else -np.inf))


def penalty_cases(V):
    """rep_penalty x the sign of the penalised logit (positive: divided, negative and zero: multiplied), window 30 and window
    0, the competitor one step below and one step above the reference's processed value.  Greedy rows only: the arg-max
    resolves one bit."""
    audio_vocab, _ = SC.TALKER_VOCABS[V]
    specs = [(p, v, w, above) for p in PENALTIES for v in (7.3, -7.3, 0.0) for w in (30, 0) for above in (0, 1)]
    cases = []
    for li, rows in enumerate(_launches(specs)):
        rng, case = _base(V, "penalty", li, greedy_of=lambda i: True)
        case["logits"][:] = -100.0
        for i, (p, v, w, above) in enumerate(rows):
            r = ROW0 + i
            x, y = 5 + i, 30 + i % 10
            set_history(case["st"], r, [x, 1, 2], audio_vocab)
            ru = case["cfg"]["rules"][r] = RR.rules(rep_penalty=p, rep_window=w)
            case["logits"][r, x] = v
            l, _, _ = RR.process_talker_rules(case["logits"][r], case["st"]["past"][r], 3, 0, ru, case["st"]["seen"][r],
                                              audio_vocab, case["cfg"]["eos"])
            _on_the_value(case, r, l[x], y, above)
        cases.append(case)
    return cases


def eos_cases(V, ignore_eos=False):
    """The EOS rules, EOS far on top of every row unless said:
      min_past   n_past = min_past - 1 / min_past, with slot flags 0 / 2 (and launch-wide ignore_eos in a second set), also
                 where progress forces EOS (n_past 32 / 33 of n_text 5): below the minimum the force is not applied;
      eos_force  progress exactly equal to eos_force (30 of n_text 5 at 2.0; 15 at 1.0): not forced; one frame above: forced;
                 0: never, at n_past 100.  EOS far below, so only the force gives it;
      eos_boost  0 / 7.5 / 15 at progress 17 / 15: the competitor one step below / above the boosted EOS value."""
    audio_vocab, eos = SC.TALKER_VOCABS[V]
    specs = [("min", mp, d, fl, nt) for mp in (4, 33) for d in (-1, 0) for fl in (0, 2) for nt in (0, 5)]
    specs += [("force", ef, n, 0, 5) for ef, ns in ((2.0, (30, 31)), (1.0, (15, 16)), (0.0, (31, 100)), (0.5, (7, 8))) for n in ns]
    specs += [("boost", b, above, 0, 5) for b in BOOSTS for above in (0, 1)]
    cases = []
    for li, rows in enumerate(_launches(specs)):
        rng, case = _base(V, "eos", li, flags_of=lambda i: rows[i][3] if rows[i][0] == "min" else 0)
        case["cfg"]["ignore_eos"] = bool(ignore_eos)
        for i, (kind, a, b, fl, nt) in enumerate(rows):
            r = ROW0 + i
            st = case["st"]
            st["n_text"][r] = nt
            if kind == "min":
                n = a + b
                ru = RR.rules(min_past=a)
                case["logits"][r, eos] = 200.0
            elif kind == "force":
                n = b
                ru = RR.rules(eos_force=a, eos_boost=0.0)
                case["logits"][r, eos] = -90.0
            else:
                n = 17
                ru = RR.rules(eos_boost=a)
            hist = [int(t) for t in rng.integers(0, audio_vocab, n)]
            set_history(st, r, hist, audio_vocab)
            case["cfg"]["rules"][r] = ru
            if kind == "boost":
                case["cfg"]["slots"][r]["t_temp"] = 0.0
                y = next(t for t in range(audio_vocab) if t not in hist)
                case["logits"][r, eos] = 3.25
                l, _, _ = RR.process_talker_rules(case["logits"][r], st["past"][r], n, nt, ru, st["seen"][r], audio_vocab, eos,
                                                  ignore_eos)
                _on_the_value(case, r, l[eos], y, b)
        cases.append(case)
    return cases


def forced_cases(V):
    """Teacher forcing: the ring and the seen-set take the forced id (on a word boundary), the codes record the decision;
    rows of every window, so the set is written whatever the window is."""
    audio_vocab, _ = SC.TALKER_VOCABS[V]
    rng, case = _base(V, "forced", 0)
    bid = boundary_ids(audio_vocab)
    forced = np.full((SC.FRAME_CAP, RT, 16), -1, np.int32)
    for i in range(R):
        r = ROW0 + i
        set_history(case["st"], r, [int(t) for t in rng.integers(0, audio_vocab, i)], audio_vocab)
        case["cfg"]["rules"][r] = RR.rules(rep_window=WINDOWS[i % len(WINDOWS)])
        if i % 4 != 3:                                   # (every fourth row runs free)
            forced[int(case["st"]["n_frames"][r]), r, 0] = bid[i % len(bid)]
        case["logits"][r, 7 + i] = 10.0
    case["cfg"]["forced"] = forced
    return [case]


def held_cases(V):
    """The hold rule's hand grid (sample_cases.hold_grid_cases) with a seen-set and non-default rules on every row: a held
    row leaves its set alone."""
    audio_vocab, _ = SC.TALKER_VOCABS[V]
    cases = SC.hold_grid_cases(V)
    for li, case in enumerate(cases):
        rng = SC.rng_for("rules", "held", V, li)
        case["st"]["seen"] = rng.integers(0, 2 ** 32, (RT, RR.seen_words(audio_vocab)), dtype=np.uint64).astype(np.uint32)
        case["cfg"]["rules"] = [RR.rules(rep_window=WINDOWS[r % len(WINDOWS)], rep_penalty=PENALTIES[r % 4]) for r in range(RT)]
    return cases


def talker_rule_cases(V):
    return window_cases(V) + penalty_cases(V) + eos_cases(V) + eos_cases(V, ignore_eos=True) + forced_cases(V) + held_cases(V)


def talker_family_cases(V):
    """The stochastic families of sample_cases (same SPREAD, FAMILIES, TEMPS, TOP_PS) under random non-default rules: one
    launch per family pair, every row with a history and rules of its own."""
    audio_vocab, eos = SC.TALKER_VOCABS[V]
    fams = [f for f in SC.FAMILIES for _ in range(6)]
    cases = []
    for li, rows in enumerate(_launches(fams)):
        rng, case = _base(V, "families", li)
        case["families"] = rows
        for i, fam in enumerate(rows):
            r = ROW0 + i
            s = case["cfg"]["slots"][r]
            s.update(t_temp=SC.TEMPS[rng.integers(5)], t_top_k=(1, 2, 50, 64, 65)[rng.integers(5)], t_top_p=SC.TOP_PS[rng.integers(6)])
            if fam == "all_ninf" and s["t_top_p"] == 0.5:
                s["t_top_p"] = 0.95      # (the mask makes the row flat over an even number of ids: half the mass is hit exactly)
            n = int(rng.choice([0, 3, 31, 40]))
            set_history(case["st"], r, [int(t) for t in rng.integers(0, audio_vocab, n)], audio_vocab)
            case["st"]["n_text"][r] = int(rng.choice([0, 7, 30]))
            case["cfg"]["rules"][r] = RR.rules(rep_penalty=PENALTIES[rng.integers(4)], rep_window=WINDOWS[rng.integers(5)],
                                               eos_boost=BOOSTS[rng.integers(3)], eos_force=(0.0, 1.0, 2.0)[rng.integers(3)],
                                               min_past=int(rng.choice([0, 4, 35])))
            case["logits"][r] = SC.make_logits(fam, rng, V, audio_vocab, s["t_top_k"], s["t_temp"])
        cases.append(case)
    return cases


def cp_rule_cases(V):
    """cp_top_p x the families, greedy and stochastic rows side by side, groups 0 and 14; top-k on the selection path and on
    the sort path."""
    fams = [f for f in SC.FAMILIES for _ in range(3)]
    cases = []
    for li, rows in enumerate(_launches(fams) * 2):
        rng = SC.rng_for("rules", "cp", V, li)
        cfg = dict(V=V, frame_cap=SC.FRAME_CAP, row0=ROW0, R=R, R_total=RT, group=(0, 14)[li % 2], slots=_slots(rng),
                   rules=[RR.rules(cp_top_p=CP_TOP_PS[(r + li) % 4]) for r in range(RT)])
        logits = np.zeros((RT, V), np.float32)
        for i, fam in enumerate(rows):
            s = cfg["slots"][ROW0 + i]
            if i % 2:
                s.update(c_temp=SC.TEMPS[1 + rng.integers(4)], c_top_k=(2, 50, 64, 65, 0)[rng.integers(5)])
            logits[ROW0 + i] = SC.make_logits(fam, rng, V, V, s["c_top_k"], s["c_temp"])
        cases.append(dict(logits=logits, cfg=cfg, families=rows, n_frames=rng.integers(1, SC.FRAME_CAP + 1, RT).astype(np.int32),
                          codes=np.full((SC.FRAME_CAP, RT, 16), -7, np.int32)))
    return cases


PROMPT_TS = (1, 31, 32, 33, 70)


def prompt_codes(T, audio_vocab, rng):
    """A codec prompt [T][16] whose column 0 holds duplicates and ids that share a seen-set word."""
    codes = rng.integers(0, 64, (T, 16)).astype(np.int32)
    pool = boundary_ids(audio_vocab) + [33, 34, 35, 33]
    codes[:, 0] = [pool[int(rng.integers(len(pool)))] if i % 3 else int(rng.integers(0, audio_vocab)) for i in range(T)]
    return codes
