"""Plain-numpy reference of the per-slot sampler rules -- TEST INFRASTRUCTURE ONLY.

Written from the contract (q3e_slot_rules in include/qwen3tts_engine.h, SlotRules / TalkerSampleArgs::rules / seen in
csrc/q3_kernels.h), not from the kernels' code; tests/sample_ref.py supplies everything the rules do not touch (the draw,
the acceptable set of a stochastic pick, the state transition, held rows).

A rules entry is a dict with the keys of DEFAULT; cfg["rules"] is a list of them, one per row of the batch, or None / absent
(the launch's constants).  A row's seen-set is a row of uint32 words, one bit per audio id; st["seen"] is [R_total][words].

tests/test_sample_rules_reference.py pins this file against tests/sample_ref.py (at default rules), against transformers'
RepetitionPenaltyLogitsProcessor (rep_window 0) and against hand-worked values.
"""
from __future__ import annotations

import numpy as np

from tests import sample_ref as SR

DEFAULT = dict(rep_penalty=1.2, rep_window=30, eos_boost=15.0, eos_force=2.0, min_past=0, cp_top_p=1.0)
MASKED = np.float32(-1e10)


def rules(**kw):
    """A rules entry: the defaults with the given fields replaced."""
    assert set(kw) <= set(DEFAULT), kw
    return dict(DEFAULT, **kw)


def seen_words(audio_vocab) -> int:
    return (int(audio_vocab) + 31) // 32


def seen_has(seen_row, t) -> bool:
    return 0 <= t < 32 * len(seen_row) and bool((int(seen_row[t >> 5]) >> (t & 31)) & 1)


def seen_add(seen_row, t, audio_vocab):
    """The seen-set transition, in place: the bit of an id in [0, audio_vocab) is set; any other id has no bit."""
    if 0 <= int(t) < int(audio_vocab):
        seen_row[int(t) >> 5] |= np.uint32(1 << (int(t) & 31))


def seen_of(ids, audio_vocab):
    """The seen-set of a list of emitted ids."""
    row = np.zeros(seen_words(audio_vocab), np.uint32)
    for t in ids:
        seen_add(row, t, audio_vocab)
    return row


def penalised_ids(past, n_past, ru, seen_row, audio_vocab):
    """The ids the repetition penalty applies to: rep_window w >= 1 -- the last min(n_past, w) ids of the 32-entry ring;
    w == 0 -- every audio id of the row's seen-set."""
    w = int(ru["rep_window"])
    if w == 0:
        return {t for t in range(int(audio_vocab)) if seen_has(seen_row, t)}
    return {int(past[(int(n_past) - 1 - i) % SR.RING]) for i in range(min(int(n_past), w))}


def process_talker_rules(logits, past, n_past, n_text, ru, seen_row=None, audio_vocab=2048, eos=2150, ignore_eos=False):
    """sample_ref.process_talker with the row's rules, np.float32 operation for operation: mask, EOS rule, repetition
    penalty, in that order.  -> (processed logits f32, forced, eos_masked): EOS is masked (-1e10, no boost) under ignore_eos
    or while n_past < min_past; forced = eos_force != 0 and progress > (double)eos_force -- the caller applies it only when
    EOS is not masked.  The boost is (float)(min((progress - 0.8) / 0.7, 1) * (double)eos_boost), added only when
    eos_boost != 0."""
    l = SR.nan_as_inf(logits)
    ids = np.arange(len(l))
    l[(ids >= audio_vocab) & (ids != eos)] = MASKED
    eos_masked = bool(ignore_eos) or int(n_past) < int(ru["min_past"])
    if eos_masked:
        l[eos] = MASKED
    forced = False
    boost_max, force_at = float(np.float32(ru["eos_boost"])), float(np.float32(ru["eos_force"]))
    if n_text > 0:
        progress = int(n_past) / (int(n_text) * 3)
        if progress > 0.8 and not eos_masked and boost_max != 0.0:
            l[eos] = l[eos] + np.float32(min((progress - 0.8) / 0.7, 1.0) * boost_max)
        forced = force_at != 0.0 and progress > force_at
    pen = np.float32(ru["rep_penalty"])
    for t in penalised_ids(past, n_past, ru, seen_row, audio_vocab):
        if 0 <= t < len(l):
            l[t] = l[t] / pen if l[t] > 0 else l[t] * pen
    return l, forced, eos_masked


def row_rules(cfg, r):
    rs = cfg.get("rules")
    if rs is None:
        return rules(rep_penalty=cfg.get("rep_penalty", 1.2))
    assert cfg.get("slots") is not None, "rules are a per-slot feature"
    return rs[r]


def talker_sets_rules(logits, st, cfg):
    """sample_ref.talker_sets under cfg["rules"]: -> {row: (set of acceptable decisions, processed logits)}; a held row has
    no entry."""
    out = {}
    for r in range(cfg["row0"], cfg["row0"] + cfg["R"]):
        if SR.talker_held(st, cfg, r):
            continue
        p = SR._row_params(cfg, r, True)
        ign = bool(cfg.get("ignore_eos", False)) or bool(SR.slot_flags(cfg, r) & 2)
        seen_row = st["seen"][r] if "seen" in st else None
        l, forced, masked = process_talker_rules(logits[r], st["past"][r], int(st["n_past"][r]), int(st["n_text"][r]),
                                                 row_rules(cfg, r), seen_row, cfg["audio_vocab"], cfg["eos"], ign)
        if forced and not masked:
            s = {cfg["eos"]}
        else:
            u = SR.uniform01(p["seed"], p["row_key"], int(st["n_frames"][r]), 0)
            s = SR.pick_set(l, p["temperature"], p["top_k"], p["top_p"], u)
        out[r] = (s, l)
    return out


def talker_apply_row_rules(st, cfg, r, code):
    """sample_ref.talker_apply_row, and where the ring took an id (the row went on) the seen-set takes the same id --
    whatever the row's window; a row that ended writes nothing."""
    before = int(st["n_past"][r])
    SR.talker_apply_row(st, cfg, r, code)
    if "seen" in st and int(st["n_past"][r]) == before + 1:
        seen_add(st["seen"][r], int(st["past"][r, before % SR.RING]), cfg["audio_vocab"])


def cp_sets_rules(logits, n_frames, cfg):
    """sample_ref.cp_sets with the row's nucleus cut: top_p = rules[r].cp_top_p (no rules: none).  The arg-max ignores it."""
    out = {}
    rs = cfg.get("rules")
    for r in range(cfg["row0"], cfg["row0"] + cfg["R"]):
        if SR.cp_held(cfg, r):
            continue
        p = SR._row_params(cfg, r, False)
        u = SR.uniform01(p["seed"], p["row_key"], int(n_frames[r]), 1 + cfg["group"])
        out[r] = SR.pick_set(logits[r], p["temperature"], p["top_k"], 0.0 if rs is None else rs[r]["cp_top_p"], u)
    return out


def prompt_seen(codes, audio_vocab):
    """The seen-set a codec prompt [T][16] leaves: column 0 of every frame."""
    return seen_of([int(c[0]) for c in codes], audio_vocab)
