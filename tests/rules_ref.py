"""CPU reference of an utterance under per-slot sampler rules (q3e_admit_ruled) -- TEST INFRASTRUCTURE ONLY.

tests/prompt_ref.generate_prompted restated with a rules-aware decision, from the oracle's public pieces (talker.forward,
talker.logits, cp.predict, fe.feedback_embedding) and the contract of q3e_slot_rules in include/qwen3tts_engine.h.  The
history is the plain chronological list of emitted ids, prompt first, so "the last w ids" and "every id" are list
operations here and cannot share the device's ring or bit-set arithmetic.  At default rules decide_ruled is
prompt_ref.decide (pinned by tests/test_sample_rules_reference.py)."""
import numpy as np

from oracle import frontend as fe
from tests import prompt_ref as pr

AUDIO_VOCAB = 2048


def decide_ruled(cpu, logits, past, n_text, ignore_eos, ru, n_prompt=0):
    """One talker decision under the rules `ru` (engine.SlotRules) -> (code_0, top-1/top-2 gap of the processed logits).
    past: every id emitted so far, the prompt's n_prompt first."""
    eos = cpu.cfg.codec_eos
    lg = np.array(logits, dtype=np.float32, copy=True)
    lg[AUDIO_VOCAB:eos] = -1e10
    lg[eos + 1:] = -1e10
    masked = bool(ignore_eos) or len(past) - n_prompt < ru.min_frames
    forced = False
    if masked:
        lg[eos] = -1e10
    if n_text > 0:
        progress = len(past) / (n_text * 3)
        if progress > 0.8 and not masked and ru.eos_boost != 0:
            lg[eos] += np.float32(min((progress - 0.8) / 0.7, 1.0) * float(np.float32(ru.eos_boost)))
        forced = ru.eos_force != 0 and progress > float(np.float32(ru.eos_force)) and not masked
    pen = np.float32(ru.rep_penalty)
    for t in set(past if ru.rep_window == 0 else past[-ru.rep_window:]):   # (every emitted id is an audio id)
        if 0 <= t < len(lg):
            lg[t] = lg[t] / pen if lg[t] > 0 else lg[t] * pen
    code0 = eos if forced else int(np.argmax(lg))
    srt = np.sort(lg)
    return code0, float(srt[-1] - srt[-2])


def generate_ruled(cpu, prefix, P, n_text, pad, max_frames, ru, ignore_eos=False, want_margins=False):
    """prompt_ref.generate_prompted under the rules `ru`: -> the GENERATED frames (and their margins)."""
    cfg = cpu.cfg
    P = np.zeros((0, 16), np.int32) if P is None else np.asarray(P).reshape(-1, 16)
    rows = pr.prompted_prefix(cpu, prefix, P, pad)
    cpu.talker.clear()
    hidden = cpu.talker.forward(rows, 0)
    pos = rows.shape[0]
    past = [int(c) for c in P[:, 0]]
    frames, margins_all = [], []
    for _ in range(max_frames):
        code0, m0 = decide_ruled(cpu, cpu.talker.logits(hidden), past, n_text, ignore_eos, ru, len(P))
        if code0 == cfg.codec_eos or code0 >= AUDIO_VOCAB:
            margins_all.append([m0] + [np.inf] * 15)
            break
        codes, margins = cpu.cp.predict(hidden, code0)
        margins_all.append([m0] + [float(x) for x in margins])
        frames.append([code0] + [int(c) for c in codes])
        past.append(code0)
        fb = fe.feedback_embedding(code0, codes, cpu.codec_embedding, cpu.cp_emb, pad)
        hidden = cpu.talker.forward(fb, pos)
        pos += 1
    return (frames, margins_all) if want_margins else frames
