"""CPU reference of a codec-prompted utterance (q3e_admit_prompted) -- TEST INFRASTRUCTURE ONLY.

CpuPipeline.generate restated from the oracle's public pieces (talker.forward, talker.logits,
fe.process_talker_logits, cp.predict, fe.feedback_embedding) with the two things a prompt changes: the prefill runs over
[prefix ; rows(P)], rows(P)[i] = feedback_embedding(P[i]), and `past` starts as the prompt's column 0.  Everything else
-- the sampler rules, the EOS handling, the margins -- is generate()'s, line for line."""
import numpy as np

from oracle import frontend as fe


def prompt_rows(cpu, P, pad):
    """[T][16] codec ids -> [T][hidden] f32 talker rows (tts_client.py:199-208 per frame)."""
    P = np.asarray(P)
    rows = [fe.feedback_embedding(int(r[0]), [int(c) for c in r[1:]], cpu.codec_embedding, cpu.cp_emb, pad) for r in P]
    return np.stack(rows).astype(np.float32) if len(rows) else np.zeros((0, cpu.codec_embedding.shape[1]), np.float32)


def prompted_prefix(cpu, prefix, P, pad):
    """The n_rows + T rows the utterance's pass prefills."""
    return np.ascontiguousarray(np.concatenate([np.asarray(prefix, np.float32), prompt_rows(cpu, P, pad)], axis=0))


def frame0_logits(cpu, prefix, P, pad):
    """Raw talker logits of the first generated frame."""
    cpu.talker.clear()
    return cpu.talker.logits(cpu.talker.forward(prompted_prefix(cpu, prefix, P, pad), 0))


def decide(cpu, logits, past, n_text, ignore_eos):
    """One talker decision as generate() takes it -> (code_0, top-1/top-2 gap of the processed logits)."""
    lg, forced = fe.process_talker_logits(logits, list(past), n_text, cpu.cfg.codec_eos)
    if ignore_eos:
        lg[cpu.cfg.codec_eos] = -1e10
        code0 = int(np.argmax(lg))
    else:
        code0 = int(forced) if forced is not None else int(np.argmax(lg))
    srt = np.sort(lg)
    return code0, float(srt[-1] - srt[-2])


def generate_prompted(cpu, prefix, P, n_text, pad, max_frames, ignore_eos=False, want_margins=False, past=None):
    """-> the GENERATED frames (and their margins, laid out as CpuPipeline.generate's).  past: the history the sampler
    starts with (default: the prompt's column 0, what the engine seeds)."""
    cfg = cpu.cfg
    P = np.asarray(P).reshape(-1, 16)
    rows = prompted_prefix(cpu, prefix, P, pad)
    cpu.talker.clear()
    hidden = cpu.talker.forward(rows, 0)
    pos = rows.shape[0]
    past = [int(c) for c in P[:, 0]] if past is None else list(past)
    frames, margins_all = [], []
    for _ in range(max_frames):
        code0, m0 = decide(cpu, cpu.talker.logits(hidden), past, n_text, ignore_eos)
        if code0 == cfg.codec_eos or code0 >= 2048:
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


def random_prompt(rng, T):
    return rng.integers(0, 2048, size=(T, 16)).astype(np.int32)
