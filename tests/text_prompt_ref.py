"""CPU reference of a text slot that continues a codec prompt (q3e_slot_params.reserved == 3) -- TEST INFRASTRUCTURE ONLY.

tests/prompt_ref.py's generate_prompted with one thing changed: the row added last to the feedback of GENERATED frame f is
rows[f] while f < len(rows), the pad row afterwards.  The prompt's own rows still add the pad row, `past` still starts as
the prompt's column 0, and the sampler rules, the EOS handling and the margins are generate()'s, line for line.  Assembled
from the oracle's public pieces, as prompt_ref.py is."""
import numpy as np

from oracle import frontend as fe
from tests import prompt_ref as pr


def generate_text_prompted(cpu, prefix, P, rows, n_text, pad, max_frames, ignore_eos=False, want_margins=False, past=None,
                           mask_eos_until=None):
    """-> the GENERATED frames (and their margins, laid out as CpuPipeline.generate's).  rows: [n][hidden] text rows, row f
    for generated frame f.  past: the history the sampler starts with (default: the prompt's column 0).
    mask_eos_until (None: never): the first generated frame that is sampled under the EOS rules with `n_text`; the frames
    before it are sampled as a text slot before its final push is -- EOS masked, n_text 0."""
    cfg = cpu.cfg
    P = np.asarray(P).reshape(-1, 16)
    rows = np.asarray(rows, np.float32).reshape(-1, cpu.codec_embedding.shape[1])
    full = pr.prompted_prefix(cpu, prefix, P, pad)
    cpu.talker.clear()
    hidden = cpu.talker.forward(full, 0)
    pos = full.shape[0]
    past = [int(c) for c in P[:, 0]] if past is None else list(past)
    frames, margins_all = [], []
    for f in range(max_frames):
        open_text = mask_eos_until is not None and f < mask_eos_until
        code0, m0 = pr.decide(cpu, cpu.talker.logits(hidden), past, 0 if open_text else n_text, ignore_eos or open_text)
        if code0 == cfg.codec_eos or code0 >= 2048:
            margins_all.append([m0] + [np.inf] * 15)
            break
        codes, margins = cpu.cp.predict(hidden, code0)
        margins_all.append([m0] + [float(x) for x in margins])
        frames.append([code0] + [int(c) for c in codes])
        past.append(code0)
        fb = fe.feedback_embedding(code0, codes, cpu.codec_embedding, cpu.cp_emb, rows[f] if f < len(rows) else pad)
        hidden = cpu.talker.forward(fb, pos)
        pos += 1
    return (frames, margins_all) if want_margins else frames
