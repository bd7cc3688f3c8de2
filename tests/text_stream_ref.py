"""CPU oracle that FOLLOWS the device through a text-stream utterance (tests/test_gpu_text_stream.py).

After every frame step the oracle is fed the ids the device decided in that frame, with the text row of that frame where
tts_client.py:207-208 adds tts_pad, so a near-tie flip ends nothing: every frame of the run is graded.  oracle/ is
imported, not edited."""
import numpy as np

from oracle import frontend as ofe
from oracle import oracle as orc


class Follower:
    """One utterance: a talker KV cache of its own (swapped into the shared TalkerOracle around every forward), the code
    predictor shared.  rows[f] is the row added to the feedback of frame f; frames past the rows take `pad`."""

    def __init__(self, cfg, talker, cp, prefix, rows, pad):
        self.cfg, self.talker, self.cp = cfg, talker, cp
        self.rows, self.pad = [np.asarray(r, np.float32) for r in rows], np.asarray(pad, np.float32)
        talker.clear()
        self.kc, self.vc = talker.kc, talker.vc
        self.hidden = self._forward(prefix, 0)
        self.pos = prefix.shape[0]
        self.past = []
        self.f = 0

    def _forward(self, embd, pos):
        self.talker.kc, self.talker.vc = self.kc, self.vc
        return self.talker.forward(embd, pos)

    def row(self, f):
        return self.rows[f] if f < len(self.rows) else self.pad

    def logits(self, hidden=None):
        return self.talker.logits(self.hidden if hidden is None else hidden)

    def grade(self, ids, near_tie, n_text=0, mask_eos=True):
        """Decisions of the device's frame `ids` [16] against the oracle's from its current hidden state -> list of
        (group, oracle gap) of the decisions that are neither the oracle's arg-max nor within near_tie of it."""
        cfg, bad = self.cfg, []
        lg, forced = ofe.process_talker_logits(self.logits(), self.past, n_text, cfg.codec_eos)
        if mask_eos:
            lg[cfg.codec_eos] = -1e10
        assert forced is None or mask_eos
        gap = float(lg.max() - lg[int(ids[0])])
        if gap >= near_tie:
            bad.append((0, gap))
        # the code predictor is fed the device's ids; it reports its own decisions and their top-1/top-2 gaps
        codes, margins = self.cp.predict(self.hidden, int(ids[0]), forced=np.asarray(ids[1:], np.int32))
        for g in range(15):
            if int(codes[g]) != int(ids[1 + g]) and not float(margins[g]) < near_tie:
                bad.append((1 + g, float(margins[g])))
        return bad

    def feed(self, ids):
        """The talker step that follows the device's frame `ids`: its feedback with this frame's row."""
        fb = ofe.feedback_embedding(int(ids[0]), [int(c) for c in ids[1:]], self.talker.codec_embedding, self.cp.emb,
                                    self.row(self.f))
        self.hidden = self._forward(fb, self.pos)
        self.past.append(int(ids[0]))
        self.pos += 1
        self.f += 1
        return self.hidden


def logit_distance(talker, h_a, h_b):
    """max |logit(h_a) - logit(h_b)| over the codec head: the measure tests/test_gpu_engine.py bounds by NEAR_TIE / 2."""
    return float(np.abs(talker.logits(h_a) - talker.logits(h_b)).max())
