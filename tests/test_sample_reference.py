"""tests/sample_ref.py (the reference the GPU sampling tests grade every device decision with) against hand-worked
values and oracle/frontend.py's restatement of the reference servers -- so the kernels' reference cannot share a
misunderstanding with the kernels -- and, from the reference alone, the share of ambiguous cases in every input family
tests/test_gpu_sample_decisions.py runs (at most 5 %)."""
import numpy as np
import pytest

from oracle import frontend as fe
from tests import sample_cases as SC
from tests import sample_ref as SR
from tests.test_golden_frontend import _talker_tables

GOLDEN64 = 0x9E3779B97F4A7C15


def _ring(chron):
    ring = np.zeros(32, np.int32)
    for i in range(max(0, len(chron) - 32), len(chron)):
        ring[i % 32] = chron[i]
    return ring


# ---- uniform01 ------------------------------------------------------------------------------------------------------
def test_uniform01_hand_values():
    """Key (0, row, 0, 0) makes z = (1 + row) * golden: the state of splitmix64 seeded with 0 after 1 + row steps, whose
    outputs are published test vectors; the draw is their top 24 bits."""
    splitmix64_seed0 = (16294208416658607535, 7960286522194355700, 487617019471545679)
    for row, out in enumerate(splitmix64_seed0):
        assert SR.uniform01(0, row, 0, 0) == (out >> 40) / 2.0 ** 24
    assert SR.uniform01(0, 0, 0, 0) == 0xE220A8 / 16777216.0
    # the counter: row + frame * 2^20 + group * 2^44, times golden, added to the seed modulo 2^64
    assert SR.uniform01(5, 3, 2, 1) == SR.uniform01((5 + GOLDEN64 * (3 + (2 << 20) + (1 << 44))) % 2 ** 64, 0, 0, 0)
    assert SR.uniform01(2 ** 64 - 1, 1, 0, 0) == SR.uniform01(GOLDEN64 - 1, 0, 0, 0)      # wraps
    assert SR.uniform01(0, 1 << 20, 0, 0) == SR.uniform01(0, 0, 1, 0)                      # the documented packing


def _uniform01_u64(seed, row, frame, group):
    """The same hash in wrapping np.uint64 arithmetic."""
    with np.errstate(over="ignore"):
        u = np.uint64
        z = u(seed) + u(GOLDEN64) * (u(1) + u(row) + (u(frame) << u(20)) + (u(group) << u(44)))
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
        return float(np.float32(int(z >> u(40))) * np.float32(1.0 / 16777216.0))


def test_uniform01_every_key_part_changes_the_draw():
    rng = np.random.default_rng(3)
    for _ in range(200):
        seed = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))
        row, frame, group = int(rng.integers(0, 64)), int(rng.integers(0, 4096)), int(rng.integers(0, 16))
        u = SR.uniform01(seed, row, frame, group)
        assert 0.0 <= u < 1.0 and u == _uniform01_u64(seed, row, frame, group)
        others = {SR.uniform01(seed ^ 1, row, frame, group), SR.uniform01(seed, row + 1, frame, group),
                  SR.uniform01(seed, row, frame + 1, group), SR.uniform01(seed, row, frame, group + 1)}
        assert u not in others and len(others) == 4
    assert SR.uniform01(0, 0, 0, 0) != SR.uniform01(2 ** 64 - 1, 0, 0, 0)


# ---- pre-processing and greedy picks against the reference servers' restatement --------------------------------------
def test_greedy_matches_recorded_reference_cases(golden):
    H, TD, TV, CV = (int(x) for x in golden["talker_dims"])
    head = _talker_tables(int(golden["talker_seed"]), H, TD, TV, CV)["codec_head"]
    cases = [(golden[f"sample_{ci}_hidden"], [int(x) for x in golden[f"sample_{ci}_past"]], int(golden[f"sample_{ci}_ntext"]),
              int(golden[f"sample_{ci}_tok"])) for ci in range(int(golden["sample_n"]))]
    cases.append((golden["sample_rep_hidden"], [int(x) for x in golden["sample_rep_past"]], 50, int(golden["sample_rep_tok"])))
    forced_seen = 0
    for hidden, past, n_text, tok in cases:
        logits = hidden @ head.T
        l, forced = SR.process_talker(logits, _ring(past), len(past), n_text)
        want_l, want_forced = fe.process_talker_logits(logits, past, n_text)
        np.testing.assert_array_equal(l.view(np.uint32), want_l.view(np.uint32))
        assert forced == (want_forced is not None)
        got = 2150 if forced else SR.first_argmax(l)
        assert got == tok == fe.sample_talker(logits, past, n_text, temperature=0.0)
        forced_seen += forced
    assert forced_seen >= 1
    lg = golden["cps_logits"]
    assert SR.pick_set(lg, 0.0, 50, 0.0, 0.3) == {int(golden["cps_greedy"])} == {fe.sample_cp(lg, 0.0)}


def test_process_talker_matches_frontend_on_random_states():
    """Ring of 32 with a window of 30 against the chronological list, before and after n_past wraps; every progress
    regime; positive, negative and zero logits under the penalty."""
    rng = np.random.default_rng(7)
    V = 3072
    for n_past in (0, 1, 29, 30, 31, 32, 33, 64, 100):
        for n_text in (0, 1, 11, 14, 16, 40, 41, 42, 50):
            past = [int(x) for x in rng.integers(0, 2152, n_past)]
            logits = (4.0 * rng.standard_normal(V)).astype(np.float32)
            logits[rng.integers(0, V, 40)] = 0.0
            l, forced = SR.process_talker(logits, _ring(past), n_past, n_text)
            want_l, want_forced = fe.process_talker_logits(logits, past, n_text)
            np.testing.assert_array_equal(l.view(np.uint32), want_l.view(np.uint32), err_msg=f"{n_past} {n_text}")
            assert forced == (want_forced is not None)
            assert SR.window_ids(_ring(past), n_past) == past[::-1][:30]
    # ignore_eos: EOS is masked and never boosted; NaN orders as +inf
    l, _ = SR.process_talker(np.array([np.nan, 1.0] + [0.0] * 62, np.float32), np.zeros(32, np.int32), 0, 0, 48, 50, True)
    assert l[0] == np.inf and l[50] == np.float32(-1e10) and l[49] == np.float32(-1e10) and SR.first_argmax(l) == 0


class _Pick:
    """Stands in for np.random inside the frontend samplers: picks entry j and records the probabilities."""

    def __init__(self, j):
        self.j, self.p = j, None

    def choice(self, n, p=None):
        self.p = np.asarray(p)
        return min(self.j, n - 1)


@pytest.mark.parametrize("top_k", [2, 50])
def test_kept_set_matches_frontend_samplers(top_k):
    """Tie-free rows: the entries kept after top-k and top-p 0.95, their order and their probabilities are those inside
    oracle/frontend.sample_talker; the top-k set is the one inside sample_cp."""
    rng = np.random.default_rng(top_k)
    for trial in range(6):
        logits = (rng.uniform(1.0, 6.0) * rng.standard_normal(3072)).astype(np.float32)
        past = [int(x) for x in rng.integers(0, 2048, 12)]
        T = (0.5, 0.8, 1.0)[trial % 3]
        l, _ = SR.process_talker(logits, _ring(past), len(past), 7)
        assert len(np.unique(l[:2048])) == 2048
        order, p = SR.kept_exact(l, top_k, T, 0.95)
        toks = []
        for j in range(len(order) + 1):
            pk = _Pick(j)
            toks.append(fe.sample_talker(logits, past, 7, temperature=T, top_k=top_k, rng=pk))
        assert toks[:-1] == [int(i) for i in order] and toks[-1] == toks[-2]      # no further entry is kept
        np.testing.assert_allclose(pk.p, p, rtol=1e-5)
        # away from the boundaries the acceptable set is the inverse CDF's entry
        C = np.cumsum(p)
        for u in rng.random(50):
            s = SR.acceptable_picks(l, top_k, T, 0.95, u)
            k = int(np.searchsorted(C, u, side="right"))
            if np.abs(C - u).min() > 1e-4:
                assert s == {int(order[min(k, len(order) - 1)])}
        # code predictor: no top-p
        cp = (rng.uniform(1.0, 6.0) * rng.standard_normal(2048)).astype(np.float32)
        order, p = SR.kept_exact(cp, top_k, T, 0.0)
        got = {fe.sample_cp(cp, T, top_k, _Pick(j)) for j in range(top_k)}
        assert got == {int(i) for i in order} and len(order) == top_k


def test_acceptable_picks_hand_cases():
    ln = lambda *w: np.log(np.array(w, np.float64)).astype(np.float32)
    l = ln(1, 4, 2, 1)                       # weights 4, 2, 1, 1 in sampling order 1, 2, 0, 3: C = 4, 6, 7, 8
    assert SR.acceptable_picks(l, 0, 1.0, 1.0, 0.40) == {1}
    assert SR.acceptable_picks(l, 0, 1.0, 1.0, 0.60) == {2}
    assert SR.acceptable_picks(l, 0, 1.0, 1.0, 0.80) == {0}          # ties: the lower index comes first
    assert SR.acceptable_picks(l, 0, 1.0, 1.0, 0.90) == {3}
    assert SR.acceptable_picks(l, 2, 1.0, 1.0, 0.70) == {2}          # top-2: C = 4, 6
    assert SR.acceptable_picks(l, 3, 1.0, 1.0, 0.99) == {0}          # the tie at the top-k boundary keeps index 0, not 3
    assert SR.acceptable_picks(l, 0, 1.0, 0.7, 0.70) == {2}          # top-p 0.7: cumsum .5 .75 -> 2 entries
    assert SR.acceptable_picks(l, 0, 0.5, 1.0, 0.72) == {1}          # T = 0.5 squares the weights: 16, 4, 1, 1 -> C/S = .727
    assert SR.acceptable_picks(l, 0, 0.5, 1.0, 0.74) == {2}
    for tk in (0, -3, 4, 5):                                         # <= 0 or > n: all
        assert SR.acceptable_picks(l, tk, 1.0, 1.0, 0.90) == {3}
    for tp in (0.0, 1.0, 1.5):                                       # top-p applies only inside (0, 1)
        assert SR.acceptable_picks(l, 0, 1.0, tp, 0.90) == {3}
    # an exact hit of top_p is inside the error band: both prefixes count.  (Prefix 1 -> id 1; prefix 2 -> C = 4, 6
    # and u = 0.99 -> id 2.)
    assert SR.acceptable_picks(l, 0, 1.0, 0.5, 0.99) == {1, 2}
    # u within gamma of a boundary: both neighbours
    assert SR.acceptable_picks(l, 0, 1.0, 1.0, 0.5 + 1e-8) == {1, 2}
    assert SR.acceptable_picks(l, 0, 1.0, 1.0, 0.5 + 1e-5) == {2}
    # entries at -inf are never kept; nothing finite on top: no draw
    m = np.array([-np.inf, 0.0, -np.inf, 0.0], np.float32)
    assert SR.acceptable_picks(m, 3, 1.0, 1.0, 0.999999) == {3}
    assert SR.acceptable_picks(np.full(4, -np.inf, np.float32), 3, 1.0, 1.0, 0.5) == {0}
    assert SR.acceptable_picks(np.array([0, np.nan, np.inf, 1], np.float32), 0, 1.0, 0.9, 0.9) == {1}
    assert SR.acceptable_picks(np.array([0, 5, np.inf, np.inf], np.float32), 0, 1.0, 0.9, 0.9) == {2}
    # temperature: <= 1e-6 (as float32) is greedy
    assert SR.is_greedy(0.0) and SR.is_greedy(1e-6) and not SR.is_greedy(SC.JUST_ABOVE)
    assert SR.pick_set(l, 1e-6, 50, 0.95, 0.99) == {1}


def test_state_transitions_hand_cases():
    def state(n_frames, done=0, n_past=4):
        return dict(past=np.arange(32, dtype=np.int32)[None].copy(), n_past=np.array([n_past], np.int32), n_text=np.zeros(1, np.int32),
                    done=np.array([done], np.int32), n_frames=np.array([n_frames], np.int32), pos0=np.array([9], np.int32),
                    pos=np.array([-7], np.int32), codes=np.full((2, 1, 16), -7, np.int32))
    cfg = dict(audio_vocab=2048, eos=2150, frame_cap=2, row0=0, R=1)
    st = state(1)
    SR.talker_apply_row(st, cfg, 0, 123)
    assert (st["codes"][1, 0, 0], st["past"][0, 4], st["n_past"][0], st["pos"][0], st["done"][0], st["n_frames"][0]) == (123, 123, 5, 13, 0, 2)
    for code in (2150, 2048):                   # EOS, non-audio id
        st = state(1)
        SR.talker_apply_row(st, cfg, 0, code)
        assert (st["codes"][1, 0, 0], st["past"][0, 4], st["n_past"][0], st["pos"][0], st["done"][0], st["n_frames"][0]) == (-1, 4, 4, -7, 1, 2)
    st = state(2)                               # beyond the codes array: not recorded, the row ends
    SR.talker_apply_row(st, cfg, 0, 123)
    assert (st["codes"] == -7).all() and st["done"][0] == 1 and st["n_frames"][0] == 3 and st["n_past"][0] == 4
    slots = [SC.slot()]
    for nf, want in ((2, 3), (3, 3), (4, 4)):   # per-slot: an ended row's counter stops at frame_cap + 1
        st = state(nf, done=1)
        SR.talker_apply_row(st, dict(cfg, slots=slots), 0, 123)
        assert st["n_frames"][0] == want and (st["codes"] == -7).all()
    st = state(0)                               # frame budget reached
    SR.talker_apply_row(st, dict(cfg, max_frames=4), 0, 123)
    assert st["done"][0] == 1 and st["codes"][0, 0, 0] == -1
    forced = np.full((2, 1, 16), -1, np.int32)
    forced[0, 0, 0], forced[0, 0, 3] = 55, 66
    st = state(0)
    SR.talker_apply_row(st, dict(cfg, forced=forced), 0, 123)
    assert st["codes"][0, 0, 0] == 123 and st["past"][0, 4] == 55
    # code predictor: frame n_frames - 1, clamped; column group + 1
    codes = np.full((2, 1, 16), -7, np.int32)
    c2 = dict(frame_cap=2, group=2, forced=forced)
    assert SR.cp_apply_row(codes, [0], c2, 0, 8) == 66 and codes[0, 0, 3] == 8
    assert SR.cp_apply_row(codes, [2], c2, 0, 9) == 9 and codes[1, 0, 3] == 9
    before = codes.copy()
    assert SR.cp_apply_row(codes, [3], c2, 0, 10) == 10 and (codes == before).all()


def test_feedback_matches_frontend_bit_for_bit():
    rng = np.random.default_rng(5)
    H = 1024
    talker = rng.standard_normal((300, H)).astype(np.float32)
    tabs = [rng.standard_normal((64, H)).astype(np.float32) for _ in range(15)]
    pad = rng.standard_normal(H).astype(np.float32)
    for _ in range(8):
        ids = [int(rng.integers(0, 300))] + [int(x) for x in rng.integers(0, 64, 15)]
        for p in (pad, None):
            got = SR.feedback_row(ids, talker, tabs, p)
            np.testing.assert_array_equal(got.view(np.uint32), fe.feedback_embedding(ids[0], ids[1:], talker, tabs, p).view(np.uint32))
    # ids out of range or negative embed as zeros
    ids = [300] + [-1, 64] + [3] * 13
    want = np.zeros(H, np.float32)
    for g in range(2, 15):
        want += tabs[g][3]
    np.testing.assert_array_equal(SR.feedback_row(ids, talker, tabs, None), want)
    np.testing.assert_array_equal(SR.gather_row(talker, 300), np.zeros(H, np.float32))
    np.testing.assert_array_equal(SR.gather_row(talker, 299), talker[299])
    row = talker[0]
    np.testing.assert_allclose(SR.ssq_parts(row).sum(), float((row.astype(np.float64) ** 2).sum()), rtol=1e-12)
    assert SR.ssq_parts(row).shape == (H // 16,)
    np.testing.assert_array_equal(SR.xh_row([32.0, -8e6, 1e-3], [0.5, 1.0, 1.0]), [1.0, -65504.0, 6.25e-5])
    np.testing.assert_array_equal(SR.fp16_ulp([1.0, 65504.0, 0.0, 3e-8]), [2.0 ** -10, 32.0, 2.0 ** -24, 2.0 ** -24])


# ---- the GPU test's inputs: at most 5 % of the stochastic cases of a family are ambiguous -----------------------------
@pytest.mark.parametrize("slots_mode", [0, 1], ids=["scalar", "slots"])
def test_ambiguity_cap(slots_mode):
    worst = {}
    for kernel, vocabs in (("talker", sorted(SC.TALKER_VOCABS)), ("cp", SC.CP_VOCABS)):
        for V in vocabs:
            if kernel == "talker":
                cases = SC.talker_decision_cases(V, slots_mode)
                shares = SC.ambiguous_share(cases, lambda c: {r: s for r, (s, _) in SR.talker_sets(c["logits"], c["st"], c["cfg"]).items()})
            else:
                cases = SC.cp_decision_cases(V, slots_mode)
                shares = SC.ambiguous_share(cases, lambda c: SR.cp_sets(c["logits"], c["n_frames"], c["cfg"]))
            SC.share_report(f"{kernel} V={V} {'slots' if slots_mode else 'scalar'}", shares)
            assert set(shares) == set(SC.FAMILIES)
            for fam, (a, n) in shares.items():
                assert n >= 40, "too few stochastic cases to speak of a share"
                assert a <= 0.05 * n, f"{kernel} V={V} {fam}: {a} of {n} ambiguous"
                worst[kernel] = max(worst.get(kernel, 0.0), a / n)
    print("worst share per kernel:", {k: f"{100 * v:.1f} %" for k, v in worst.items()})


# ---- text slots: hold rule, EOS mask, held rows of the code predictor, the feedback's last addend ----------------------
def _hold_state(n_past, done):
    return dict(past=np.arange(32, dtype=np.int32)[None].copy(), n_past=np.array([n_past], np.int32), n_text=np.zeros(1, np.int32),
                done=np.array([done], np.int32), n_frames=np.array([1], np.int32), pos0=np.array([9], np.int32),
                pos=np.array([-7], np.int32), codes=np.full((2, 1, 16), -7, np.int32), held=np.array([-7], np.int32))


def test_hold_rule_hand_grid():
    """text_avail 5, budget 12: held exactly for a live flags-3 row with n_past in 5 .. 11 (n_past >= 1 decides alone
    where text_avail is 0)."""
    assert SC.HOLD_N_PAST == (0, 1, 4, 5, 6, 11, 12) and len(SC.hold_grid()) == 56
    seen = 0
    for n_past, flags, done in SC.hold_grid():
        st = _hold_state(n_past, done)
        cfg = dict(audio_vocab=48, eos=50, frame_cap=2, row0=0, R=1, slots=[SC.slot(max_frames=12, flags=flags)],
                   text_avail=np.array([5], np.int32))
        want = flags == 3 and not done and n_past in (5, 6, 11)
        assert SR.talker_held(st, cfg, 0) == want, (n_past, flags, done)
        assert SR.talker_held_after(st, cfg).tolist() == [int(want)]
        assert (0 in SR.talker_sets(np.zeros((1, 64), np.float32), st, cfg)) == (not want)
        seen += want
    assert seen == 3
    st = _hold_state(0, 0)
    flags3 = [SC.slot(max_frames=12, flags=3)]
    for avail, n_past, want in ((0, 0, False), (0, 1, True), (1, 1, True), (2, 1, False), (12, 11, False), (11, 11, True), (0, 12, False)):
        st["n_past"][0] = n_past
        assert SR.talker_held(st, dict(slots=flags3, text_avail=[avail]), 0) == want, (avail, n_past)
    # hold is per-slot mode with text_avail: without either nothing is held and held[] is not written
    st["n_past"][0] = 6
    assert not SR.talker_held(st, dict(slots=flags3), 0) and not SR.talker_held(st, dict(text_avail=[5]), 0)
    assert SR.talker_held_after(st, dict(slots=flags3, row0=0, R=1)).tolist() == [-7]
    # rows outside the launch keep what they had
    st3 = dict(n_past=np.array([6, 6, 6]), done=np.zeros(3, np.int32), held=np.array([-7, -7, -7], np.int32))
    cfg3 = dict(slots=[SC.slot(max_frames=12, flags=f) for f in (3, 3, 1)], text_avail=[5, 5, 5], row0=1, R=2)
    assert SR.talker_held_after(st3, cfg3).tolist() == [-7, 1, 0]


def test_eos_mask_hand_cases():
    """flags & 2: the EOS logit is -1e10 (still penalised when EOS repeats) and neither boost nor forced EOS applies;
    flags 0 and 1 are the plain row."""
    V, av, eos = 64, 48, 50
    l = np.full(V, -5.0, np.float32)
    l[eos], l[7] = 9.0, 1.0
    for flags in (0, 1, 2, 3):
        for n_past, n_text in ((31, 5), (3, 5), (3, 0)):
            st = _hold_state(n_past, 0)
            st["n_text"][0] = n_text
            st["past"][0, :] = 40                      # (an id that is on top of nothing)
            cfg = dict(audio_vocab=av, eos=eos, frame_cap=2, row0=0, R=1, slots=[SC.slot(flags=flags)])
            picks, proc = SR.talker_sets(l[None], st, cfg)[0]
            if flags & 2:
                assert picks == {7} and proc[eos] == np.float32(-1e10)
            else:
                assert picks == {eos}
                boost = min((n_past / (3 * n_text) - 0.8) / 0.7, 1.0) * 15.0 if n_text and n_past / (3 * n_text) > 0.8 else 0.0
                assert proc[eos] == np.float32(9.0) + np.float32(boost)
    st = _hold_state(3, 0)
    st["past"][0, :3] = eos                            # EOS repeats: -1e10 * 1.2
    _, proc = SR.talker_sets(l[None], st, dict(audio_vocab=av, eos=eos, row0=0, R=1, slots=[SC.slot(flags=2)]))[0]
    assert proc[eos] == np.float32(-1e10) * np.float32(1.2)
    # scalar mode has no flags
    assert SR.slot_flags(dict(), 0) == 0


def test_cp_held_hand_cases():
    V = 64
    forced = np.full((2, 1, 16), -1, np.int32)
    base = dict(V=V, frame_cap=2, group=2, slots=[SC.slot()], row0=0, R=1)
    for rec, want in ((17, 17), (-1, 0), (V, 0), (V + 5, 0), (0, 0), (V - 1, V - 1)):
        codes = np.full((2, 1, 16), -7, np.int32)
        codes[1, 0, 3] = rec
        before = codes.copy()
        cfg = dict(base, held=np.array([1], np.int32))
        assert SR.cp_held(cfg, 0) and SR.cp_sets(np.zeros((1, V), np.float32), [2], cfg) == {}
        assert SR.cp_apply_row(codes, [2], cfg, 0, 33) == want and (codes == before).all()
        assert SR.cp_feedback_codes(codes, [2], cfg, 0, want)[3] == want
        # teacher forcing overrides afterwards; the other groups' forced ids still replace the recorded ones
        forced[1, 0, 3], forced[1, 0, 5] = 21, 22
        assert SR.cp_apply_row(codes, [2], dict(cfg, forced=forced), 0, 33) == 21 and (codes == before).all()
        assert SR.cp_feedback_codes(codes, [2], dict(cfg, forced=forced), 0, 21)[3:6] == [21, -7, 22]
        forced[:] = -1
        # beyond the codes array the last frame is read and nothing is forced
        forced[1, 0, 3] = 21
        assert SR.cp_apply_row(codes, [4], dict(cfg, forced=forced), 0, 33) == want
        forced[:] = -1
        # held = 0, or scalar mode: the row decides and records
        for c2 in (dict(base, held=np.array([0], np.int32)), dict(base, held=np.array([1], np.int32), slots=None)):
            c = before.copy()
            assert not SR.cp_held(c2, 0) and SR.cp_apply_row(c, [2], c2, 0, 33) == 33 and c[1, 0, 3] == 33


def test_feedback_last_hand_cases():
    cap, H = 8, 4
    pad = np.full(H, -1.0, np.float32)
    text = np.arange(6 * H, dtype=np.float32).reshape(6, H)
    for avail in (0, 1, 3, 6):
        for nf in (0, 1, avail, avail + 1, cap, cap + 1):
            got = SR.feedback_last(pad, text, avail, nf)
            if 1 <= nf <= avail:
                assert got is not pad and (got == text[nf - 1]).all(), (avail, nf)
            else:
                assert got is pad, (avail, nf)
    assert SR.feedback_last(pad, None, 3, 1) is pad and SR.feedback_last(None, text, 3, 4) is None
    # the frame is the slot's own, not the clamped frame of the codes array: frame_cap 2, n_frames 4 -> text row 3
    assert (SR.feedback_last(pad, text, 6, 4) == text[3]).all() and SR.cp_frame(4, 2) == (1, False)
    tabs = [np.zeros((2, H), np.float32)] * 15
    row = SR.feedback_row([0] * 16, np.ones((1, H), np.float32), tabs, SR.feedback_last(pad, text, 6, 2))
    np.testing.assert_array_equal(row, np.float32(1.0) + text[1])


def test_ambiguity_cap_text_cases():
    """The stochastic rows of the text-slot cases (tests/test_gpu_sample_decisions.py): at most 5 % ambiguous per family;
    held rows make no draw and do not count."""
    total = {}
    for kernel, vocabs in (("talker", SC.TEXT_TALKER_VOCABS), ("cp", SC.TEXT_CP_VOCABS)):
        for V in vocabs:
            if kernel == "talker":
                cases = SC.text_talker_cases(V)
                shares = SC.ambiguous_share(cases, lambda c: {r: s for r, (s, _) in SR.talker_sets(c["logits"], c["st"], c["cfg"]).items()})
                held = sum(SR.talker_held(c["st"], c["cfg"], r) for c in cases for r in range(SC.TEXT_ROW0, SC.TEXT_ROW0 + SC.TEXT_R))
                assert held == 3 + 6              # the grid's three held cells + those that fill the last launch
            else:
                cases = SC.text_cp_cases(V)
                shares = SC.ambiguous_share(cases, lambda c: SR.cp_sets(c["logits"], c["n_frames"], c["cfg"]))
            SC.share_report(f"{kernel} V={V} text slots", shares)
            for fam, (a, n) in shares.items():
                assert n >= 4 and a <= 0.05 * n, f"{kernel} V={V} {fam}: {a} of {n} ambiguous"
                ta, tn = total.get((kernel, fam), (0, 0))
                total[kernel, fam] = (ta + a, tn + n)
    assert set(f for _, f in total) == {"hold", "eos_mask", "cp_held", "text_rows"}
    print("text-slot cases:", {f"{k} {f}": f"{a}/{n}" for (k, f), (a, n) in total.items()})
