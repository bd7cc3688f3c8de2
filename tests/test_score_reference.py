"""tests/score_ref.py, the float64 reference of the score of an emitted id, checked from outside: against
scipy.special.log_softmax on finite rows, and by hand on the allowed-set mask, the id outside the set and the degenerate
rows.  CPU only."""
import numpy as np
import pytest
from scipy.special import log_softmax

from tests import sample_cases as SC
from tests import score_ref as R

INF, NAN = np.inf, np.nan


@pytest.mark.parametrize("V", [4, 64, 2048, 3072])
@pytest.mark.parametrize("scale", [0.1, 1.0, 50.0])
def test_full_row_is_log_softmax(V, scale):
    rng = SC.rng_for("score_ref", V, scale)
    for dtype in (np.float32, np.float64):
        z = (scale * rng.standard_normal(V)).astype(dtype)
        want = log_softmax(z.astype(np.float64))
        np.testing.assert_allclose(R.log_probs(z), want, rtol=1e-13, atol=1e-12)
        for u in (0, V - 1, int(rng.integers(V))):
            assert abs(R.log_prob(z, u) - want[u]) <= 1e-12 + 1e-13 * abs(want[u])
    assert abs(np.exp(R.log_probs(z)).sum() - 1.0) < 1e-12


@pytest.mark.parametrize("V,audio_vocab,eos", [(64, 48, 50), (3072, 2048, 2150), (100, 78, 90)])
def test_talker_mask_is_log_softmax_over_the_allowed_ids(V, audio_vocab, eos):
    rng = SC.rng_for("score_ref_mask", V)
    z = (8.0 * rng.standard_normal(V)).astype(np.float32)
    z[audio_vocab:] += 40.0          # the forbidden ids on top: they must not enter the sum or the maximum
    ids = list(range(audio_vocab)) + [eos]
    want = log_softmax(z[ids].astype(np.float64))
    allowed = R.talker_allowed(V, audio_vocab, eos)
    assert allowed.sum() == audio_vocab + 1 and allowed[eos] and not allowed[audio_vocab] and not allowed[V - 1]
    for k, u in enumerate(ids):
        assert abs(R.talker_log_prob(z, u, audio_vocab, eos) - want[k]) <= 1e-12 + 1e-13 * abs(want[k])
    # outside the set: -inf, also beyond the row and below zero
    for u in (audio_vocab, eos - 1, eos + 1, V - 1, V, V + 7, -1):
        if u != eos:
            assert R.talker_log_prob(z, u, audio_vocab, eos) == -INF
    assert abs(np.exp(R.log_probs(z, allowed)).sum() - 1.0) < 1e-12


def test_hand_cases():
    ln2, ln3 = np.log(2.0), np.log(3.0)
    # two equal logits: each ln(1/2); a third far below adds nothing measurable
    assert R.log_prob([1.0, 1.0], 0) == pytest.approx(-ln2, abs=1e-15)
    assert R.log_prob([5.0, 5.0, 5.0], 2) == pytest.approx(-ln3, abs=1e-15)
    assert R.log_prob([0.0, ln2], 1) == pytest.approx(np.log(2.0 / 3.0), abs=1e-15)
    # a shift of the row changes nothing
    assert R.log_prob([1000.0, 1000.0 + ln2], 0) == pytest.approx(np.log(1.0 / 3.0), abs=1e-12)
    # a -inf id beside finite ones: -inf; the finite ones share the mass
    assert R.log_prob([-INF, 0.0, 0.0], 0) == -INF
    assert R.log_prob([-INF, 0.0, 0.0], 1) == pytest.approx(-ln2, abs=1e-15)
    # the talker's set {0, 1} + {3}: id 2 is outside whatever its logit
    z = [0.0, 0.0, 100.0, 0.0]
    assert R.talker_log_prob(z, 2, 2, 3) == -INF
    assert R.talker_log_prob(z, 3, 2, 3) == pytest.approx(-ln3, abs=1e-15)
    assert R.talker_log_prob(z, 0, 2, 3) == pytest.approx(-ln3, abs=1e-15)


def test_degenerate_rows():
    # m = +inf (a +inf logit, or a NaN read as +inf): inf - inf, NaN for every id
    for top in (INF, NAN):
        for u in (0, 1, 2, 5):
            assert np.isnan(R.log_prob([0.0, top, -1.0], u))
        assert np.isnan(R.talker_log_prob([0.0, top, 9.0, 1.0], 0, 2, 3))
    # ... but only inside the allowed set: a NaN among the forbidden ids is not seen
    assert R.talker_log_prob([0.0, 0.0, NAN, 0.0], 0, 2, 3) == pytest.approx(-np.log(3.0), abs=1e-15)
    # nothing above -inf: NaN, for ids inside and outside
    for u in (0, 2, 7):
        assert np.isnan(R.log_prob([-INF, -INF, -INF], u))
    assert np.isnan(R.talker_log_prob([-INF, -INF, 5.0, -INF], 0, 2, 3))
    assert np.isnan(R.talker_log_prob([-INF, -INF, 5.0, -INF], 2, 2, 3))
    # one finite id holds all the mass
    assert R.log_prob([-INF, 3.0, -INF], 1) == 0.0
    assert R.log_prob([-INF, 3.0, -INF], 0) == -INF
    assert R.nan_as_inf([NAN, 1.0, -INF]).tolist() == [INF, 1.0, -INF]


def test_matches_rule():
    assert R.matches(NAN, NAN) == (True, 0.0)
    assert R.matches(-INF, -INF) == (True, 0.0)
    assert not R.matches(NAN, -INF)[0] and not R.matches(-INF, NAN)[0]
    assert not R.matches(-1e30, -INF)[0] and not R.matches(INF, -INF)[0] and not R.matches(0.0, NAN)[0]
    assert R.matches(-3.0 - 1.2e-5, -3.0)[0] and not R.matches(-3.0 - 1.4e-5, -3.0)[0]
    assert R.matches(-300.0 - 3.0e-4, -300.0)[0] and not R.matches(-300.0 - 3.2e-4, -300.0)[0]


def test_every_family_of_the_sampling_cases_has_the_expected_kind():
    """The families the GPU test runs: which give a finite score, which NaN."""
    rng = SC.rng_for("score_ref_families")
    for fam in SC.FAMILIES:
        z = SC.make_logits(fam, rng, 64, 64, 50, 1.0)
        lp = R.log_probs(z)
        if fam in ("nan_top", "inf_top", "all_ninf"):
            assert np.isnan(lp).all(), fam
        elif fam == "few_finite":
            assert np.isfinite(lp).sum() == 3 and (lp[~np.isfinite(lp)] == -INF).all()
        else:
            assert np.isfinite(lp).all() and abs(np.exp(lp).sum() - 1.0) < 1e-12, fam
