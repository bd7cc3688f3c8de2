"""Float64 reference of the score of an emitted id (include/qwen3tts_engine.h: q3e_scores_reserve).

    lp = z_u - m - log(sum_{v in A} exp(z_v - m)),   z = the logit with NaN read as +inf,   m = max over A

A is every id for a code-predictor group, {v < audio_vocab} + {eos} for the talker; an id outside A (or outside the row)
has z_u = -inf.  Degenerate rows give what IEEE arithmetic gives: m = +inf or nothing above -inf -> NaN, a -inf id beside
finite ones -> -inf.  No sampler setting is an argument: the score is the model's distribution, not the sampler's."""
from __future__ import annotations

import numpy as np


def nan_as_inf(z):
    z = np.array(z, np.float64, copy=True)
    z[np.isnan(z)] = np.inf
    return z


def talker_allowed(V, audio_vocab, eos):
    """-> bool [V]: the ids the talker may emit."""
    a = np.arange(V) < audio_vocab
    if 0 <= eos < V:
        a[eos] = True
    return a


def log_prob(logits, u, allowed=None):
    """Score of id u under one row of logits (any float dtype), in float64.  allowed: bool mask, None = every id."""
    z = nan_as_inf(logits)
    if allowed is None:
        allowed = np.ones(z.shape[0], bool)
    za = z[allowed]
    zu = z[u] if 0 <= u < z.shape[0] and allowed[u] else -np.inf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = za.max() if za.size else -np.inf
        return np.float64(zu) - m - np.log(np.sum(np.exp(za - m)))


def talker_log_prob(logits, u, audio_vocab, eos):
    return log_prob(logits, u, talker_allowed(len(logits), audio_vocab, eos))


def log_probs(logits, allowed=None):
    """Scores of every id of the row at once (float64 [V]; -inf outside `allowed`)."""
    z = nan_as_inf(logits)
    if allowed is None:
        allowed = np.ones(z.shape[0], bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        za = z[allowed]
        m = za.max() if za.size else -np.inf
        return np.where(allowed, z, -np.inf) - m - np.log(np.sum(np.exp(za - m)))


def matches(got, ref, atol=1e-5, rtol=1e-6):
    """The tests' comparison: NaN with NaN and +-inf with the same infinity exactly, finite values within
    atol + rtol * |ref|.  -> (ok, error: 0 for an exact non-finite match, inf for a mismatch of kind)."""
    got, ref = float(got), float(ref)
    if np.isnan(ref) or np.isnan(got):
        ok = bool(np.isnan(ref) and np.isnan(got))
        return ok, 0.0 if ok else np.inf
    if np.isinf(ref) or np.isinf(got):
        ok = got == ref
        return ok, 0.0 if ok else np.inf
    err = abs(got - ref)
    return err <= atol + rtol * abs(ref), err
