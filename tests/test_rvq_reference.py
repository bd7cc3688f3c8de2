"""tests/rvq_ref.py on the CPU: the float64 split RVQ pinned against enc_ref.rvq_encode on the two golden configurations, and
every case builder of tests/test_gpu_enc_rvq.py run with the condition that makes its case a fair test (exactness, the
ties, at most 1 % undecided decisions).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from qwen3_tts_axera_russian_amd import weights as W
from tests import enc_common as C
from tests import rvq_ref as R
from tests.enc_ref import rvq_encode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mimi_encode_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(C.CASES))
def test_reference_is_enc_refs_rvq(gold, name):
    """same ids as enc_ref.rvq_encode (float64 distances) from the fixture's embeddings, free and following forced ids"""
    keys = json.loads(bytes(gold[f"{name}.keys"]).decode())
    state = C.seeded_state(C.CASES[name]["seed"], [(k, tuple(s)) for k, s in keys])
    _, t, _ = W.state_to_enc(state, json.loads(bytes(gold[f"{name}.config"]).decode()), 16)
    prog = np.asarray(t["enc.program"])
    proj = np.asarray(t[f"enc.op{len(prog) - 2}.weight"], np.float64)[:, :, 0]
    books = np.asarray(t[f"enc.op{len(prog) - 1}.codebook"], np.float64)
    n_sem = int(prog[-1][6])
    for n in C.CASES[name]["lengths"]:
        z = proj @ gold[f"{name}.embedding{n}"].astype(np.float64)        # [2 dim][T]
        codes, _, _ = rvq_encode(z, books, n_sem)
        res = R.rvq_reference(*R.split(z.T), books, n_sem)
        assert np.array_equal(res.ids, codes) and np.array_equal(codes, gold[f"{name}.codes{n}"])
        assert (res.excess == 0).all() and (res.gap >= 0).all()
        forced = (codes + 1 + np.arange(codes.shape[1])[None, :]) % books.shape[1]   # some other path
        fc, _, ratio = rvq_encode(z, books, n_sem, forced=forced)
        fres = R.rvq_reference(*R.split(z.T), books, n_sem, forced=forced)
        assert np.array_equal(fres.ids, fc)
        assert ((fres.excess > 0) == (ratio > 1)).all()


def test_reference_takes_the_lowest_index_and_restarts():
    E = np.zeros((3, 4, 4))
    E[0, 1] = E[0, 3] = [1, 0, 0, 0]
    E[1, 2] = [0, 1, 0, 0]
    E[2, 0] = E[2, 1] = [0, 0, 5, 0]
    E[2, 2] = E[2, 3] = [0, 0, 6, 0]
    zs, za = np.array([[1.0, 1, 0, 0]]), np.array([[0.0, 0, 6, 0]])
    res = R.rvq_reference(zs, za, E, 2)
    # stage 0: entries 1 and 3 tie -> 1; stage 1 continues [0, 1, 0, 0] -> 2; stage 2 restarts from za -> 2 (of 2, 3)
    assert res.ids.tolist() == [[1, 2, 2]]
    assert res.gap[0, 0] == 0 and res.gap[0, 2] == 0 and res.gap[0, 1] > 0


def test_exact_cases_are_exact():
    c = R.exact_case(1, 5, 300, 8, 2, 2063)
    R.assert_exact(c)
    assert len({tuple(r) for r in c.ref.ids.tolist()}) > 100          # the frames differ: a mix-up of frames shows
    assert (c.ref.gap == 0).any()                                     # and small integers tie by themselves
    R.assert_exact(R.exact_case(2, 1, 5, 1024, 1, 40))
    R.assert_exact(R.exact_case(3, 32, 257, 8, 2, 40))
    bad = R.Case(c.codebook * np.float32(4096), c.n_sem, c.z * np.float32(4096), c.ref)
    bad.ref = R.rvq_reference(*R.split(bad.z), bad.codebook, bad.n_sem)
    with pytest.raises(AssertionError):
        R.assert_exact(bad)


@pytest.mark.parametrize("name", [t[0] for t in R.TIES])
def test_tie_cases_tie(name):
    for frames in (6, 50):
        c = R.tie_case(name, frames)      # the builder asserts equal scores strictly below every other
        tied = next(t for n, t, _ in R.TIES if n == name)
        assert (c.ref.ids == min(tied)).all() and (c.ref.gap == 0).all()


@pytest.mark.parametrize("name", list(R.REAL))
def test_real_cases_are_decided(name):
    c = R.real_case(name)                 # the builder asserts the 1 % cap
    und = R.undecided(c.ref)
    print(f"{name}: {int(und.sum())} of {und.size} decisions undecided")
    assert len(set(c.ref.ids[:, 0].tolist())) > min(c.shape[1], c.ref.ids.shape[0]) // 4      # not degenerate
    # the float64 ids grade themselves: nothing differs, every excess is 0
    n_und, n_diff = R.grade_real(c, c.ref.ids)
    assert n_und == int(und.sum()) and n_diff == 0
    # and a wrong id at a decided decision is caught
    f, q = np.argwhere(~und)[0]
    wrong = c.ref.ids.copy()
    wrong[f, q] = (wrong[f, q] + 1) % c.shape[1]
    with pytest.raises(AssertionError):
        R.grade_real(c, wrong)


def test_fp32_residual_stays_inside_the_bound():
    """The kernel carries r in fp32 (one rounding per component and stage), the reference in float64.  On the real cases,
    ids chosen from float64 scores of an fp32-carried residual pass the float64 grading: the drift is far inside the bound."""
    for name in ("small", "passes"):
        c = R.real_case(name)
        E = c.codebook
        nq, cb, dim = E.shape
        zs, za = R.split(c.z)
        ids = np.zeros(c.ref.ids.shape, np.int64)
        for q in range(nq):
            if q == 0 or q == c.n_sem:
                r = (zs if q == 0 else za).copy()
            Eq = E[q].astype(np.float64)
            s = (Eq * Eq).sum(1)[None] - 2.0 * r.astype(np.float64) @ Eq.T
            ids[:, q] = s.argmin(1)
            r = (r - E[q][ids[:, q]]).astype(np.float32)
        R.grade_real(c, ids)


@pytest.mark.parametrize("k,cout,bias", [(1, 1, False), (2, 5, True), (7, 32, True), (16, 5, False)])
def test_conv_in_reference_is_a_causal_conv1d(k, cout, bias):
    r = np.random.default_rng(k)
    x, w = r.standard_normal((3, 40)), r.standard_normal((cout, k))
    b = r.standard_normal(cout) if bias else None
    y, mag, carry = R.conv_in_reference(x, w, b)
    want = F.conv1d(F.pad(torch.from_numpy(x)[:, None], (k - 1, 0)), torch.from_numpy(w)[:, None],
                    torch.from_numpy(b) if bias else None).numpy()
    assert np.abs(y - want).max() <= 1e-12 and (mag >= np.abs(y) - 1e-12).all()
    assert np.array_equal(carry, x[:, 40 - (k - 1):])
    # two pushes carrying k - 1 samples are the whole clip; a push shorter than the history keeps its older part
    y1, _, h1 = R.conv_in_reference(x[:, :3], w, b)
    y2, _, h2 = R.conv_in_reference(x[:, 3:], w, b, left=h1)
    assert np.abs(np.concatenate([y1, y2], 2) - y).max() <= 1e-12 and np.array_equal(h2, carry)
    assert h1.shape == (3, k - 1) and np.array_equal(h1[:, max(k - 1 - 3, 0):], x[:, max(3 - (k - 1), 0):3])
