"""float64 reference of the encoder's split residual VQ (enc_rvq_kernel, csrc/q3_enc.hip) and the cases its tests run --
test infrastructure, no GPU.

The kernel's contract, restated: per frame, stage q scores every entry j of codebook q as s_j = ||e_j||^2 - 2 r.e_j, takes
the LOWEST index among the smallest scores, and subtracts that entry from the residual r; r starts from the semantic
projection and restarts from the acoustic one at stage n_sem.  rvq_reference does that in float64 on the raw scores (no
square root, no distance: the order of s_j is the order of ||r - e_j||, and the tie rule is on s_j).
tests/test_rvq_reference.py pins it against enc_ref.rvq_encode on the two golden configurations.

Every case builder asserts, on the CPU, the condition that makes its case a fair test of an fp32 kernel:

  exact   entries and inputs are multiples of 1/4, so every product is a multiple of 1/16 and every partial sum of the fma
          chain, n2, the scores and all residuals are multiples of 1/16.  A multiple of 1/16 below 2^24 / 16 in magnitude is
          an fp32 number, so while max_j (n2_j + 2 sum_d |r_d||e_jd|) -- which bounds every one of those magnitudes -- stays
          below 2^20 at every stage the kernel rounds nothing: its scores ARE the float64 scores, its ids the float64 ids.
  tie     exact data in which two (or three) chosen entries score the same and strictly below every other entry.
  real    Gaussian data at the codebook scale of weights.make_synthetic_enc.  Per (frame, stage) the kernel's score is within
              bound = (dim + 3) * 2^-24 * max_j (n2_j + 2 sum_d |r_d||e_jd|)
          of the float64 one (dim fma roundings, the rounding of n2, the final multiply-subtract), so a decision whose
          float64 gap between best and second best exceeds 2 * bound is DECIDED and must come out the same; at most 1 % of a
          case's decisions may be undecided."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

U32 = 2.0 ** -24          # fp32 unit roundoff
UNDECIDED_CAP = 0.01      # of a real case's decisions


@dataclass
class RvqResult:
    ids: np.ndarray       # int64 [F][nq]  the float64 arg-min (lowest index among equal scores)
    gap: np.ndarray       # [F][nq]  second smallest score - smallest (inf with one entry)
    excess: np.ndarray    # [F][nq]  score of the id the residual followed - smallest
    bound: np.ndarray     # [F][nq]  the fp32 forward error bound of the stage's scores
    mag: np.ndarray       # [nq]     max over frames and entries of n2_j + 2 sum_d |r_d||e_jd|


def rvq_reference(zs, za, codebook, n_sem, forced=None) -> RvqResult:
    """zs, za [F][dim]: the semantic and the acoustic projection of F frames; codebook [nq][cb][dim].  forced [F][nq]: the
    residual follows these ids (e.g. the GPU's own) instead of the arg-min; ids, gap and bound are then those met on that path."""
    E = np.asarray(codebook, np.float64)
    nq, cb, dim = E.shape
    zs, za = np.asarray(zs, np.float64), np.asarray(za, np.float64)
    F = zs.shape[0]
    ids = np.zeros((F, nq), np.int64)
    gap = np.full((F, nq), np.inf)
    excess = np.zeros((F, nq))
    bound = np.zeros((F, nq))
    mag = np.zeros(nq)
    rows = np.arange(F)
    r = None
    for q in range(nq):
        if q == 0 or q == n_sem:
            r = (zs if q == 0 else za).copy()
        n2 = (E[q] * E[q]).sum(1)
        s = n2[None, :] - 2.0 * (r @ E[q].T)
        m = (n2[None, :] + 2.0 * (np.abs(r) @ np.abs(E[q]).T)).max(1)
        idx = s.argmin(1)                      # numpy: the first (lowest) index of the minimum
        best = s[rows, idx]
        if cb > 1:
            gap[:, q] = np.partition(s, 1, axis=1)[:, 1] - best
        use = idx if forced is None else np.asarray(forced)[:, q]
        ids[:, q] = idx
        excess[:, q] = s[rows, use] - best
        bound[:, q] = (dim + 3) * U32 * m
        mag[q] = m.max() if F else 0.0
        r = r - E[q][use]
    return RvqResult(ids, gap, excess, bound, mag)


def split(z):
    """z [F][2 dim] (a frame's semantic | acoustic halves, the stream layout) -> (zs, za)"""
    d = z.shape[1] // 2
    return z[:, :d], z[:, d:]


def to_clip_layout(z, B):
    """[F][2 dim] frames, F = B * T, frame g = b * T + t -> [B][2 dim][T] as enc_run hands the quantiser its input"""
    F, C = z.shape
    assert F % B == 0
    return np.ascontiguousarray(z.reshape(B, F // B, C).transpose(0, 2, 1))


# ---- cases -----------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    codebook: np.ndarray  # f32 [nq][cb][dim]
    n_sem: int
    z: np.ndarray         # f32 [F][2 dim]
    ref: RvqResult

    @property
    def shape(self):
        return self.codebook.shape


def assert_exact(case: Case):
    """the exact-integer condition, from the case's own data"""
    for a in (case.codebook, case.z):
        assert np.array_equal(a * 4, np.round(a * 4)), "not multiples of 1/4"
    assert case.ref.mag.max() * 16 < 2 ** 24, f"magnitude {case.ref.mag.max() * 16:.0f} / 16 leaves fp32's integers"


@functools.lru_cache(maxsize=None)
def exact_case(seed, nq, cb, dim, n_sem, frames) -> Case:
    r = np.random.default_rng(seed)
    E = (r.integers(-4, 5, (nq, cb, dim)) / 4).astype(np.float32)
    z = (r.integers(-8, 9, (frames, 2 * dim)) / 4).astype(np.float32)
    c = Case(E, n_sem, z, rvq_reference(*split(z), E, n_sem))
    assert_exact(c)
    return c


# tie placements: (name, the tied indices, cb).  Thread tid scores j = p * 1024 + e * 256 + tid; a wave is 64 lanes.
TIES = [
    ("same_thread_e", (10, 266), 600),
    ("same_thread_pass", (10, 1034), 1300),
    ("neighbour_lanes", (20, 21), 64),
    ("wave_edge_63_64", (63, 64), 300),
    ("wave_edge_255_256", (255, 256), 300),
    ("last_entry_clamped", (5, 299), 300),        # cb - 1, cb no multiple of 256: threads past cb re-read entry cb - 1
    ("three_way", (7, 300, 1100), 1200),
]


@functools.lru_cache(maxsize=None)
def tie_case(name, frames) -> Case:
    """dim 8, two stages, n_sem 1.  Stage 0: the tied entries are DUPLICATES (one vector c0) and the semantic input is c0 plus
    a per-frame offset.  Stage 1 (the acoustic restart): the tied entries are DISTINCT, c1 + u_k for orthogonal u_k of one
    length, and the acoustic input is c1 plus a per-frame offset orthogonal to every u_k: midway.  Every other entry is
    4 away in coordinate 0."""
    tied, cb = next((t, c) for n, t, c in TIES if n == name)
    dim = 8
    r = np.random.default_rng(sum(name.encode()) * 7 + frames)
    E = (r.integers(-2, 3, (2, cb, dim)) / 4).astype(np.float32)
    c = (r.integers(-2, 3, (2, dim)) / 4).astype(np.float32)
    E[:, :, 0] = c[:, None, 0] + 4.0
    u = np.zeros((3, dim), np.float32)
    u[0, 1], u[1, 1], u[2, 2] = 0.5, -0.5, 0.5
    for k, j in enumerate(tied):
        E[0, j] = c[0]
        E[1, j] = c[1] + u[k]
    off = np.zeros((frames, 2, dim), np.float32)
    off[:, :, 3:] = r.integers(-1, 2, (frames, 2, dim - 3)) / 4
    z = (c[None] + off).reshape(frames, 2 * dim).astype(np.float32)
    case = Case(E, 1, z, rvq_reference(*split(z), E, 1))
    assert_exact(case)
    # the fair-test condition in float64: the tied scores are equal, and strictly below every other score
    rr = split(z)
    for q in range(2):
        rq = rr[q].astype(np.float64)      # (stage 1 = n_sem restarts from the acoustic half)
        Eq = E[q].astype(np.float64)
        s = (Eq * Eq).sum(1)[None] - 2.0 * rq @ Eq.T
        t = s[:, list(tied)]
        assert (t == t[:, :1]).all(), f"{name} stage {q}: the tied scores differ"
        rest = np.delete(s, list(tied), axis=1)
        assert (rest.min(1) > t[:, 0]).all(), f"{name} stage {q}: another entry scores as low"
    assert (case.ref.ids == min(tied)).all()
    return case


# real-valued cases: (nq, cb, dim, n_sem, frames)
REAL = {
    "product": (16, 2048, 256, 1, 2100),      # the product's own quantiser, above the 16-frame threshold
    "small": (16, 64, 16, 1, 2100),           # tests' tiny table
    "passes": (6, 1500, 64, 3, 300),          # two passes of 1024 entries with a clamped tail, three semantic stages
}


def real_data(name):
    """codebooks as weights.make_synthetic_enc draws them (0.9 * 0.85^place / sqrt(dim) per component), inputs at the scale of
    the first stage's entries"""
    nq, cb, dim, n_sem, frames = REAL[name]
    r = np.random.default_rng(1000 + sum(name.encode()))
    place = np.array([q if q < n_sem else q - n_sem for q in range(nq)])
    E = (0.9 * (0.85 ** place)[:, None, None] * r.standard_normal((nq, cb, dim)) / np.sqrt(dim)).astype(np.float32)
    z = (0.9 * r.standard_normal((frames, 2 * dim)) / np.sqrt(dim)).astype(np.float32)
    return E, n_sem, z


@functools.lru_cache(maxsize=None)
def real_case(name) -> Case:
    E, n_sem, z = real_data(name)
    c = Case(E, n_sem, z, rvq_reference(*split(z), E, n_sem))
    und = undecided(c.ref)
    assert und.sum() <= UNDECIDED_CAP * und.size, f"{name}: {int(und.sum())} of {und.size} decisions undecided"
    return c


def undecided(res: RvqResult) -> np.ndarray:
    return ~(res.gap > 2.0 * res.bound)


def grade_real(case: Case, got: np.ndarray):
    """GPU ids of a real case against float64, the residual following the GPU's ids -> (undecided decisions on that path, ids that
    differ from the float64 ids of the case).  Asserts: a decided decision equals the float64 arg-min, an undecided one is
    within 2 * bound of the smallest score."""
    nq, cb, _ = case.shape
    assert got.shape == case.ref.ids.shape and (got >= 0).all() and (got < cb).all()
    path = rvq_reference(*split(case.z), case.codebook, case.n_sem, forced=got)
    und = undecided(path)
    wrong = ~und & (got != path.ids)
    assert not wrong.any(), f"{int(wrong.sum())} decided decisions differ, first (frame, stage) {np.argwhere(wrong)[0].tolist()}"
    far = und & (path.excess > 2.0 * path.bound)
    assert not far.any(), f"{int(far.sum())} undecided decisions farther than 2 * bound, first {np.argwhere(far)[0].tolist()}"
    return int(und.sum()), int((got != case.ref.ids).sum())


# ---- the first conv (enc_conv_in_kernel): one input channel, k causal taps ---------------------------------------------------
def conv_in_reference(x, w, bias=None, left=None):
    """x [B][n], w [cout][k], bias [cout], left [B][k - 1] = what stands left of column 0 (None: zeros, a whole clip) ->
    (y [B][cout][n] float64, sum of magnitudes |bias| + sum_k |w_k||x| per output, the k - 1 samples the next call carries)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, n = x.shape
    cout, k = w.shape
    left = np.zeros((B, k - 1)) if left is None else np.asarray(left, np.float64)
    xx = np.concatenate([left, x], 1)                                     # [B][k - 1 + n]
    win = np.stack([xx[:, j:j + n] for j in range(k)], -1)                # [B][n][k]: tap j reads column l + j - (k - 1)
    b = np.zeros(cout) if bias is None else np.asarray(bias, np.float64)
    y = np.einsum("bnk,ck->bcn", win, w) + b[None, :, None]
    mag = np.einsum("bnk,ck->bcn", np.abs(win), np.abs(w)) + np.abs(b)[None, :, None]
    return y, mag, xx[:, xx.shape[1] - (k - 1):]
