"""enc_rvq_kernel (csrc/q3_enc.hip), the encoder's quantiser, one launch at a time through the test hook
q3t_enc_rvq_case -- the tables enc_load builds, enc_launch_rvq's own tile rule -- against the float64 reference and the
cases of tests/rvq_ref.py (whose conditions tests/test_rvq_reference.py asserts on the CPU):

  a. exact-integer data at frame counts around every edge of both tilings, both layouts: ids equal float64, no tolerance
  b. ties placed where the scan or the reduction could break them the wrong way: the lowest index wins
  c. codebook and stage geometry the loader admits and the product never ships
  d. real-valued data: every decided decision equals float64, every undecided one is within 2 * bound
  e. a frame's ids depend on nothing but the frame: the tile width, the layout, the call, its place in the call
  f. non-finite input stays inside its frame
  g. the hook refuses what enc_load refuses

The hook fills the pad columns of the clip layout with NaN and guards the codes buffer (-3), so every case here also
checks that no pad is read and no tail frame written."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import rvq_ref as R

pytestmark = pytest.mark.gpu

WIDTHS_RUN = set()        # tile widths the cases of this file launched (q3t_enc_rvq_tile of their frame counts)


@pytest.fixture(scope="module")
def tl(test_lib):
    return test_lib


def run(tl, codebook, n_sem, z, layout="stream", B=None, rc=0):
    """z [F][2 dim] -> ids [F][nq].  layout "clip": the frames as B clips of F / B columns, [B][2 dim][T] with pitch and
    NaN pads on the device; "stream": [F][2 dim], ld = T = 1."""
    E = np.ascontiguousarray(codebook, np.float32)
    nq, cb, dim = E.shape
    F = z.shape[0]
    assert z.shape == (F, 2 * dim)
    if layout == "clip":
        B = B or 1
        zz, T, stream = R.to_clip_layout(np.asarray(z, np.float32), B), F // B, 0
    else:
        zz, B, T, stream = np.ascontiguousarray(z, np.float32), F, 1, 1
    codes = np.full((F, nq), -1, np.int64)
    got = tl.q3t_enc_rvq_case(hiplib.fptr(E), nq, cb, dim, n_sem, stream, B, T, hiplib.fptr(zz), codes.ctypes.data_as(hiplib.i64p))
    assert got == rc, f"q3t_enc_rvq_case -> {got}"
    WIDTHS_RUN.add(int(tl.q3t_enc_rvq_tile(F)))
    return codes


def clips_for(n):
    """the clip count a call of n frames is laid out with: 3 where 3 divides n, else its smallest other factor (1: a prime)"""
    for B in (3, 2, 23):
        if n % B == 0:
            return B
    return 1


# ---- a. exact ids, both tile widths ------------------------------------------------------------------------------------------
# 1, 3, 4, 5, 2047: the 4-frame tile, alone, with a tail and without; 2048, 2049, 2063: the 16-frame tile without a tail, with a
# tail of 1 and of 15.  A clip call holds B * T frames, so 3 clips cannot hold most of those counts: the clip layout runs them
# with the clip count clips_for gives, and the counts of THREE_CLIPS add three-clip calls with tails of every kind, where
# frame g = b * T + t crosses a clip boundary inside a tile.
EDGES = (1, 3, 4, 5, 2047, 2048, 2049, 2063)
THREE_CLIPS = (6, 9, 2046, 2061, 2064, 2079)


@pytest.mark.parametrize("frames,layout", [(n, lay) for n in EDGES for lay in ("clip", "stream")] + [(n, "clip") for n in THREE_CLIPS])
def test_exact_ids_at_tile_edges(tl, frames, layout):
    c = R.exact_case(11, 5, 300, 8, 2, frames)
    B = clips_for(frames)
    assert frames not in THREE_CLIPS or B == 3
    got = run(tl, c.codebook, c.n_sem, c.z, layout, B)
    assert np.array_equal(got, c.ref.ids), f"{int((got != c.ref.ids).sum())} ids differ from float64"


def test_both_tile_widths_ran(tl):
    """the cases above took both kernels: a later change of the threshold cannot quietly remove the coverage"""
    assert {int(tl.q3t_enc_rvq_tile(n)) for n in EDGES} == {4, 16}
    assert int(tl.q3t_enc_rvq_tile(2047)) == 4 and int(tl.q3t_enc_rvq_tile(2048)) == 16
    for n in EDGES:
        c = R.exact_case(11, 5, 300, 8, 2, n)
        assert np.array_equal(run(tl, c.codebook, c.n_sem, c.z), c.ref.ids)
    assert WIDTHS_RUN == {4, 16}, WIDTHS_RUN


# ---- b. ties take the lowest index --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [6, 2050])
@pytest.mark.parametrize("name", [t[0] for t in R.TIES])
def test_ties_take_the_lowest_index(tl, name, frames):
    c = R.tie_case(name, frames)
    tied = next(t for n, t, _ in R.TIES if n == name)
    assert int(tl.q3t_enc_rvq_tile(frames)) == (4 if frames < 2048 else 16)
    for layout, B in (("stream", None), ("clip", 2)):
        got = run(tl, c.codebook, c.n_sem, c.z, layout, B)
        assert (got == min(tied)).all(), f"{name} {layout}: ids {sorted(set(got.ravel().tolist()))}, tied {tied}"
        assert np.array_equal(got, c.ref.ids)


# ---- c. geometry the loader admits ---------------------------------------------------------------------------------------------
GEOMETRY = [      # (cb, dim, nq, n_sem)
    (1, 4, 1, 1), (5, 8, 16, 1), (255, 8, 6, 3), (256, 4, 4, 4), (257, 8, 32, 2), (1500, 8, 6, 3), (2048, 256, 4, 4),
    (2051, 8, 16, 1), (5, 1024, 1, 1), (257, 1024, 6, 3),
]


@pytest.mark.parametrize("frames", [7, 2051])
@pytest.mark.parametrize("cb,dim,nq,n_sem", GEOMETRY)
def test_geometry_the_loader_admits(tl, cb, dim, nq, n_sem, frames):
    c = R.exact_case(cb * 31 + dim, nq, cb, dim, n_sem, frames)
    got = run(tl, c.codebook, c.n_sem, c.z, "clip", 1)
    assert np.array_equal(got, c.ref.ids), f"{int((got != c.ref.ids).sum())} of {got.size} ids differ from float64"
    if cb > 1 and frames > 100:
        assert len(set(got[:, 0].tolist())) > 1


# ---- d. real data ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product_ids(tl):
    """the product-shaped real case in one call (the 16-frame kernel), stream layout: shared by d and e"""
    c = R.real_case("product")
    assert int(tl.q3t_enc_rvq_tile(c.z.shape[0])) == 16
    return run(tl, c.codebook, c.n_sem, c.z)


@pytest.mark.parametrize("name", list(R.REAL))
def test_real_data_decisions(tl, name, product_ids):
    """Every decided decision equals float64; an undecided one is within 2 * bound, the residual following the GPU's ids.
    Measured on MI355X (undecided decisions on the GPU's path, ids differing from float64): product 61 and 0 of 33 600, small 2
    and 0 of 33 600, passes 2 and 0 of 1 800."""
    c = R.real_case(name)
    got = product_ids if name == "product" else run(tl, c.codebook, c.n_sem, c.z, "clip", 3)
    n_und, n_diff = R.grade_real(c, got)
    print(f"{name}: {n_und} of {got.size} decisions undecided, {n_diff} ids differ from float64")


# ---- e. a frame depends on nothing but the frame ---------------------------------------------------------------------------------
def test_a_frame_depends_on_nothing_but_the_frame(tl, product_ids):
    c = R.real_case("product")
    F = c.z.shape[0]
    assert F == 2100
    # in pieces below the threshold: the 4-frame kernel, other tile offsets
    cuts = [0, 1000, 1003, F]
    assert all(int(tl.q3t_enc_rvq_tile(b - a)) == 4 for a, b in zip(cuts, cuts[1:]))
    pieces = np.concatenate([run(tl, c.codebook, c.n_sem, c.z[a:b]) for a, b in zip(cuts, cuts[1:])])
    assert np.array_equal(pieces, product_ids), f"{int((pieces != product_ids).sum())} ids differ between the kernels"
    # the other layout, 3 clips of 700 columns (pitch 704: NaN pads)
    clip = run(tl, c.codebook, c.n_sem, c.z, "clip", 3)
    assert np.array_equal(clip, product_ids)
    # another frame order: other neighbours in the tile, other tiles
    perm = np.random.default_rng(5).permutation(F)
    shuf = run(tl, c.codebook, c.n_sem, c.z[perm])
    assert np.array_equal(shuf, product_ids[perm])


# ---- f. non-finite input ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [9, 2050])
def test_non_finite_input_stays_in_its_frame(tl, frames):
    c = R.exact_case(77, 6, 300, 8, 3, frames)
    dim, cb = 8, 300
    z = c.z.copy()
    f_nan, f_inf, f_ninf = 5, frames - 2, 2       # inside tiles that hold other frames, in both tilings
    z[f_nan, 3] = np.nan                          # the semantic half
    z[f_inf, 1] = np.inf
    z[f_ninf, dim + 2] = -np.inf                  # the acoustic half
    for layout, B in (("stream", None), ("clip", 1)):
        got = run(tl, c.codebook, c.n_sem, z, layout, B)
        assert (got >= 0).all() and (got < cb).all()
        clean = np.ones(frames, bool)
        clean[[f_nan, f_inf, f_ninf]] = False
        assert np.array_equal(got[clean], c.ref.ids[clean]), "a non-finite frame changed another frame's ids"
        assert (got[f_nan, :3] == 0).all(), got[f_nan]                      # every score NaN: the documented guard
        assert np.array_equal(got[f_nan, 3:], c.ref.ids[f_nan, 3:])         # the acoustic stages restart from finite input
        assert np.array_equal(got[f_inf, 3:], c.ref.ids[f_inf, 3:])
        assert np.array_equal(got[f_ninf, :3], c.ref.ids[f_ninf, :3])


# ---- g. the hook's refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,cb,dim,n_sem", [(0, 4, 4, 1), (33, 4, 4, 1), (2, 0, 4, 1), (2, -1, 4, 1), (2, 4, 0, 1), (2, 4, 2, 1),
                                             (2, 4, 6, 1), (2, 4, 1028, 1), (2, 4, 4, 0), (2, 4, 4, 3), (2, 4, 4, -1)])
def test_hook_refuses_what_the_loader_refuses(tl, nq, cb, dim, n_sem):
    E = np.zeros(max(nq, 1) * max(cb, 1) * max(dim, 1), np.float32)
    z = np.zeros(4 * 2 * max(dim, 1), np.float32)
    codes = np.zeros(4 * max(nq, 1), np.int64)
    assert tl.q3t_enc_rvq_case(hiplib.fptr(E), nq, cb, dim, n_sem, 1, 4, 1, hiplib.fptr(z), codes.ctypes.data_as(hiplib.i64p)) == -2


def test_hook_refuses_a_non_finite_codebook_and_bad_calls(tl):
    E = np.zeros((2, 4, 4), np.float32)
    z = np.zeros((4, 8), np.float32)
    codes = np.zeros((4, 2), np.int64)
    cp = codes.ctypes.data_as(hiplib.i64p)
    assert tl.q3t_enc_rvq_case(hiplib.fptr(E), 2, 4, 4, 1, 1, 4, 1, hiplib.fptr(z), cp) == 0
    for bad in (np.nan, np.inf):
        E2 = E.copy()
        E2[1, 2, 3] = bad
        assert tl.q3t_enc_rvq_case(hiplib.fptr(E2), 2, 4, 4, 1, 1, 4, 1, hiplib.fptr(z), cp) == -2
    assert tl.q3t_enc_rvq_case(hiplib.fptr(E), 2, 4, 4, 1, 1, 2, 2, hiplib.fptr(z), cp) == -2      # a stream call has T = 1
    assert tl.q3t_enc_rvq_case(hiplib.fptr(E), 2, 4, 4, 1, 0, 0, 4, hiplib.fptr(z), cp) == -2
    assert tl.q3t_enc_rvq_case(None, 2, 4, 4, 1, 1, 4, 1, hiplib.fptr(z), cp) == -2
