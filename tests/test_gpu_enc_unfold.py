"""The encoder's strided-conv input kernels, one launch each through the test hooks, against tests/enc_unfold_ref.py (pinned
on the CPU by tests/test_glue_ops_reference.py):

  enc_unfold_kernel (csrc/q3_enc.hip)                 q3t_enc_unfold_case: ragged whole clips
  enc_stream_unfold_kernel (csrc/q3_enc_stream.hip)   q3t_enc_stream_unfold_case: one push; the test drives whole streams call
                                                      by call, the history block going in and coming back
  enc_stream_emit_kernel                              q3t_enc_stream_emit_case

All three move data: without ELU the outputs are compared bit for bit.  With ELU (expm1f on values < 0) the clip kernel is
within voc_conv_ref.ELU_ERR of float64 with +-0 unchanged (the device's expm1f returns +0 for -0: the kernels once applied it from
<= 0 on and lost the sign, which test_clip_unfold and test_stream_unfold found), and the stream kernel gives the clip kernel's bits.  The hooks hold
NaN in the input's pad columns (the tests also in the skipped columns and past a clip's own length) and guard every word the
kernel is not to write: the columns from the output count on, other streams' history rows, the rows between the emitted
frames, 32 words behind each buffer (-3)."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import enc_unfold_ref as E
from tests.voc_conv_ref import ELU_ERR

pytestmark = pytest.mark.gpu

MAX_STREAMS = 4
STREAMS = np.array([2, 0], np.int32)        # B = 2 entries over a swapped map; streams 1 and 3 are not named
WORST = {}


@pytest.fixture(scope="module")
def tl(test_lib):
    yield test_lib
    print("worst ELU error / ELU_ERR per kernel:", {k: float(f"{v:.3g}") for k, v in sorted(WORST.items())})


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clip_unfold(tl, x, lens, k, s, replicate, elu, rc=0):
    B, Cin, Lmax = x.shape
    y = np.full((B, Cin * k, -(-Lmax // s) if s > 0 else Lmax), np.nan, np.float32)
    got = tl.q3t_enc_unfold_case(hiplib.fptr(f32(x)), B, Cin, hiplib.iptr(np.ascontiguousarray(lens, np.int32)), k, s, replicate, elu,
                                 hiplib.fptr(y))
    assert got == rc, f"q3t_enc_unfold_case -> {got}"
    return y


def stream_unfold(tl, x, skip, n_in, n_out, k, s, replicate, elu, finish, hist, streams, before, rc=0):
    """x [B][Cin][skip + n_in]; hist [MAX_STREAMS][Cin][k - 1] is updated in place -> y [B][Cin * k][n_out]"""
    B, Cin, _ = x.shape
    y = np.full((B, Cin * k, n_out), np.nan, np.float32)
    xs = f32(x) if x.size else np.zeros(1, np.float32)
    got = tl.q3t_enc_stream_unfold_case(hiplib.fptr(xs), B, Cin, skip, n_in, n_out, k, s, replicate, elu, finish, hiplib.fptr(hist),
                                        hist.shape[0], hiplib.iptr(np.ascontiguousarray(streams, np.int32)),
                                        hiplib.iptr(np.ascontiguousarray(before, np.int32)), hiplib.fptr(y))
    assert got == rc, f"q3t_enc_stream_unfold_case -> {got}"
    return y


def check_elu(key, y, v, what):
    """y = the kernel's ELU of the moved values v: untouched above 0 and at +-0, within ELU_ERR of float64 below"""
    keep = ~(v < 0)
    assert np.array_equal(bits(y)[keep], bits(v)[keep]), f"{what}: a value >= 0 (or -0) changed"
    err = np.abs(y.astype(np.float64) - E.elu64(v))[~keep]
    if err.size:
        WORST[key] = max(WORST.get(key, 0.0), float(err.max()) / ELU_ERR)
        assert err.max() <= ELU_ERR, f"{what}: ELU off by {err.max():.3e}"


def data(r, shape):
    """N(0, 1.5) inside [-8, 8] (ELU_ERR's range) with +-0 among the values"""
    x = np.clip(1.5 * r.standard_normal(shape), -8, 8).astype(np.float32)
    flat = x.reshape(-1)
    flat[::5] = np.array([-0.0, 0.0], np.float32)[np.arange(len(flat[::5])) % 2]
    return x


@pytest.mark.parametrize("Cin", [1, 3])
@pytest.mark.parametrize("k,s,replicate,elu", E.GEOMETRIES)
def test_clip_unfold(tl, k, s, replicate, elu, Cin):
    r = np.random.default_rng([k, s, replicate, elu, Cin])
    all_lens = E.CLIP_LENS(s)
    batches = [tuple(all_lens[i:i + 3]) for i in range(0, len(all_lens), 3)] + [tuple(all_lens[::-1][:3])] + [(n,) for n in all_lens]
    for lens in batches:
        Lmax = max(lens)
        x = np.full((len(lens), Cin, Lmax), np.nan, np.float32)
        for b, n in enumerate(lens):
            x[b, :, :n] = data(r, (Cin, n))
        y = clip_unfold(tl, x, lens, k, s, replicate, elu)
        v = E.clip_unfold(x, lens, k, s, replicate)
        what = f"k={k} s={s} replicate={replicate} elu={elu} Cin={Cin} lens={lens}"
        assert not np.isnan(y).any(), f"{what}: a NaN of the pad or of the columns past a clip's own length came through"
        for b, n in enumerate(lens):
            assert not bits(y[b, :, -(-n // s):]).any(), f"{what}: columns past ceil(len / s) are +0"
        if elu:
            check_elu("enc_unfold", y, v, what)
        else:
            assert np.array_equal(bits(y), bits(v)), what
        if len(lens) > 1:       # clip b alone: the same bits
            for b, n in enumerate(lens):
                one = clip_unfold(tl, x[b:b + 1, :, :n], (n,), k, s, replicate, elu)
                assert np.array_equal(bits(one[0]), bits(y[b, :, :one.shape[2]])), f"{what}: clip {b} alone differs"


def run_stream(tl, x, k, s, replicate, elu, pushes, skip, r):
    """x [2][Cin][T]: entry b is stream STREAMS[b].  Drives the pushes through the hook and the reference side by side; -> the
    outputs side by side [2][Cin * k][ceil(T / s)]"""
    B, Cin, T = x.shape
    hist = np.zeros((MAX_STREAMS, Cin, k - 1), np.float32)
    hist[1], hist[3] = 7.5, -2.25                       # (the hook keeps the unnamed rows off the device and hands them back)
    refs = [E.StreamUnfold(Cin, k, s, replicate) for _ in range(B)]
    at, ys = 0, []
    for n_in, fin in pushes:
        before = refs[0].before
        n_out = E.stream_counts(before, n_in, fin, s)
        new = x[:, :, at:at + n_in]
        at += n_in
        want = np.stack([ref.push(new[b], fin) for b, ref in enumerate(refs)])
        xin = np.concatenate([np.full((B, Cin, skip), np.nan, np.float32), new], axis=2)
        prev = hist.copy()
        if n_in == 0 and n_out == 0:                    # the walk launches nothing for such a push, and the hook says so
            stream_unfold(tl, xin, skip, 0, 0, k, s, replicate, elu, fin, hist, STREAMS, [before] * B, rc=-2)
            assert np.array_equal(bits(hist), bits(prev))
            continue
        y = stream_unfold(tl, xin, skip, n_in, n_out, k, s, replicate, elu, fin, hist, STREAMS, [before] * B)
        assert not np.isnan(y).any(), "a NaN of the skipped or pad columns came through"
        ys.append(y)
        if not elu:
            assert np.array_equal(bits(y), bits(want))
        assert np.array_equal(bits(hist[[1, 3]]), bits(prev[[1, 3]]))
        for b, ref in enumerate(refs):
            row, was = hist[STREAMS[b]], prev[STREAMS[b]]
            if fin:
                assert np.array_equal(bits(row), bits(was)), "a finishing push leaves the history alone"
            else:
                cnt = ref.cnt()
                assert np.array_equal(bits(row[:, :cnt]), bits(ref.carry[:, :cnt])), "the carry is not the reference's"
                assert np.array_equal(bits(row[:, cnt:]), bits(was[:, cnt:])), "a word past the live carry moved"
    assert at == T
    return np.concatenate(ys, axis=2)


@pytest.mark.parametrize("skip", [0, 5])
@pytest.mark.parametrize("k,s,replicate,elu", E.GEOMETRIES)
def test_stream_unfold(tl, k, s, replicate, elu, skip):
    r = np.random.default_rng([k, s, replicate, elu, skip])
    Cin = 2
    for T in E.STREAM_T(s):
        x = data(r, (2, Cin, T))
        v = E.clip_unfold(x, (T, T), k, s, replicate)
        clip = clip_unfold(tl, x, (T, T), k, s, replicate, elu)
        cuts = dict(E.splits(T, s, 5))
        if T % s:
            cuts["tail out of the carry"] = [(T, 0), (0, 1)]
        for name, pushes in cuts.items():
            y = run_stream(tl, x, k, s, replicate, elu, pushes, skip, r)
            what = f"k={k} s={s} replicate={replicate} elu={elu} T={T} skip={skip} split {name}"
            assert y.shape == clip.shape, what
            assert np.array_equal(bits(y), bits(clip)), f"{what}: the pushes side by side are not the clip's unfold"
            if elu:
                check_elu("enc_stream_unfold", y, v, what)
            else:
                assert np.array_equal(bits(y), bits(v)), what


def test_stream_unfold_entries_at_different_totals(tl):
    """one launch over two streams at different totals that give the same n_out: each entry has its own carry count"""
    k, s, Cin = 8, 4, 2
    r = np.random.default_rng(3)
    hist = data(r, (MAX_STREAMS, Cin, k - 1))
    before = [6, 9]                                     # 6 and 5 live carry columns; 13 // 4 - 1 = 16 // 4 - 2 = 2 outputs
    refs = []
    for b in range(2):
        ref = E.StreamUnfold(Cin, k, s, 0)
        ref.before = before[b]
        ref.carry[:] = hist[STREAMS[b]]
        refs.append(ref)
    x = data(r, (2, Cin, 7))
    want = np.stack([ref.push(x[b], 0) for b, ref in enumerate(refs)])
    y = stream_unfold(tl, x, 0, 7, 2, k, s, 0, 0, 0, hist, STREAMS, before)
    assert np.array_equal(bits(y), bits(want))
    for b, ref in enumerate(refs):
        assert np.array_equal(bits(hist[STREAMS[b]][:, :ref.cnt()]), bits(ref.carry[:, :ref.cnt()]))
    stream_unfold(tl, x, 0, 7, 2, k, s, 0, 0, 0, hist, STREAMS, [6, 8], rc=-2)      # 8 + 7 gives 1 output, not 2


@pytest.mark.parametrize("C", [1, 255, 256, 257, 512])
def test_stream_emit(tl, C):
    r = np.random.default_rng(C)
    GUARD = 0x7fc5a5a5
    off = np.array([4, 0, 9], np.int32)
    for n in (1, 3):
        for skip in (0, 5):
            y = r.standard_normal((3, C, skip + n)).astype(np.float32)
            y[:, :, :skip] = np.nan
            rows = 9 + n + 2
            out = np.zeros((rows, C), np.float32)
            got = tl.q3t_enc_stream_emit_case(hiplib.fptr(y), 3, C, skip, n, hiplib.iptr(off), rows, hiplib.fptr(out))
            assert got == 0, f"q3t_enc_stream_emit_case -> {got}"
            want = E.emit(y, skip, n, off, rows, GUARD)
            assert (want == GUARD).any()
            assert np.array_equal(bits(out), want), f"C={C} n={n} skip={skip}"


def test_hook_refusals(tl):
    x = np.zeros((2, 1, 16), np.float32)
    clip_unfold(tl, x, (16, 9), 8, 4, 0, 0)
    clip_unfold(tl, x, (16, 0), 8, 4, 0, 0, rc=-2)
    clip_unfold(tl, x, (16, 9), 3, 4, 0, 0, rc=-2)          # fewer taps than the stride
    clip_unfold(tl, x, (16, 9), 8, 0, 0, 0, rc=-2)
    clip_unfold(tl, x, (16, 9), 8, 4, 2, 0, rc=-2)
    hist = np.zeros((MAX_STREAMS, 1, 7), np.float32)
    ok = lambda **kw: dict(dict(skip=0, n_in=16, n_out=4, k=8, s=4, replicate=0, elu=0, finish=0, hist=hist, streams=STREAMS, before=[0, 0]), **kw)
    stream_unfold(tl, x, **ok())
    stream_unfold(tl, x, rc=-2, **ok(n_out=5))                                   # not what the totals give
    stream_unfold(tl, x, rc=-2, **ok(streams=[2, 2]))
    stream_unfold(tl, x, rc=-2, **ok(streams=[2, 4]))
    stream_unfold(tl, x, rc=-2, **ok(before=[0, -4]))
    stream_unfold(tl, x, rc=-2, **ok(k=3))
    stream_unfold(tl, x, rc=-2, **ok(k=40, hist=np.zeros((MAX_STREAMS, 1, 39), np.float32)))      # more than 32 carried columns
    y = np.zeros((3, 4, 3), np.float32)
    out = np.zeros((12, 4), np.float32)
    emit = lambda off, rows, n=3: tl.q3t_enc_stream_emit_case(hiplib.fptr(y), 3, 4, 0, n, hiplib.iptr(np.asarray(off, np.int32)), rows, hiplib.fptr(out))
    assert emit([4, 0, 9], 12) == 0
    assert emit([4, 0, 9], 11) == -2 and emit([4, 2, 9], 12) == -2 and emit([4, -1, 9], 12) == -2 and emit([4, 0, 9], 12, 0) == -2
