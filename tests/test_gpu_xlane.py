"""The register-file cross-lane exchanges of csrc/q3_xlane.h (xlane_xor: DPP inside a row of 16 lanes, permlane swaps
across rows) against __shfl_xor, and the attention kernels built on them at the shapes where an exchange inside the
per-group branches of the softmax walk could go wrong (groups with no key, one group's worth, the prefetch edge).

  * q3t_xlane_case: one kernel applies a butterfly built on xlane_xor and the same butterfly built on __shfl_xor to the same
    registers; the two outputs must be the same 32-bit words -- sums keep their tree, so nothing weaker is expected -- for
    every (op, width), on 64 x 256 values that mix normals with +-0, +-inf, NaN, denormals and runs of equal values.  The
    max and arg-max results are also held against numpy wherever a group has no NaN (both forms wrong alike would pass the
    first check), the arg-max index with the lowest-index tie rule.
  * q3t_attn against tests/attn_ref.py at the bounds of tests/test_gpu_attention.py (its run()), for the cases that file does
    not have: a whole batch of 1 / 3 / 32 rows at ONE position (the frame loop's lockstep shape; that file mixes positions
    inside a batch) on each side of a 16-lane group filling up (15, 16, 17) and of the prefetch running out (127, 128, 129
    at 256 threads, 255, 256, 257 at 1024), and the short kernel at 1, 3 and 32 rows."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests.test_gpu_attention import run

pytestmark = pytest.mark.gpu

N = 64 * 256
OPS = {"sum": 0, "max": 1, "argmax": 2}


def xlane_input():
    rng = np.random.default_rng(7)
    x = rng.standard_normal(N).astype(np.float32)
    # [0, 4096): plain normals.  [4096, 8192): small integers (ties everywhere, exact sums).
    x[4096:8192] = rng.integers(-3, 4, 4096).astype(np.float32)
    # [8192, N): normals with one value in six replaced by a special one.  Three regions, so that two DIFFERENT NaN words
    # never meet in one sum: NaN with +inf, NaN with -inf, and both infinities (whose sum is the hardware's default NaN)
    # without an input NaN.  Which of two NaN operands' payloads an addition returns depends on the operand order, addition
    # is commutative to the compiler, and the order it picks is not a property of the exchange: with every special value
    # in one pot the two forms differed in the SIGN of such NaNs (0x7fc00000 against 0xffc00000, 672 of 16 384 words of
    # the 64-lane sum) and in nothing else.
    common = [0.0, -0.0, 1e-40, -1e-40, 1.401298464e-45, 1.0, 1.0, -2.5, -2.5]
    for lo, hi, extra in ((8192, 10240, [np.nan, np.inf]), (10240, 12288, [np.nan, -np.inf]),
                          (12288, N, [np.inf, -np.inf])):
        special = np.array(common + extra + extra, np.float32)
        at = lo + np.flatnonzero(rng.random(hi - lo) < 1 / 6)
        x[at] = special[rng.integers(0, len(special), len(at))]
    # whole groups of one value: 64 lanes of +0, of -0, of 1, of -inf, of a denormal
    for i, v in enumerate(np.array([0.0, -0.0, 1.0, -np.inf, 1e-40], np.float32)):
        x[16000 + 64 * i:16000 + 64 * (i + 1)] = v
    return x


X = xlane_input()


@pytest.mark.parametrize("width", [4, 16, 64])
@pytest.mark.parametrize("op", ["sum", "max", "argmax"])
def test_xlane_matches_shfl_bit_for_bit(test_lib, op, width):
    words = N * (2 if op == "argmax" else 1)
    new = np.full(words, 1234.5, np.float32)
    old = np.full(words, -1234.5, np.float32)
    rc = test_lib.q3t_xlane_case(OPS[op], width, N, hiplib.fptr(X), hiplib.fptr(new), hiplib.fptr(old))
    assert rc == 0, rc
    a, b = new.view(np.uint32), old.view(np.uint32)
    bad = np.flatnonzero(a != b)
    assert not len(bad), (f"{op} over {width} lanes: {len(bad)} words differ, first at {bad[0]}: "
                          f"xlane {a[bad[0]]:#010x}, shfl {b[bad[0]]:#010x}")
    # and the common answer is the right one
    g = X.reshape(-1, width)
    clean = ~np.isnan(g).any(1)
    if op == "sum":
        ints = slice(4096 // width, 8192 // width)                  # small integers: any summation order is exact
        np.testing.assert_array_equal(new.reshape(-1, width)[ints], np.repeat(g[ints].sum(1, keepdims=True), width, 1))
    else:
        want = np.repeat(g.max(1, keepdims=True), width, 1)
        assert (new[:N].reshape(-1, width)[clean] == want[clean]).all(), f"{op} over {width} lanes: wrong maximum"
    if op == "argmax":
        idx = new[N:].view(np.int32).reshape(-1, width)
        first = (np.arange(N).reshape(-1, width)[:, :1] + g.argmax(1)[:, None]).repeat(width, 1)   # lowest index of the maximum
        assert (idx[clean] == first[clean]).all(), f"arg-max over {width} lanes: a tie did not go to the lowest index"


def test_xlane_hook_refuses_partial_waves(test_lib):
    """The helpers' contract is whole exchange groups: the hook launches whole waves only and takes no other op or width."""
    buf = np.zeros(256, np.float32)
    p = hiplib.fptr(buf)
    assert test_lib.q3t_xlane_case(0, 16, 100, p, p, p) == -2
    assert test_lib.q3t_xlane_case(0, 8, 128, p, p, p) == -2
    assert test_lib.q3t_xlane_case(3, 16, 128, p, p, p) == -2


def lockstep(test_lib, variant, R, p, threads, seed):
    """R rows of distinct (permuted) slots, all at cached position p: one frame-loop step of a batch."""
    rng = np.random.default_rng(seed)
    n_slots = R + 2
    n_ctx = 32 if p < 30 else (p + 16) // 16 * 16
    return run(test_lib, variant, 0, R, slot=rng.permutation(n_slots)[:R], pos=[p] * R, threads=threads,
               n_slots=n_slots, n_ctx=n_ctx, seed=seed)


@pytest.mark.parametrize("R", [1, 3, 32])
def test_fused_batch_shape_lockstep_positions(test_lib, R):
    """attn_kernel<FUSED, 8> at 256 threads (16 groups x 8 prefetched keys): 0 and 1 cached keys (all groups but at most
    one sit out every exchange), 15 / 16 / 17 (prefetch slot 1 empty, one group's, two groups'), 127 / 128 / 129 (the
    prefetch exactly full; the first key of the in-loop path)."""
    for p in (0, 1, 15, 16, 17, 127, 128, 129):
        if R == 1 and p != 17:
            continue                                   # one row at those positions: tests/test_gpu_attention.py
        lockstep(test_lib, "fused<8> 256 threads, lockstep", R, p, 256, 1000 * R + p)


def test_fused_one_row_shape_three_rows(test_lib):
    """attn_kernel<FUSED, 4> at 1024 threads (64 groups x 4 prefetched keys) around its prefetch edge, 3 rows (one row:
    tests/test_gpu_attention.py; 32 rows never take this shape)."""
    for p in (255, 256, 257):
        lockstep(test_lib, "fused<4> 1024 threads, lockstep", 3, p, 1024, 3000 + p)


@pytest.mark.parametrize("R", [1, 3, 32])
def test_short_kernel_rows(test_lib, R):
    """attn_short_kernel (pos == null, every row at pos_base) with no cached key, one, and all 15."""
    for p in (0, 1, 15):
        rng = np.random.default_rng(50 * R + p)
        run(test_lib, "short, 1 / 3 / 32 rows", 0, R, slot=rng.permutation(R + 2)[:R], pos_base=p, threads=256,
            n_slots=R + 2, n_ctx=32, seed=500 * R + p)
