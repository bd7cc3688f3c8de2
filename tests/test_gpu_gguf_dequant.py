"""launch_dequant (csrc/q3_dequant.hip) through the hook q3t_dequant_case, bit for bit against ggml's formulas evaluated
in float64 (tests/gguf_ref.py dequant64): the f32 output is that value rounded once to float32, the fp16 output its
round-to-nearest-even with saturation at +-65504.  No tolerance: every product of the formulas is exact in fp32 and the
K-quants' subtraction is the one rounding.

Shapes, per block type: K in {one block, two blocks, 1024, 3072} (a superblock boundary, the model's two widths) x rows in
{1, 16, 48} (below, at and past the 16-row tile the packed weights are made of), a row sub-range that starts at a non-zero
row (what the loader does with the padded tables never starts there, but the kernel takes a pointer into the middle of a
tensor for it), and one case made of every edge block (all zero, all 0xFF, every 6-bit scale / minimum value at every
position j < 4 and j >= 4).  Blocks: every byte random, d / dmin any finite fp16 (+-0, subnormals, negatives, 65504).
The hook puts a guard behind the output and fails the case when it was written."""
import ctypes

import numpy as np
import pytest

from tests import gguf_ref as R

pytestmark = pytest.mark.gpu

u8p = ctypes.POINTER(ctypes.c_uint8)
u16p = ctypes.POINTER(ctypes.c_uint16)
f32p = ctypes.POINTER(ctypes.c_float)


def run_case(lib, tname, blocks, rows_total, K, row0, rows, f16):
    blocks = np.ascontiguousarray(blocks, np.uint8)
    out = np.zeros((rows, K), np.uint16 if f16 else np.float32)
    flag = ctypes.c_int(-1)
    rc = lib.q3t_dequant_case(R.TYPES[tname][1], blocks.ctypes.data_as(u8p), blocks.nbytes, rows_total, K, row0, rows,
                              out.ctypes.data_as(u16p) if f16 else None, None if f16 else out.ctypes.data_as(f32p),
                              ctypes.byref(flag))
    assert rc == 0, rc
    return out, flag.value


def check(lib, tname, blocks, rows_total, K, row0, rows):
    want32 = R.dequant64(tname, blocks, K)[row0:row0 + rows].astype(np.float32)
    got32, flag = run_case(lib, tname, blocks, rows_total, K, row0, rows, f16=False)
    assert flag == 0
    np.testing.assert_array_equal(got32.view(np.uint32), want32.view(np.uint32))
    got16, flag = run_case(lib, tname, blocks, rows_total, K, row0, rows, f16=True)
    assert flag == 0
    np.testing.assert_array_equal(got16, R.f16_sat(want32).view(np.uint16))
    return want32


@pytest.mark.parametrize("tname", R.BLOCK_TYPES)
def test_dequant_is_the_float64_formula_rounded_once(test_lib, tname):
    bs = R.TYPES[tname][2]
    seen_sat = False
    for ki, K in enumerate((bs, 2 * bs, 1024, 3072)):
        for ri, rows in enumerate((1, 16, 48)):
            blocks = R.case_blocks(tname, rows * K // bs, seed=10 * ki + ri)
            w = check(test_lib, tname, blocks, rows, K, 0, rows)
            seen_sat |= bool((np.abs(w) > 65504).any())
    assert seen_sat                    # the fp16 saturation was exercised


@pytest.mark.parametrize("tname", R.BLOCK_TYPES)
def test_dequant_row_sub_range(test_lib, tname):
    bs = R.TYPES[tname][2]
    for K, total, row0, rows in ((bs, 5, 3, 2), (1024, 48, 16, 32), (3072, 19, 7, 11)):
        blocks = R.case_blocks(tname, total * K // bs, seed=77 + row0)
        check(test_lib, tname, blocks, total, K, row0, rows)


@pytest.mark.parametrize("tname", R.BLOCK_TYPES)
def test_dequant_every_edge_block(test_lib, tname):
    e = R.edge_blocks(tname)
    check(test_lib, tname, e, len(e), R.TYPES[tname][2], 0, len(e))


@pytest.mark.parametrize("tname", R.BLOCK_TYPES)
def test_non_finite_scale_raises_the_flag(test_lib, tname):
    bs = R.TYPES[tname][2]
    rng = np.random.default_rng(5)
    n_scales = len(R._D_OFFSETS[tname])
    for which, bits in ((0, 0x7c00), (n_scales - 1, 0x7e01), (0, 0xfc00), (n_scales - 1, 0xffff)):   # d = +-Inf, dmin (or d) = NaN
        blocks = R.random_blocks(tname, 3 * 2, rng)
        _, flag = run_case(test_lib, tname, blocks, 3, 2 * bs, 0, 3, f16=True)
        assert flag == 0
        one = blocks[4:5].copy()
        R.put_halves(one, tname, which, np.array([bits], np.uint16))
        blocks[4] = one[0]
        for f16 in (True, False):
            _, flag = run_case(test_lib, tname, blocks, 3, 2 * bs, 0, 3, f16=f16)
            assert flag == 1
        # a row range that does not hold the block leaves the flag alone
        _, flag = run_case(test_lib, tname, blocks, 3, 2 * bs, 0, 2, f16=True)
        assert flag == 0
