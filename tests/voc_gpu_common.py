"""What the vocoder's one-op GPU tests share (tests/test_gpu_voc_conv.py, test_gpu_voc_ops.py, test_gpu_voc_incr_ops.py): the
signatures of the host-only hooks, the knobs' defaults, one debug run and the element-by-element grade."""
import ctypes

import numpy as np

from qwen3_tts_axera_russian_amd import hiplib


def hooks(lib):
    lib.voc_debug_run.restype = ctypes.c_int
    lib.voc_debug_run.argtypes = [ctypes.c_void_p, hiplib.i64p, ctypes.c_int, ctypes.c_int, hiplib.f32p, hiplib.i32p, hiplib.i32p]
    lib.voc_debug_last_variant.restype = ctypes.c_char_p
    lib.voc_debug_last_variant.argtypes = []
    for n in ("voc_set_fill", "voc_set_narrow_k1"):
        getattr(lib, n).restype = ctypes.c_int
        getattr(lib, n).argtypes = [ctypes.c_int]
    return lib


def reset(lib):
    lib.voc_set_exact_fp32(0)
    lib.voc_set_fused_units(1)
    lib.voc_set_narrow_k1(1)
    lib.voc_set_fill(-1)
    lib.voc_set_max_workgroups(0)


def variant(lib):
    return lib.voc_debug_last_variant().decode()


def run(lib, h, codes, n_ops, shape):
    """the activation after n_ops ops for codes [B][T][16] -> [B][C][L] (shape: what the reference says it is)"""
    codes = np.ascontiguousarray(codes, np.int64)
    B = codes.shape[0]
    out = np.full((B,) + tuple(shape[1:]), np.nan, np.float32)
    C, L = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert lib.voc_debug_run(h, codes.ctypes.data_as(hiplib.i64p), B, n_ops, hiplib.fptr(out), hiplib.iptr(C), hiplib.iptr(L)) == 0
    assert (int(C[0]), int(L[0])) == tuple(shape[1:])
    return out


def grade(y, ref, bound):
    """-> the largest error / bound (0 / 0 counts as 0); asserts the bound element by element"""
    err = np.abs(y.astype(np.float64) - ref)
    assert np.all(np.isfinite(y))
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    return ratio
