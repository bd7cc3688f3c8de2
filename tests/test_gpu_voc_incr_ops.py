"""The carry-state kernels of the incremental decode (voc_incr_prepend_kernel, voc_incr_prepend_split_kernel, voc_attn_incr_kernel:
csrc/q3_voc_kernels.hip), one op at a time.

voc_debug_incr_push (csrc/q3_voc_stream.hip) is a push whose walk ends after the first n_ops ops and which returns the new columns
of that activation; the histories of the ops that ran move on as in a real push.  Three streams of one handle, at different phases,
are driven through it with the push patterns of tests/voc_ops_ref.py; each stream's columns, joined over its pushes, are compared
with the references of tests/voc_ops_ref.py evaluated ONCE over the whole stream (every op is causal, so that evaluation is the
incremental one): integer tables bit for bit, real tables under the per-op bounds, attention to the project's 2e-4 of scale.
D: the bits of every column are the same whatever the push pattern and whichever stream slot carries it."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from tests import voc_ops_ref as R
from tests.voc_gpu_common import grade as _grade, hooks as _hooks, reset as _reset

pytestmark = pytest.mark.gpu

CHUNK = 64       # frames a push may carry


@pytest.fixture(scope="module")
def lib(gpu_lib):
    lib = _hooks(gpu_lib)
    lib.voc_debug_incr_push.restype = ctypes.c_int
    lib.voc_debug_incr_push.argtypes = [ctypes.c_void_p, ctypes.c_int, hiplib.i32p, hiplib.i64p, hiplib.i32p, ctypes.c_int, hiplib.f32p,
                                        ctypes.c_int64, hiplib.i64p, hiplib.i32p]
    _reset(lib)
    yield lib
    _reset(lib)


def _drive(lib, s, codes, n_ops, pattern, slots, C):
    """codes [S][N][16]: stream b's frames, carried by slot slots[b] and pushed as push_plan(N, pattern, b) says -- round r of the
    drive is one push holding the r-th piece of every stream that still has one -> [S][C][N]"""
    S, N = codes.shape[0], codes.shape[1]
    for k in set(slots):
        assert lib.voc_incr_reset(s, k) == 0
    plans = [R.push_plan(N, pattern, b) for b in range(S)]
    done = [0] * S
    cols = [[] for _ in range(S)]
    for r in range(max(len(p) for p in plans)):
        live = [b for b in range(S) if r < len(plans[b])]
        streams = np.array([slots[b] for b in live], np.int32)
        n_new = np.array([plans[b][r] for b in live], np.int32)
        frames = np.ascontiguousarray(np.concatenate([codes[b, done[b]:done[b] + plans[b][r]] for b in live]), np.int64)
        out = np.full(int(n_new.sum()) * C, np.nan, np.float32)
        off = np.zeros(len(live) + 1, np.int64)
        Cd = np.zeros(1, np.int32)
        rc = lib.voc_debug_incr_push(s, len(live), hiplib.iptr(streams), frames.ctypes.data_as(hiplib.i64p), hiplib.iptr(n_new), n_ops,
                                     hiplib.fptr(out), out.size, off.ctypes.data_as(hiplib.i64p), hiplib.iptr(Cd))
        assert rc == 0 and int(Cd[0]) == C and int(off[-1]) == out.size
        for e, b in enumerate(live):
            cols[b].append(out[off[e]:off[e + 1]].reshape(C, plans[b][r]))
            done[b] += plans[b][r]
    assert all(d == N for d in done)
    return np.stack([np.concatenate(c, axis=1) for c in cols])


@pytest.mark.parametrize("name", list(R.INCR_CASES))
def test_incremental_op(lib, test_lib, tmp_path, name):
    c = R.INCR_CASES[name]
    t, n_ops, codes = R.make_incr(name)
    is_attn = c["ops"][0]["op"] == W.VOP_ATTN
    if c["N"] > 1000:
        codes = codes[:1]            # one long stream
    S, N = codes.shape[0], c["N"]
    path = str(tmp_path / "case.q3w")
    W.write_pack(path, {"voc_chunk": float(CHUNK)}, t)
    if c["data"] == "int":
        ref_i, peak = R.reference_int(t, codes, n_ops)
        assert peak < 2 ** 24
    h = lib.voc_load(path.encode(), CHUNK, 3)
    assert h
    try:
        for arith in c["arith"]:
            if c["data"] == "real":
                ref, bound = R.reference_f64(t, codes, n_ops, "split" if arith else "exact")
            Cout = (ref_i if c["data"] == "int" else ref).shape[1]
            s = lib.voc_incr_create(h, 3)
            assert s
            try:
                assert lib.voc_incr_set_arithmetic(s, arith) == arith       # 1: split convs, and every history moves by parity
                first = None
                for pattern in c["patterns"]:
                    tag = f"{name} arithmetic {arith} pushes {pattern}"
                    y = _drive(lib, s, codes, n_ops, pattern, list(range(S)), Cout)
                    assert np.all(np.isfinite(y)), tag
                    if is_attn:
                        scale = float(np.abs(ref).max())
                        err = np.abs(y - ref).max(axis=(0, 1)) / scale           # per column
                        print(f"{tag}: max err {err.max():.3e} of scale {scale:.3f}" +
                              (f"; columns >= 2000: {err[2000:].max():.3e}" if N > 2000 else ""))
                        assert err.max() <= R.ATTN_TOL, tag
                    elif c["data"] == "int":
                        bad = np.argwhere(y != ref_i.astype(np.float32))
                        assert bad.size == 0, f"{tag}: {len(bad)} of {y.size} differ, first at [stream, row, col] = {bad[0]}: " \
                                              f"{y[tuple(bad[0])]} != {ref_i[tuple(bad[0])]}"
                    else:
                        ratio = _grade(y, ref, bound)
                        print(f"{tag}: max err {np.abs(y - ref).max():.3e}, worst err / bound {ratio:.3f}")
                        assert ratio <= 1.0, f"{tag}: error {ratio:.2f} x the bound"
                    # D: the same bits whatever the push pattern ...
                    if first is None:
                        first = y
                    assert np.array_equal(y.view(np.uint32), first.view(np.uint32)), f"{tag}: differs from pushes {c['patterns'][0]}"
                # ... and whichever slot carries the stream
                if S == 3:
                    moved = _drive(lib, s, codes, n_ops, c["patterns"][-1], [1, 2, 0], Cout)
                    assert np.array_equal(moved.view(np.uint32), first.view(np.uint32)), f"{name} arithmetic {arith}: streams moved to other slots"
            finally:
                lib.voc_incr_free(s)
        if is_attn:
            # below `window` columns the incremental kernel performs voc_attn_kernel's operations in the same order (the window's
            # first key is column 0, the angles are the absolute columns): the same bits as the full-chunk wave kernel
            o = c["ops"][0]
            L = min(o["window"], N)
            tab = np.asarray(t["voc.op0.embedding"], np.float32)
            x = np.ascontiguousarray(tab[codes[:, :L, 0]].transpose(0, 2, 1))                      # [S][3 H D][L]
            full = np.zeros((S, Cout, L), np.float32)
            assert test_lib.q3t_voc_attn(0, hiplib.fptr(x), hiplib.fptr(full), S, o["H"], o["D"], L, o["window"], float(o["theta"])) == 0
            assert np.array_equal(full.view(np.uint32), first[:, :, :L].view(np.uint32)), f"{name}: the first {L} columns differ from voc_attn_kernel's"
    finally:
        lib.voc_free(h)
