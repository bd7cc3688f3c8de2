"""Every instantiation of the vocoder's conv kernels (conv_kernel, conv_out1_kernel, resunit_kernel, snake_split_kernel,
conv_split_kernel: csrc/q3_voc_kernels.hip) against plain references of the same operation, one op at a time.

The tables, references and error bounds are tests/voc_conv_ref.py (pinned on the CPU by tests/test_voc_conv_reference.py).
Every launch goes through voc_load / voc_run (enc_load / enc_debug_run for the ELU forms), so pitches, zeroed pads, weight
packing and LDS sizes are the product's own; voc_debug_last_variant() names the instantiation a launch took and the tests
assert it, voc_set_fill() moves the tile-height rule's workgroup target so that the tall tiles are reached at test sizes.

  A  integer data: every product and sum is exact in f32 and in the split form -> equal to the int64 reference bit for bit
  B  real data (as make_synthetic_voc draws it): |y - float64| <= the derived bound, element by element
  C  on every A and B case, bit for bit: chunk b alone = chunk b inside B = 3; voc_set_max_workgroups(3) = uncapped;
     voc_set_fill(0) = the default where the tile height changes
  D  the kernels' own Snake / GELU / ELU against float64 on a dense grid (the three measured constants of voc_conv_ref.py)
  E  an input above 65 504 on the split path: voc_decode returns the exact path's bits
  F  the ELU instantiations through the smallest encoder table the loader takes
and a last test: the union of the instantiations reached equals voc_conv_ref.REACHABLE."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from tests import voc_conv_ref as R
from tests.enc_ref import enc_reference
from tests.voc_gpu_common import grade as _grade, hooks as _hooks, reset as _reset, run as _run, variant as _variant

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHED = {}     # instantiation -> a case that reached it
ORDERS = set()   # split tile orders seen ("myfast" / "plain")
WORST = {}       # (family, arithmetic) -> (error / bound, case)
PAIRS = [(n, d) for n, c in R.CASES.items() for d in c["data"]]


@pytest.fixture(scope="module")
def lib(gpu_lib):
    yield _hooks(gpu_lib)
    _reset(gpu_lib)


def _knobs(lib, c, arith):
    lib.voc_set_exact_fp32(1 if arith == "exact" else 0)
    lib.voc_set_fused_units(c["fused"])
    lib.voc_set_narrow_k1(c["narrow"])
    lib.voc_set_fill(-1 if c["fill"] is None else c["fill"])
    lib.voc_set_max_workgroups(0)


def _note(variant, case):
    for part in variant.split("+"):
        base, _, order = part.partition("/")
        REACHED.setdefault(base, case)
        if base.startswith("split<"):
            ORDERS.add(order or "plain")


def _worst(variant, arith, ratio, case):
    fam = variant.split("+")[-1].split("<")[0]
    if ratio > WORST.get((fam, arith), (-1.0, ""))[0]:
        WORST[(fam, arith)] = (ratio, case)


def _check_table(lib, path, c, t, n_ops, codes, data, name, arithmetics=("exact", "split"), want_override=None):
    T = c["T"]
    if data == "int":
        ref_i, peak = R.reference_int(t, codes, n_ops)
        assert peak < 2 ** 24
    for arith in arithmetics:
        _knobs(lib, c, arith)
        if data == "real":
            ref, bound = R.reference_f64(t, codes, n_ops, arith)
        h = lib.voc_load(path.encode(), T, 3)
        assert h
        try:
            shape = ref_i.shape if data == "int" else ref.shape
            y = _run(lib, h, codes, n_ops, shape)
            variant = _variant(lib)
            _note(variant, name)
            want = want_override or c[arith]
            if want:
                assert variant == want, f"{name} ({arith}) ran {variant}, meant for {want}"
            if data == "int":      # A: bit for bit
                bad = np.argwhere(y != ref_i.astype(np.float32))
                assert bad.size == 0, f"{name} {arith} {variant}: {len(bad)} of {y.size} differ, first at [b, row, col] = {bad[0]}: " \
                                      f"{y[tuple(bad[0])]} != {ref_i[tuple(bad[0])]}"
            else:                  # B: the derived bound
                ratio = _grade(y, ref, bound)
                print(f"{name} {arith} {variant}: max err {np.abs(y - ref).max():.3e}, worst err / bound {ratio:.3f}")
                _worst(variant, arith, ratio, name)
                assert ratio <= 1.0, f"{name} {arith} {variant}: error {ratio:.2f} x the bound"
            # C: invariances, bit for bit
            for b in range(3):
                alone = _run(lib, h, codes[b:b + 1], n_ops, shape)
                assert np.array_equal(alone[0], y[b]), f"{name} {arith} {variant}: chunk {b} alone differs from chunk {b} of 3"
            lib.voc_set_max_workgroups(3)
            capped = _run(lib, h, codes, n_ops, shape)
            lib.voc_set_max_workgroups(0)
            assert np.array_equal(capped, y), f"{name} {arith} {variant}: 3 persistent workgroups differ from one per tile"
            if c["fill_changes"] and want:
                lib.voc_set_fill(0)
                tall = _run(lib, h, codes, n_ops, shape)
                v2 = _variant(lib)
                _note(v2, name)
                assert v2 != variant, f"{name}: voc_set_fill(0) kept {variant}"
                assert np.array_equal(tall, y), f"{name} {arith}: {v2} (fill 0) differs from {variant}"
        finally:
            lib.voc_free(h)


@pytest.mark.parametrize("name,data", PAIRS)
def test_conv_variant(lib, tmp_path, name, data):
    """families A (data = int), B (real) and C of one case table, in both arithmetics"""
    c = R.CASES[name]
    t, n_ops, codes = R.build_table(c["ops"], c["T"], c["cin"], data, c["seed"])
    path = str(tmp_path / "case.q3w")
    W.write_pack(path, {"voc_chunk": float(c["T"])}, t)
    if data == "real" and name.startswith("x_out1_T") and c["T"] >= 7:
        ref = R.reference_f64(t, codes, n_ops)
        assert (ref == 1.0).any() and (ref == -1.0).any() and (np.abs(ref) < 1.0).any()     # the clamp hit on both sides
    try:
        _check_table(lib, path, c, t, n_ops, codes, data, name)
    finally:
        _reset(lib)


OUT1_CASES = [n for n in R.CASES if n.startswith("x_out1_")]


def _child_out1():
    """(child process, Q3_VOC_OUT1=0) the one-row 7-tap convs through the general path: families A, B, C again"""
    import tempfile
    lib = _hooks(hiplib.load())
    assert os.environ.get("Q3_VOC_OUT1") == "0"
    with tempfile.TemporaryDirectory() as tmp:
        for name in OUT1_CASES:
            c = R.CASES[name]
            for data in c["data"]:
                t, n_ops, codes = R.build_table(c["ops"], c["T"], c["cin"], data, c["seed"])
                path = os.path.join(tmp, "case.q3w")
                W.write_pack(path, {"voc_chunk": float(c["T"])}, t)
                _check_table(lib, path, c, t, n_ops, codes, data, name, arithmetics=("exact",), want_override="conv<1,7,8,ct0,act3>")
    print("CHILD " + json.dumps({"reached": sorted(REACHED), "worst": {f"{k[0]}/{k[1]}": v[0] for k, v in WORST.items()}}))


def test_out1_shapes_through_the_general_path():
    """Q3_VOC_OUT1 is read once per process: a fresh child runs conv_out1's cases on conv_kernel<1,7,8> instead"""
    env = dict(os.environ, Q3_VOC_OUT1="0")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_voc_conv import _child_out1; _child_out1()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][-1]
    got = json.loads(line[6:])
    assert got["reached"] == ["conv<1,7,8,ct0,act3>"]
    print("general path, worst err / bound:", got["worst"])


# ----------------------------------------------------------------------------------------------------------------------
# D: the kernels' own activations
# ----------------------------------------------------------------------------------------------------------------------
def _grid(lim, n):
    """n values: a dense linear grid over [-lim, lim], a geometric one towards zero, zero, subnormals, +-8, +-lim"""
    rng = np.random.default_rng(11)
    spec = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1.17549435e-38, -1.17549435e-38, 6e-8, -6e-8, 6.1e-5, -6.1e-5,
                     8.0, -8.0, lim, -lim, np.pi, -np.pi, 2 * np.pi, 3 * np.pi, 4 * np.pi, 5 * np.pi, np.pi / 2, -np.pi / 2])
    geo = lim * 2.0 ** -rng.uniform(0, 40, size=n // 8) * rng.choice([-1.0, 1.0], size=n // 8)
    lin = np.linspace(-lim, lim, n - len(spec) - len(geo))
    g = np.concatenate([spec, geo, lin]).astype(np.float32)
    assert g.size == n
    return g


def _probe_table(T, flags, alpha=0.0, beta=0.0):
    g = None
    prog = [[W.VOP_EMBMEAN, 1, T, 16, 0, 0, 0, 0], [W.VOP_CONV, 16, 16, 1, 1, flags, 0, 0], [W.VOP_CONV, 16, 1, 1, 1, 0, 0, 0]]
    t = {"voc.program": np.asarray(prog, np.int32), "voc.op1.weight": np.eye(16, dtype=np.float32)[:, :, None],
         "voc.op2.weight": np.ones((1, 16, 1), np.float32)}
    if flags & W.VF_SNAKE:
        t["voc.op1.alpha"] = np.full(16, alpha, np.float32)
        t["voc.op1.beta"] = np.full(16, beta, np.float32)
    return t, g


def _probe(lib, tmp_path, x, flags, exact):
    """the device's activation of the values x [T * 16] through a 1-tap identity conv (exact: conv_kernel stages it;
    split: snake_split_kernel applies it and the fp16 MFMA passes hi + lo / 2048 on)"""
    T = x.size // 16
    t, _ = _probe_table(T, flags)
    t["voc.op0.embedding"] = x.reshape(T, 16)
    path = str(tmp_path / f"probe_{flags}_{exact}_{T}.q3w")
    W.write_pack(path, {"voc_chunk": float(T)}, t)
    codes = np.zeros((1, T, 16), np.int64)
    codes[0, :, 0] = np.arange(T)
    lib.voc_set_exact_fp32(exact)
    h = lib.voc_load(path.encode(), T, 1)
    assert h
    try:
        y = _run(lib, h, codes, 2, (1, 16, T))
        _note(_variant(lib), "probe")
    finally:
        lib.voc_free(h)
        lib.voc_set_exact_fp32(0)
    return y[0].T.reshape(-1).astype(np.float64)     # [T][16] -> the order of x


def test_activation_probe_snake_gelu(lib, tmp_path):
    """SIN2_ERR and GELU_ERR of tests/voc_conv_ref.py: measured <= constant; the split path adds its 2^-22 representation"""
    try:
        x = _grid(16.0, 2048 * 16)
        x64 = x.astype(np.float64)
        ref = x64 + np.sin(x64) ** 2            # alpha = beta = 0: a = expf(0) = 1, inv_beta = 1 / (1 + 1e-9f) = 1 in f32
        m_exact = float(np.abs(_probe(lib, tmp_path, x, W.VF_SNAKE, 1) - ref).max())
        m_split = float(np.abs(_probe(lib, tmp_path, x, W.VF_SNAKE, 0) - ref).max())
        xg = _grid(8.0, 2048 * 16)
        refg = R.gelu64(xg.astype(np.float64))
        g_exact = float(np.abs(_probe(lib, tmp_path, xg, W.VF_GELU, 1) - refg).max())
        g_split = float(np.abs(_probe(lib, tmp_path, xg, W.VF_GELU, 0) - refg).max())
        print(f"PROBE sin2 (t + sin^2 t, |t| <= 16): exact {m_exact:.3e} split {m_split:.3e}  constant {R.SIN2_ERR:.3e}")
        print(f"PROBE gelu (|x| <= 8): exact {g_exact:.3e} split {g_split:.3e}  constant {R.GELU_ERR:.3e}")
        # not asserted: the fast sine far outside the decoder's range (Snake arguments of the published decoder stay below ~30).
        # a = 1, so s2 = fl(x + sin^2 x) - x is known to half an ulp of x (6e-5 at 2000)
        for lo, hi in ((16, 64), (64, 256), (256, 1000), (1000, 2000)):
            xs = np.random.default_rng(hi).uniform(lo, hi, size=256 * 16).astype(np.float32) * np.random.default_rng(lo).choice([-1.0, 1.0], size=256 * 16).astype(np.float32)
            s2 = _probe(lib, tmp_path, xs, W.VF_SNAKE, 1) - xs.astype(np.float64)
            print(f"PROBE sin^2 error for {lo} <= |arg| <= {hi}: {np.abs(s2 - np.sin(xs.astype(np.float64)) ** 2).max():.3e} "
                  f"(resolution {np.spacing(np.float32(hi)) / 2:.1e})")
        assert m_exact <= R.SIN2_ERR and g_exact <= R.GELU_ERR
        assert m_split <= R.SIN2_ERR + 2.0 ** -22 * 17 + 2.0 ** -36
        assert g_split <= R.GELU_ERR + 2.0 ** -22 * 8 + 2.0 ** -36
    finally:
        _reset(lib)


def _enc_run(lib, h, pcm, n_ops, shape):
    pcm = np.ascontiguousarray(pcm, np.float32)
    B, n = pcm.shape
    ns = np.full(B, n, np.int32)
    out = np.full((B,) + tuple(shape[1:]), np.nan, np.float32)
    C, L = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert lib.enc_debug_run(h, hiplib.fptr(pcm.reshape(-1)), hiplib.iptr(ns), B, n_ops, hiplib.fptr(out), hiplib.iptr(C), hiplib.iptr(L)) == 0
    assert (int(C[0]), int(L[0])) == tuple(shape[1:])
    return out


def test_activation_probe_elu(lib, tmp_path):
    """ELU_ERR: the staged ELU of conv_kernel<.., act4> through CONV_IN k = 1 (x = +-2^-j pcm, exact) and an identity conv"""
    n = 4096
    prog = [[W.EOP_CONV_IN, 1, 16, 1, 0, 0, 0, 0], [W.EOP_CONV, 16, 16, 1, 1, W.EF_ELU, 0, 0], [W.EOP_RVQ, 16, 1, 1, 8, 0, 1, 0]]
    w0 = np.array([(-1.0) ** c * 2.0 ** -(c // 2) for c in range(16)], np.float32)
    t = {"enc.program": np.asarray(prog, np.int32), "enc.op0.weight": w0.reshape(16, 1, 1),
         "enc.op1.weight": np.eye(16, dtype=np.float32)[:, :, None], "enc.op2.codebook": np.zeros((1, 1, 8), np.float32)}
    path = str(tmp_path / "probe_elu.q3w")
    W.write_pack(path, {"enc_sample_rate": 24000.0}, t)
    pcm = _grid(8.0, n)[None, :]
    x = w0.astype(np.float64)[:, None] * pcm[0].astype(np.float64)[None, :]
    h = lib.enc_load(path.encode(), 1, n)
    assert h
    try:
        y = _enc_run(lib, h, pcm, 2, (1, 16, n))[0]
        _note(_variant(lib), "probe_elu")
    finally:
        lib.enc_free(h)
    m = float(np.abs(y - R.elu64(x)).max())
    print(f"PROBE elu (|x| <= 8): {m:.3e}  constant {R.ELU_ERR:.3e}")
    assert m <= R.ELU_ERR


# ----------------------------------------------------------------------------------------------------------------------
# E: the split path's overflow redo
# ----------------------------------------------------------------------------------------------------------------------
def test_split_overflow_decodes_on_the_exact_path(lib, tmp_path):
    """One input above 65 504 cannot be carried as two fp16 terms: snake_split raises the flag and voc_decode repeats the call
    on the exact path -- the same bits as a decode with voc_set_exact_fp32(1); without the redo the split result differs."""
    T = 131
    t, n_ops, codes = R.build_table([R.conv(64, 3, 1, R.SNAKE)], T, 16, "real", 41, big=70000.0)
    path = str(tmp_path / "ovf.q3w")
    W.write_pack(path, {"voc_chunk": float(T)}, t)
    out = {}
    try:
        for exact in (1, 0):
            lib.voc_set_exact_fp32(exact)
            h = lib.voc_load(path.encode(), T, 3)
            assert h and lib.voc_chunk_samples(h) == T
            try:
                y = np.empty((3, T), np.float32)
                assert lib.voc_decode(h, codes.ctypes.data_as(hiplib.i64p), 3, hiplib.fptr(y)) == 0
                out[exact] = y
                if not exact:
                    raw = _run(lib, h, codes, -1, (3, 1, T))[:, 0]     # the split walk itself, no flag read
            finally:
                lib.voc_free(h)
        assert np.all(np.isfinite(out[1])) and np.abs(out[1]).max() > 1000.0
        assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
        assert not np.array_equal(raw.view(np.uint32), out[1].view(np.uint32))
    finally:
        _reset(lib)


# ----------------------------------------------------------------------------------------------------------------------
# F: the ELU instantiations (reachable only from an encoder table)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["int", "real"])
@pytest.mark.parametrize("name", list(R.ENC_CASES))
def test_elu_variant(lib, tmp_path, name, data):
    c = R.ENC_CASES[name]
    t = R.build_enc_table(c["C"], c["M"], c["k"], c["dil"], data, c["seed"])
    pcm = R.enc_pcm(c["n"], data, c["seed"])
    path = str(tmp_path / "enc_case.q3w")
    W.write_pack(path, {"enc_sample_rate": 24000.0}, t)
    ref, bound = R.enc_reference_f64(t, pcm, bound=True)
    for b in range(3):      # the reference the issue names: tests/enc_ref.py in float64
        want, _ = enc_reference(t, pcm[b], n_ops=2, dtype=torch.float64)
        assert np.abs(ref[b] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
    try:
        lib.voc_set_fill(0)
        h = lib.enc_load(path.encode(), 3, c["n"])
        assert h
        try:
            y = _enc_run(lib, h, pcm, 2, ref.shape)
            variant = _variant(lib)
            _note(variant, name)
            assert variant == c["variant"], f"{name} ran {variant}, meant for {c['variant']}"
            if data == "int":
                assert np.array_equal(ref, np.round(ref))
                assert np.array_equal(y, ref.astype(np.float32))
            else:
                ratio = _grade(y, ref, bound)
                print(f"{name} {variant}: max err {np.abs(y - ref).max():.3e}, worst err / bound {ratio:.3f}")
                _worst("elu<", "exact", ratio, name)
                assert ratio <= 1.0
            for b in range(3):
                assert np.array_equal(_enc_run(lib, h, pcm[b:b + 1], 2, ref.shape)[0], y[b])
            lib.voc_set_max_workgroups(3)
            assert np.array_equal(_enc_run(lib, h, pcm, 2, ref.shape), y)
            lib.voc_set_max_workgroups(0)
            lib.voc_set_fill(-1)
            assert np.array_equal(_enc_run(lib, h, pcm, 2, ref.shape), y)     # the default target's 32-row tiles
        finally:
            lib.enc_free(h)
    finally:
        _reset(lib)


def test_every_reachable_variant_was_reached(lib):
    """The union of the instantiations the tests above reached is the list derived from the launchers (and both tile orders
    of the split kernel were walked).  Run the whole file: this test reads what the others recorded."""
    print("worst error / bound per family:", {f"{k[0]}/{k[1]}": (round(v[0], 3), v[1]) for k, v in sorted(WORST.items())})
    missing, extra = R.REACHABLE - set(REACHED), set(REACHED) - R.REACHABLE
    assert not missing and not extra, f"not reached: {sorted(missing)}; reached but not listed: {sorted(extra)}"
    assert ORDERS == {"myfast", "plain"}
