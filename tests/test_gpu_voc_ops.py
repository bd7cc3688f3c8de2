"""The vocoder's non-conv kernels (chan_norm_kernel, dwconv_kernel, glu_kernel, rvq_kernel, embmean_kernel, and voc_attn_kernel /
voc_attn_tile_kernel behind voc_run's VOP_ATTN dispatch: csrc/q3_voc_kernels.hip) against plain references of the same operation,
one op at a time, through voc_load / voc_debug_run.

The tables, references and error bounds are tests/voc_ops_ref.py (pinned on the CPU by tests/test_voc_ops_reference.py); the
families are those of tests/test_gpu_voc_conv.py:

  A  integer data (dwconv, rvq, embmean nq = 1, 2, 16): every product and sum is exact in f32 -> the int64 reference bit for bit
  B  real data: |y - float64| <= the derived bound, element by element (attention: the project's grade, 2e-4 of the output's scale)
  C  on every case, bit for bit: chunk b alone = chunk b inside B = 3; voc_set_max_workgroups(3) = uncapped
  D  the device's SiLU against float64 on a dense grid: the measured constant SILU_ERR
and one ConvNeXt block as a chain, in both arithmetics of its convs."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import weights as W
from tests import voc_ops_ref as R
from tests.voc_gpu_common import grade as _grade, hooks as _hooks, reset as _reset, run as _run, variant as _variant

pytestmark = pytest.mark.gpu

PAIRS = [(n, d) for n, c in R.CASES.items() for d in c["data"]]
WORST = {}       # family (/ arithmetic) -> (error / bound -- attention: error / scale --, case)


@pytest.fixture(scope="module")
def lib(gpu_lib):
    _reset(_hooks(gpu_lib))
    yield gpu_lib
    _reset(gpu_lib)
    print("worst error / bound per kernel (attention: error / scale):", {k: (float(f"{v[0]:.3g}"), v[1]) for k, v in sorted(WORST.items())})


def _note(key, ratio, case):
    if ratio > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (ratio, case)


def _columns_of_row(codes, row):
    """where the front put row `row` of the input table: (b, t) with codes[b][t][0] == row"""
    return [(b, int(np.flatnonzero(codes[b, :, 0] == row)[0])) for b in range(codes.shape[0])]


@pytest.mark.parametrize("name,data", PAIRS)
def test_op(lib, tmp_path, name, data):
    """families A (data = int), B (real) and C of one case table"""
    c = R.CASES[name]
    fam, T = c["family"], c["T"]
    t, n_ops, codes = R.make(name, data)
    path = str(tmp_path / "case.q3w")
    W.write_pack(path, {"voc_chunk": float(T)}, t)
    if data == "int":
        ref_i, peak = R.reference_int(t, codes, n_ops)
        assert peak < 2 ** 24
    try:
        for arith in (("exact", "split") if fam == "convnext" else ("exact",)):
            _reset(lib)
            lib.voc_set_exact_fp32(1 if arith == "exact" else 0)
            if data == "real":
                ref, bound = R.reference_f64(t, codes, n_ops, arith)
            h = lib.voc_load(path.encode(), T, 3)
            assert h, f"{name}: voc_load refused the table"
            try:
                shape = ref_i.shape if data == "int" else ref.shape
                y = _run(lib, h, codes, n_ops, shape)
                assert np.all(np.isfinite(y))
                if fam == "attn":
                    variant = _variant(lib)
                    assert variant in ("attn", "attn_tile")
                    if c["variant"]:
                        assert variant == c["variant"], f"{name} ran {variant}, meant for {c['variant']}"
                    scale = float(np.abs(ref).max())
                    err = float(np.abs(y - ref).max()) / scale
                    print(f"{name} {variant}: max err {err:.3e} of scale {scale:.3f}")
                    _note(variant, err, name)
                    assert err <= R.ATTN_TOL, f"{name} {variant}: max err {err:.2e} of scale {scale:.3f}"
                elif data == "int":      # A: bit for bit
                    bad = np.argwhere(y != ref_i.astype(np.float32))
                    assert bad.size == 0, f"{name}: {len(bad)} of {y.size} differ, first at [b, row, col] = {bad[0]}: " \
                                          f"{y[tuple(bad[0])]} != {ref_i[tuple(bad[0])]}"
                else:                    # B: the derived bound
                    if fam == "convnext":    # the closing conv (32 input channels) runs in the arithmetic asked for
                        assert _variant(lib).startswith("conv<" if arith == "exact" else "snake_split+split<"), _variant(lib)
                    ratio = _grade(y, ref, bound)
                    print(f"{name} {arith}: max err {np.abs(y - ref).max():.3e}, worst err / bound {ratio:.3f}")
                    _note(fam if fam != "convnext" else f"convnext/{arith}", ratio, name)
                    assert ratio <= 1.0, f"{name} {arith}: error {ratio:.2f} x the bound"
                if fam == "norm" and "const" in c["special"] and c["ops"][0]["kind"] == 1:
                    # a column of one integer: the mean is that integer, every d is +0 and LayerNorm returns its bias, bit for bit
                    bias = np.asarray(t["voc.op1.bias"], np.float32)
                    for b, col in _columns_of_row(codes, c["special"].index("const")):
                        assert np.array_equal(y[b, :, col].view(np.uint32), bias.view(np.uint32)), f"{name}: chunk {b} column {col}"
                # C: invariances, bit for bit
                for b in range(3):
                    alone = _run(lib, h, codes[b:b + 1], n_ops, shape)
                    assert np.array_equal(alone[0].view(np.uint32), y[b].view(np.uint32)), f"{name} {arith}: chunk {b} alone differs from chunk {b} of 3"
                lib.voc_set_max_workgroups(3)
                capped = _run(lib, h, codes, n_ops, shape)
                lib.voc_set_max_workgroups(0)
                assert np.array_equal(capped.view(np.uint32), y.view(np.uint32)), f"{name} {arith}: 3 persistent workgroups differ from uncapped"
            finally:
                lib.voc_free(h)
    finally:
        _reset(lib)


def test_unused_id_slots_do_not_reach_the_result(lib, tmp_path):
    """NQ < 16: whatever the slots NQ .. 15 of a frame hold, the bits of an rvq / embmean output stay (the reference never reads
    them; this is the same statement about the device alone, on the tables' own codes with those slots rewritten)"""
    for name in ("rvq_q2_d8_o8_T5", "rvq_q1_d8_o8", "emb_q3_T5", "emb_q2_T5"):
        c = R.CASES[name]
        t, n_ops, codes = R.make(name, "real")
        path = str(tmp_path / f"{name}.q3w")
        W.write_pack(path, {"voc_chunk": float(c["T"])}, t)
        h = lib.voc_load(path.encode(), c["T"], 3)
        assert h
        try:
            shape = R.reference_f64(t, codes, n_ops).shape
            y = _run(lib, h, codes, n_ops, shape)
            for fill in (0, 2 ** 62, -2 ** 62, c["cb"] - 1):
                other = codes.copy()
                other[:, :, c["nq"]:] = fill
                assert np.array_equal(_run(lib, h, other, n_ops, shape).view(np.uint32), y.view(np.uint32)), f"{name}: fill {fill}"
        finally:
            lib.voc_free(h)


def test_silu_probe(lib, tmp_path):
    """D: SILU_ERR of tests/voc_ops_ref.py.  A GLU (kind 0) whose up half is 1 returns the kernel's own SiLU: measured <= constant."""
    T = 2048
    g = R.grid(16.0, T * 16)
    x = np.ones((T, 32), np.float32)
    x[:, :16] = g.reshape(T, 16)
    t, n_ops = R.build_table([R.glu(0)], x, "real", 3)
    path = str(tmp_path / "probe_silu.q3w")
    W.write_pack(path, {"voc_chunk": float(T)}, t)
    codes = np.zeros((1, T, 16), np.int64)
    codes[0, :, 0] = np.arange(T)
    h = lib.voc_load(path.encode(), T, 1)
    assert h
    try:
        y = _run(lib, h, codes, n_ops, (1, 16, T))[0].T.reshape(-1).astype(np.float64)      # [T][16]: the order of g
    finally:
        lib.voc_free(h)
    m = float(np.abs(y - R.silu64(g)).max())
    print(f"PROBE silu (|x| <= 16): {m:.3e}  constant {R.SILU_ERR:.3e}  recorded {R.SILU_MEASURED:.3e}")
    assert m <= R.SILU_ERR
