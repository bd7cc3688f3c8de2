"""tests/voc_ops_ref.py (the float64 / int64 references of tests/test_gpu_voc_ops.py and tests/test_gpu_voc_incr_ops.py) pinned on
the CPU: on every table the float64 walk agrees with oracle/voc_ref.py evaluated in float64 to 1e-12 of the output's scale, both at
the op under test and at the table's end; the int64 and float64 walks agree exactly on the integer tables, which stay below 2^24 in
summed magnitude; every table is one weights.write_pack takes.  (The walk takes a norm's eps as the loader forms it, in f32; the
oracle takes eps_e9 * 1e-9 in double: the comparison runs the walk on the oracle's eps, and a second assertion bounds what the
loader's rounding of eps can change.)"""
import numpy as np
import pytest

from oracle.voc_ref import voc_reference
from qwen3_tts_axera_russian_amd import weights as W
from tests import voc_ops_ref as R

PAIRS = [(n, d) for n, c in R.CASES.items() for d in c["data"]]


def _close(y, want):
    assert y.shape == want.shape
    assert np.abs(y - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)


def _pin(t, n_ops, codes, data, tmp_path, chunk):
    total = len(np.asarray(t["voc.program"]))
    for n in (n_ops, total):
        _close(R.reference_f64(t, codes, n, table_eps=True), voc_reference(t, codes, n, dtype=np.float64))
    y, bound = R.reference_f64(t, codes, n_ops, "split")
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(bound)) and np.all(bound >= 0)
    # the loader's f32 eps is within 2^-24 of the table's: the output moves by half that at most, relative (d y / y = -d eps / 2 v)
    assert np.all(np.abs(y - R.reference_f64(t, codes, n_ops, table_eps=True)) <= 2.0 ** -24 * np.abs(y) + 1e-300)
    if data == "int":
        yi, peak = R.reference_int(t, codes, n_ops)
        assert peak < 2 ** 24
        assert np.array_equal(yi.astype(np.float64), y)
    assert int(np.asarray(t["voc.program"])[-1][2]) == 1          # ends in one channel: a table the loader takes
    W.write_pack(str(tmp_path / "case.q3w"), {"voc_chunk": float(chunk)}, t)


@pytest.mark.parametrize("name,data", PAIRS)
def test_reference_matches_oracle(name, data, tmp_path):
    t, n_ops, codes = R.make(name, data)
    _pin(t, n_ops, codes, data, tmp_path, R.CASES[name]["T"])


@pytest.mark.parametrize("name", list(R.INCR_CASES))
def test_incremental_reference_matches_oracle(name, tmp_path):
    """the whole-stream evaluation the incremental tests compare with (every op is causal: it is the incremental one)"""
    c = R.INCR_CASES[name]
    t, n_ops, codes = R.make_incr(name)
    if c["N"] > 1000:
        codes = codes[:1]          # (the long attention stream: one row pins the reference)
    _pin(t, n_ops, codes, c["data"], tmp_path, 64)


def test_loader_eps_is_the_f32_value():
    for e9 in (1000, 10000, 1, 999999):
        assert R.loader_eps(e9) == float(np.float32(e9 * 1e-9)) and abs(R.loader_eps(e9) - e9 * 1e-9) <= 2.0 ** -24 * e9 * 1e-9


def test_push_plans_cover_the_stream():
    for pat in R.PUSH_PATTERNS:
        plans = [R.push_plan(300, pat, b) for b in range(3)]
        assert all(sum(p) == 300 and min(p) >= 1 and max(p) <= 64 for p in plans)
    assert {1, 6, 7, 64} <= {n for pat in R.PUSH_PATTERNS for n in R.push_plan(300, pat, 0)}      # n < H, n = H, n > H at H = 6


def test_edge_ids_are_planted():
    for name, c in R.CASES.items():
        if c["family"] in ("rvq", "embmean"):
            _, _, codes = R.make(name, c["data"][-1])
            used = codes[:, :, :c["nq"]]
            assert ((used < 0) | (used >= c["cb"])).any(), name
            if c["nq"] < 16:
                assert (np.abs(codes[:, :, c["nq"]:]) >= 2 ** 40).any(), name
