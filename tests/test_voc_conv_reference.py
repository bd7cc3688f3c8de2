"""tests/voc_conv_ref.py (the float64 / int64 references of tests/test_gpu_voc_conv.py) pinned on the CPU: on every case
table the float64 reference agrees with oracle/voc_ref.py evaluated in float64 (torch's conv1d / conv_transpose1d) to
1e-12 of the output's scale, the int64 and float64 references agree exactly on the integer data, and every integer case
stays below 2^24 in summed magnitude (so that f32 is exact whatever the summation order).  The encoder tables of the ELU
cases are pinned to tests/enc_ref.py the same way."""
import numpy as np
import pytest
import torch

from oracle.voc_ref import voc_reference
from tests import voc_conv_ref as R
from tests.enc_ref import enc_reference

PAIRS = [(n, d) for n, c in R.CASES.items() for d in c["data"]]


@pytest.mark.parametrize("name,data", PAIRS)
def test_reference_matches_oracle(name, data):
    c = R.CASES[name]
    t, n_ops, codes = R.build_table(c["ops"], c["T"], c["cin"], data, c["seed"])
    y, bound = R.reference_f64(t, codes, n_ops, "split")
    want = voc_reference(t, codes, n_ops, dtype=np.float64)
    assert y.shape == want.shape
    assert np.abs(y - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
    assert np.all(np.isfinite(bound)) and np.all(bound >= 0)
    if data == "int":
        yi, peak = R.reference_int(t, codes, n_ops)
        assert peak < 2 ** 24
        assert np.array_equal(yi.astype(np.float64), y)      # bit for bit: every value is an integer below 2^24
    # the whole table (with its tail) is one the oracle and the loader take: it ends in one channel
    assert int(np.asarray(t["voc.program"])[-1][2]) == 1


def test_every_case_names_a_reachable_variant():
    named = set()
    for c in R.CASES.values():
        for k in ("exact", "split"):
            if c[k]:
                named |= {p.split("/")[0] for p in c[k].split("+")}
    named |= {c["variant"] for c in R.ENC_CASES.values()}
    assert named == R.REACHABLE


@pytest.mark.parametrize("name", list(R.ENC_CASES))
@pytest.mark.parametrize("data", ["int", "real"])
def test_encoder_reference_matches_enc_ref(name, data):
    c = R.ENC_CASES[name]
    t = R.build_enc_table(c["C"], c["M"], c["k"], c["dil"], data, c["seed"])
    pcm = R.enc_pcm(c["n"], data, c["seed"])
    y, bound = R.enc_reference_f64(t, pcm, bound=True)
    for b in range(3):
        want, _ = enc_reference(t, pcm[b], n_ops=2, dtype=torch.float64)
        assert np.abs(y[b] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
    if data == "int":
        assert np.array_equal(y, np.round(y)) and np.abs(y).max() < 2 ** 24
    assert np.all(bound >= 0)
