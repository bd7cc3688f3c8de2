"""tests/attn_ref.py (the float64 reference the GPU attention tests grade every kernel variant with) against transformers'
Qwen3 attention: Qwen3RMSNorm on the q / k heads, apply_rotary_pos_emb, eager GQA attention with a causal mask -- so the
kernels' reference cannot share a misunderstanding with the kernels (norm placement, the rotate-half pairing and sign,
q head h -> kv head h // 2, the 1/sqrt(128) scale, causality).

The expected values in tests/golden/attn_hf_golden.npz come from tests/golden/make_attn_golden.py (float32, random norm
weights, RoPE positions up to 4095).  With HF's own rope tables the reference must agree to float32 round-off; the tables
tests/attn_ref.rope_tables builds (the model loader's f32 arithmetic) must agree with HF's to the f32 rounding of angles
up to 4095 rad.  When transformers is importable the fixture is regenerated live as well."""
import os

import numpy as np
import pytest

from tests import attn_ref as A
from tests.golden import make_attn_golden as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_hf_golden.npz")
TOL = 2e-5       # relative to the output's max: float32 round-off of the HF evaluation


@pytest.fixture(scope="module")
def world():
    inputs, digest = G.make_inputs()
    g = np.load(GOLD)
    assert bytes(g["inputs_sha256"]).decode() == digest, \
        "seeded inputs differ from the ones the HF outputs were generated on: re-run tests/golden/make_attn_golden.py"
    return inputs, g


def reference(qkv, q_norm, k_norm, pos, cos, sin, fp16_cache=False):
    """attn_ref over one causal sequence: RoPE at `pos`, cache rows 0 .. n-1 of one slot."""
    n = qkv.shape[0]
    tab_c = np.zeros((int(pos.max()) + 1, 64), np.float32)
    tab_s = np.zeros_like(tab_c)
    tab_c[pos], tab_s[pos] = cos, sin
    q, k, v = A.prep(qkv, q_norm, k_norm, G.EPS, tab_c, tab_s, pos)
    kc = np.zeros((1, A.NKV, n, A.D))
    vc = np.zeros_like(kc)
    idx = np.arange(n)
    if fp16_cache:
        kc, vc = A.write_cache(kc.astype(np.float16), vc.astype(np.float16), k, v, np.zeros(n, int), idx)
    else:
        kc[0, :, idx], vc[0, :, idx] = k, v
    out, _ = A.attend(q, kc, vc, np.zeros(n, int), idx)
    return out


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("case", [c[0] for c in G.CASES])
def test_reference_matches_hf_qwen3_attention(world, case):
    inputs, g = world
    qkv, qn, kn, pos = inputs[case]
    want = g[f"{case}_out"].astype(np.float64)
    e = rel(reference(qkv, qn, kn, pos, g[f"{case}_cos"], g[f"{case}_sin"]), want)
    print(f"{case}: rel err vs HF {e:.2e}")
    assert e <= TOL
    # the contract's fp16 K / V cache is the only other difference (half an fp16 ulp per entry)
    assert rel(reference(qkv, qn, kn, pos, g[f"{case}_cos"], g[f"{case}_sin"], fp16_cache=True), want) <= 2e-3


def test_reference_is_sensitive_to_what_it_pins(world):
    """The fixture tells the contract's ingredients apart: each plausible misreading misses it by far more than TOL."""
    inputs, g = world
    qkv, qn, kn, pos = inputs["mid"]
    c, s = g["mid_cos"], g["mid_sin"]
    want = g["mid_out"].astype(np.float64)
    wrong = {
        "k norm weight on q": reference(qkv, kn, kn, pos, c, s),
        "rotate-half sign": reference(qkv, qn, kn, pos, c, -s),
        "rope positions off by one": reference(qkv, qn, kn, pos, np.roll(c, 1, 0), np.roll(s, 1, 0)),
    }
    swapped = qkv.copy()        # q head 2g+1 <-> 2g+2 (its kv head changes)
    q = swapped[:, :A.NH * A.D].reshape(-1, A.NH, A.D)
    q[:, 1:-1] = q[:, 1:-1].reshape(-1, 7, 2, A.D)[:, :, ::-1].reshape(-1, 14, A.D)
    wrong["gqa head map"] = reference(swapped, qn, kn, pos, c, s)
    for name, out in wrong.items():
        if name == "gqa head map":   # un-swap the output heads so only the kv mapping differs
            o = out.reshape(-1, A.NH, A.D)
            o[:, 1:-1] = o[:, 1:-1].reshape(-1, 7, 2, A.D)[:, :, ::-1].reshape(-1, 14, A.D)
        assert rel(out, want) > 100 * TOL, name


def test_rope_tables_match_hf(world):
    """The loader's f32 tables against HF's: equal but for the f32 rounding of the angle (pos * inv_freq < 4096 rad)."""
    _, g = world
    cos, sin = A.rope_tables(4096)
    for name, off, n in G.CASES:
        p = np.arange(off, off + n)
        tol = 4 * (off + n) * 2.0 ** -24
        assert np.abs(cos[p] - g[f"{name}_cos"]).max() <= tol
        assert np.abs(sin[p] - g[f"{name}_sin"]).max() <= tol


def test_fixture_regenerates_live(world):
    """With transformers importable, its Qwen3 attention on the same inputs gives the stored outputs again."""
    pytest.importorskip("transformers")
    pytest.importorskip("torch")
    import torch
    inputs, g = world
    with torch.no_grad():
        for name, (qkv, qn, kn, pos) in inputs.items():
            o, c, s = G.hf_attention(qkv, qn, kn, pos)
            assert rel(o, g[f"{name}_out"].astype(np.float64)) <= 1e-6
            np.testing.assert_allclose(c, g[f"{name}_cos"], atol=1e-6)
            np.testing.assert_allclose(s, g[f"{name}_sin"], atol=1e-6)
