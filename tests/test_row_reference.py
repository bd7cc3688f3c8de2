"""tests/row_ref.py (the reference of tests/test_gpu_row_kernels.py) against hand-worked values, and the final norm's error
bound against a numpy-float32 emulation of the kernel's operation order -- no GPU."""
import numpy as np

from tests import row_ref as RR
from tests import sample_ref as SR


def test_final_norm_hand_values():
    # sum(ssq) / H + eps = 4 exactly -> inv = 1/2
    H = 32
    h = np.arange(H, dtype=np.float32)
    g = np.full(H, 3.0, np.float32)
    ssq = np.array([100.0, 28.0 - 32 * 0.25], np.float32)     # NOT the sums of squares of h
    o = RR.final_norm_ref(h, ssq, g, 0.25, H)
    np.testing.assert_array_equal(o, h * 1.5)
    np.testing.assert_array_equal(RR.final_norm_f32(h, ssq, g, 0.25, H), (h * 1.5).astype(np.float32))
    assert RR.final_norm_roundings(2) == 13 and RR.final_norm_roundings(64) == 13 and RR.final_norm_roundings(65) == 14
    assert RR.final_norm_bound(1.0, 64) == 13 * 2.0 ** -24 + 2.0 ** -149
    np.testing.assert_array_equal(RR.f16_of([1e9, -7e4, 3.0]), [65504.0, -65504.0, 3.0])


def test_final_norm_bound_holds_for_the_f32_emulation():
    """The kernel's order in np.float32 stays inside the bound derived from counting its roundings, at both widths the GPU
    test runs, over nine decades of scale; and the bound is tight enough to tell a neighbouring row's partials apart."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for H in (96, 1024):
        parts = H // 16
        for trial in range(300):
            scale = 10.0 ** rng.uniform(-4, 5)
            h = (scale * rng.standard_normal(H)).astype(np.float32)
            ssq = (scale * scale * 16 * rng.uniform(0.2, 3.0, parts)).astype(np.float32)
            g = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)
            eps = (1e-6, 1e-5, 0.5)[trial % 3]
            o = RR.final_norm_ref(h, ssq, g, eps, H)
            err = np.abs(RR.final_norm_f32(h, ssq, g, eps, H).astype(np.float64) - o)
            bound = RR.final_norm_bound(o, parts)
            assert (err <= bound).all()
            worst = max(worst, float((err / bound).max()))
            if eps < 0.1:                                   # (eps = 0.5 swamps the small-scale rows' partials)
                other = ssq * np.float32(1.01)              # another row's partials: up to 0.5 % in the scale
                assert (np.abs(RR.final_norm_ref(h, other, g, eps, H) - o) > bound)[np.abs(o) > 0].all()
    print(f"final_norm f32 emulation: worst error / bound {worst:.3f}")
    assert 0.02 < worst <= 1.0


def test_gather_token_hand_cases():
    cap = 3
    tok = np.arange(cap * 2 * 16, dtype=np.int32).reshape(cap, 2, 16)
    assert [RR.gather_token(tok, [nf, 0], cap, 5, None, 0) for nf in (0, 1, 3, 6)] == [5, 5, 69, 69]
    assert RR.gather_token(tok, [0, 2], cap, 15, None, 1) == 32 + 16 + 15
    forced = np.full_like(tok, -1)
    forced[0, 0, 5] = 7
    assert RR.gather_token(tok, [1, 0], cap, 5, forced, 0) == 7 and RR.gather_token(tok, [2, 0], cap, 5, forced, 0) == 37
    tok[0, 0, 5] = -1                                     # a finished row is not revived
    assert RR.gather_token(tok, [1, 0], cap, 5, forced, 0) == -1


def test_prompt_ring_hand_cases():
    for T in (1, 31, 32, 33, 70):
        codes = np.stack([np.arange(100, 100 + T)] * 16, axis=1)
        ring, n = RR.prompt_ring(np.full(32, -7), codes, T)
        assert n == T
        for w in range(32):
            written = [i for i in range(T) if i & 31 == w and i >= T - 32]
            assert ring[w] == (100 + written[-1] if written else -7)
        assert (ring != -7).sum() == min(T, 32)
    ring, _ = RR.prompt_ring(np.full(32, -7), np.stack([np.arange(33)] * 16, axis=1), 33)
    assert ring[0] == 32 and ring[1] == 1                 # frame 0 is older than the ring


def test_prefix_move_hand_case():
    L, S, KV, C, E, M, H = 2, 3, 2, 6, 2, 4, 32
    rng = np.random.default_rng(2)
    kc, vc = (rng.integers(0, 60000, (L, S, KV, C, 128)).astype(np.uint16) for _ in range(2))
    pool = rng.integers(0, 60000, (E, L, 2, KV, M, 128)).astype(np.uint16)
    states = rng.standard_normal((E, H + H // 16)).astype(np.float32)
    h, ssq = rng.standard_normal((5, H)).astype(np.float32), rng.standard_normal((5, H // 16)).astype(np.float32)
    k2, v2, p2, s2, h2, q2 = RR.prefix_move_ref(kc, vc, pool, states, h, ssq, slot=2, entry=1, n_rows=3, h_row=4, restore=0)
    assert (k2 == kc).all() and (v2 == vc).all() and (h2 == h).all() and (q2 == ssq).all()
    assert (p2[0] == pool[0]).all() and (s2[0] == states[0]).all()
    assert (p2[1, 1, 0, 1, :3] == kc[1, 2, 1, :3]).all() and (p2[1, 0, 1, 0, :3] == vc[0, 2, 0, :3]).all()
    assert (p2[1, :, :, :, 3:] == pool[1, :, :, :, 3:]).all()
    assert (s2[1, :H] == h[4]).all() and (s2[1, H:] == ssq[4]).all()
    k3, v3, p3, s3, h3, q3 = RR.prefix_move_ref(kc, vc, p2, s2, h, ssq, slot=0, entry=1, n_rows=3, h_row=1, restore=1)
    assert (p3 == p2).all() and (s3 == s2).all()
    assert (k3[:, 0, :, :3] == kc[:, 2, :, :3]).all() and (v3[:, 0, :, :3] == vc[:, 2, :, :3]).all()
    assert (k3[:, 0, :, 3:] == kc[:, 0, :, 3:]).all() and (k3[:, 1:] == kc[:, 1:]).all() and (v3[:, 1:] == vc[:, 1:]).all()
    assert (h3[1] == h[4]).all() and (q3[1] == ssq[4]).all() and (np.delete(h3, 1, 0) == np.delete(h, 1, 0)).all()


def test_stored_row_check_rejects_a_wrong_row():
    import pytest
    rng = np.random.default_rng(4)
    h = rng.standard_normal(96).astype(np.float32)
    g = (1.0 + 0.3 * rng.standard_normal(96)).astype(np.float32)
    ssq = SR.ssq_parts(h).astype(np.float32)
    xh = SR.xh_row(h, g).astype(np.float16).view(np.uint16)
    RR.check_stored_row(h, ssq, xh, g, "ok")
    with pytest.raises(AssertionError):
        RR.check_stored_row(h, ssq * np.float32(1.001), xh, g, "ssq")
    with pytest.raises(AssertionError):
        RR.check_stored_row(h, ssq, np.roll(xh, 1), g, "xh")
