"""tests/text_ref.py (what tests/test_gpu_text_stages.py grades the device with) pinned on the CPU: against
frontend.TextFrontEnd on real-valued data, its fragment index against a brute-force statement of the layout, its integer
family against int64.  CPU only."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import frontend as fe
from qwen3_tts_axera_russian_amd import weights as W
from tests import linear_ref as L
from tests import text_ref as T

V, TD, MID, H, CV = 40, 64, 96, 32, 12


def small_cfg():
    return W.ModelConfig(text_vocab=V, text_dim=TD, hidden=H, im_start=30, assistant=31, newline=32, tts_pad=33, tts_bos=34,
                         tts_eos=35, codec_pad=3, codec_bos=4, codec_nothink=5, codec_think_bos=6, codec_think_eos=7)


def special_of(cfg):
    return [getattr(cfg, k) for k in T.SPECIAL_KEYS] + [0]


@pytest.fixture(scope="module")
def real():
    """tensors, the host front-end on their fp16-rounded values, (h2 float64, bound) of every table row"""
    t = T.real_tensors(5, V, TD, MID, H, CV)
    t16 = T.table_f16(t["text.embedding"])
    host = fe.TextFrontEnd(small_cfg(), t16.astype(np.float32), t["text.fc1.weight"].astype(np.float32), t["text.fc1.bias"],
                           t["text.fc2.weight"].astype(np.float32), t["text.fc2.bias"], t["talker.codec_embedding"])
    h2, bound = T.chain(t16, t["text.fc1.weight"], t["text.fc1.bias"], t["text.fc2.weight"], t["text.fc2.bias"])
    return t, host, h2, bound


def host_noise(h2):
    """f32 evaluation of the host: far inside the composed bound (which already holds f32 accumulation of both layers and
    SILU32_ERR ~ 30 f32 ulps of the SiLU); what the final .astype(float32) adds"""
    return L.ulp32(h2)


def test_chain_matches_the_host_front_end(real):
    t, host, h2, bound = real
    ids = np.random.default_rng(1).permutation(V)
    got = host.embed_text(ids).astype(np.float64)
    err = np.abs(got - h2[ids])
    assert (err <= bound[ids] + host_noise(h2[ids])).all(), float((err / bound[ids]).max())
    assert err.max() > 0                                  # f32 against float64: equal would mean nothing was compared
    # the bound is worth something: two rows swapped, or one bias dropped, are far outside it
    assert (np.abs(got[::-1] - h2[ids]) > bound[ids] + host_noise(h2[ids])).mean() > 0.9
    nob, _ = T.chain(T.table_f16(t["text.embedding"]), t["text.fc1.weight"], t["text.fc1.bias"], t["text.fc2.weight"],
                     0 * t["text.fc2.bias"])
    assert (np.abs(got - nob[ids]) > bound[ids] + host_noise(h2[ids])).mean() > 0.9


def test_stage_functions_compose_to_the_chain(real):
    """gather -> fc -> silu_f16 -> fc fed with each other's float64 results (rounded where the device rounds) stay inside the
    composed bound, and their own bounds are the terms the composed one is built from"""
    t, _, h2, bound = real
    ids = [3, 0, 39, 17, 17]
    x16 = T.gather(T.table_f16(t["text.embedding"]), ids)
    h1, d1 = T.fc(x16, t["text.fc1.weight"], t["text.fc1.bias"])
    s, ds = T.silu_f16(h1.astype(np.float32))
    a16 = L.round_f16_sat(s.astype(np.float32))
    assert (np.abs(a16.astype(np.float64) - s) <= ds).all()
    got, d2 = T.fc(a16, t["text.fc2.weight"], t["text.fc2.bias"])
    assert (np.abs(got - h2[ids]) <= bound[ids]).all()
    assert (d1 > 0).all() and (d2 > 0).all() and (d2 < bound[ids]).all()


@pytest.mark.parametrize("n", [0, 1, 5])
def test_prefix_rows_match_the_host_front_end(real, n):
    t, host, h2, bound = real
    cfg, codec = small_cfg(), t["talker.codec_embedding"]
    ids = [int(x) for x in np.random.default_rng(n).integers(0, 30, size=n)]
    proj, src, cod = T.prefix_plan("prefix", ids, special_of(cfg))
    want = host.build_prefix(ids)
    got = T.prefix_rows(h2[proj].astype(np.float32), src, cod, codec)
    assert got.shape == want.shape == (n + 9, H)
    tol = bound[proj][src] + 2 * L.ulp32(want)
    assert (np.abs(got.astype(np.float64) - want) <= tol).all()
    # the host's own rows through prefix_rows: the same f32 add, bit for bit
    np.testing.assert_array_equal(T.prefix_rows(host.embed_text(proj), src, cod, codec)[3:7], want[3:7])
    proj, src, cod = T.prefix_plan("stream", [9], special_of(cfg))
    want = host.build_prefix_stream(9)
    got = T.prefix_rows(h2[proj].astype(np.float32), src, cod, codec)
    assert got.shape == want.shape == (8, H)
    assert (np.abs(got.astype(np.float64) - want) <= bound[proj][src] + 2 * L.ulp32(want)).all()
    proj, src, cod = T.prefix_plan("embed", ids, special_of(cfg))
    assert proj == ids and src == list(range(n)) and cod == [-1] * n


@pytest.mark.parametrize("K", [32, 64, 2048, 3072])
def test_fragment_index_is_the_documented_layout(K):
    """16-row x 32-k blocks, row blocks outermost, k blocks inside; in a block 64 lanes x 8 consecutive k, lane
    (m % 16) + 16 * ((k % 32) / 8): walked in memory order"""
    rows, pos = 48, 0
    where = np.full((rows, K), -1, np.int64)
    for mb in range(rows // 16):
        for kb in range(K // 32):
            for lane in range(64):
                m, k0 = mb * 16 + lane % 16, kb * 32 + (lane // 16) * 8
                where[m, k0:k0 + 8] = np.arange(pos, pos + 8)
                pos += 8
    assert pos == rows * K and (where >= 0).all()
    np.testing.assert_array_equal(T.frag_index(np.arange(rows)[:, None], np.arange(K)[None, :], K), where)
    buf = np.empty(rows * K, np.float32)
    a = np.random.default_rng(K).standard_normal((rows, K)).astype(np.float32)
    buf[where] = a
    np.testing.assert_array_equal(T.defrag(buf, rows, K), a)
    np.testing.assert_array_equal(T.defrag(buf[:32 * K], 17, K), a[:17])


def test_gather_rounding_edges():
    """ties to even, fp16 subnormals, saturation instead of inf; bf16 bit patterns decode exactly"""
    x = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 65519.9, 65520.0, 1e9, -1e9],
                 np.float32)
    want = np.array([1.0, 1.0 + 2.0 ** -9, 0.0, 2.0 ** -23, 2.0 ** -24, 65504.0, 65504.0, 65504.0, -65504.0], np.float64)
    got = T.table_f16(x)
    assert got.dtype == np.float16 and np.isfinite(got).all()
    np.testing.assert_array_equal(got.astype(np.float64), want)
    b = T.bf16_bits(np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -70000.0], np.float32))
    np.testing.assert_array_equal(T.bf16_to_f32(b), np.array([1.0, 1.0, 1.0 + 2.0 ** -6, -70144.0], np.float32))
    np.testing.assert_array_equal(T.table_f16(b, bf16=True).astype(np.float64), [1.0, 1.0, 1.0 + 2.0 ** -6, -65504.0])


@pytest.mark.parametrize("dims", [(48, 2048, 2048, 1024, 32), (48, 2048, 3072, 1024, 32), (40, 64, 96, 32, 12)])
def test_integer_family_is_exact(dims):
    """int_chain against plain int64 arithmetic, and against the device's own recipe in f32 / fp16 (numpy): the same integers"""
    t = T.int_tensors(11, *dims)
    ids = np.random.default_rng(2).integers(0, dims[0], size=9)
    x, h1, a, h2 = T.int_chain(t, ids)
    i = lambda k: np.asarray(t[k], np.float64).astype(np.int64)
    xi = i("text.embedding")[ids]
    assert ((xi != 0).sum(1) == 4).all() and set(np.unique(np.abs(xi))) <= {0, 32, 64}
    h1i = xi @ i("text.fc1.weight").T + i("text.fc1.bias")
    h2i = np.maximum(h1i, 0) @ i("text.fc2.weight").T + i("text.fc2.bias")
    np.testing.assert_array_equal(h1, h1i)
    np.testing.assert_array_equal(h2, h2i)
    # f32 recipe of the device, numpy's exp in place of __expf: SiLU is ReLU on these values, the rest exact
    f32 = np.float32
    v = (T.table_f16(t["text.embedding"])[ids].astype(f32) @ t["text.fc1.weight"].astype(f32).T + t["text.fc1.bias"]).astype(f32)
    with np.errstate(over="ignore"):
        s = v * (f32(1) / (f32(1) + np.exp(-v, dtype=f32)))
    a16 = L.round_f16_sat(s)
    np.testing.assert_array_equal(a16.astype(np.int64), a)
    got = a16.astype(f32) @ t["text.fc2.weight"].astype(f32).T + t["text.fc2.bias"]
    np.testing.assert_array_equal(got.astype(np.int64), h2)
    assert np.abs(h2).max() > 1000                         # not a degenerate family


def test_silu_is_relu_on_multiples_of_32():
    v = np.arange(-576, 577, 32).astype(np.float32)
    s = T.silu64(v)
    relu = np.maximum(v.astype(np.float64), 0)
    assert (np.abs(s - relu) < 2.0 ** -25).all()           # below half of fp16's smallest subnormal 2^-24
    np.testing.assert_array_equal(L.round_f16_sat(s.astype(np.float32)).astype(np.float64), relu)
