"""wrapper_load_model on the talker's GGUF -- the file the reference's server is started with -- against a Q3TTSW1 container
that holds the same values: the twin of tests/test_gpu_talker.py::test_load_talker_from_rekeyed_safetensors.

Per format (F16, BF16, Q8_0, Q4_0, a Q4_K_M-shaped mix and a Q5_K_M-shaped mix: Q4_K / Q5_K everywhere, Q6_K for attn_v,
ffn_down and output) a GGUF of the tiny model (2 layers, widths 1024 / 3072, token_embd / output padded to 4000 rows) is
written from random valid blocks, and a container from tests/gguf_ref.py's float64 formulas over the same blocks, rounded
as the contract says (f32 tables: rounded once to float32; fp16 matrices: that, to nearest even, saturating).  The device
dequantisation is exact, so the two loads hold identical weights and every output must be array-equal: the hidden state
of an 11-row prefill, of one decode step, and the codec head's logits.

The matrices are drawn block-wise from a pool of 4096 random blocks per type, so the float64 formulas run over the pool
once and not over 38 M elements per format."""
import functools
import os

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.llama_cpp_bindings import LlamaCppModel
from tests import gguf_ref as R

pytestmark = pytest.mark.gpu

PARTS = (("attn_norm", "input_ln"), ("attn_q", "q_proj"), ("attn_k", "k_proj"), ("attn_v", "v_proj"), ("attn_output", "o_proj"),
         ("attn_q_norm", "q_norm"), ("attn_k_norm", "k_norm"), ("ffn_norm", "post_ln"), ("ffn_gate", "gate_proj"),
         ("ffn_up", "up_proj"), ("ffn_down", "down_proj"))
FORMATS = {"F16": {}, "BF16": {}, "Q8_0": {}, "Q4_0": {},
           "Q4_K": {"attn_v": "Q6_K", "ffn_down": "Q6_K", "output": "Q6_K"},      # Q4_K_M-shaped
           "Q5_K": {"attn_v": "Q6_K", "ffn_down": "Q6_K", "output": "Q6_K"}}      # Q5_K_M-shaped
POOL = 4096


def tiny_config():
    return W.ModelConfig(talker_layers=2), 4000      # (2 layers, hidden 1024, ffn 3072), rows of the padded tables


class Pool:
    """POOL random blocks of a type with weight-like scales, and their contract values"""

    def __init__(self, tname, seed):
        rng = np.random.default_rng(seed)
        self.tname, self.bs = tname, R.TYPES[tname][2]
        if tname == "F16":
            self.blocks = (0.02 * rng.standard_normal((POOL * 256, 1))).astype(np.float16).view(np.uint8)
        elif tname == "BF16":
            f = (0.02 * rng.standard_normal(POOL * 256)).astype(np.float32)
            self.blocks = (f.view(np.uint32) >> 16).astype(np.uint16).reshape(-1, 1).view(np.uint8)
        else:
            self.blocks = R.random_blocks(tname, POOL, rng, scale=0.02)
        self.f32 = R.dequant64(tname, self.blocks).astype(np.float32).reshape(len(self.blocks), self.bs)
        self.f16 = R.f16_sat(self.f32)

    def draw(self, rng, rows, K):
        """-> (raw bytes of a [rows][K] tensor, its float32 values, its fp16 weights)"""
        idx = rng.integers(0, len(self.blocks), rows * K // self.bs)
        return self.blocks[idx].tobytes(), self.f32[idx].reshape(rows, K), self.f16[idx].reshape(rows, K)


@functools.lru_cache(maxsize=None)
def pool(tname):
    return Pool(tname, seed=sum(map(ord, tname)))


@functools.lru_cache(maxsize=2)
def build_case(fmt):
    """-> (GGUF bytes, {name: (offset, nbytes)}, container tensors) of the tiny model in format `fmt`"""
    cfg, padded = tiny_config()
    rng = np.random.default_rng(1000 + sum(map(ord, fmt)))
    shapes = W.layer_shapes(cfg, cfg.talker_ffn)
    gg, ct = [], {}
    for i in range(cfg.talker_layers):
        for gname, cname in PARTS:
            shape = shapes[cname]
            if len(shape) == 1:      # norm vectors travel as F32
                a = W.synth_tensor(f"talker.layers.{i}.{cname}", shape, seed=77)
                gg.append((f"blk.{i}.{gname}.weight", "F32", shape, a.tobytes()))
                ct[f"talker.layers.{i}.{cname}"] = a
            else:
                tn = FORMATS[fmt].get(gname, fmt)
                raw, _, w16 = pool(tn).draw(rng, *shape)
                gg.append((f"blk.{i}.{gname}.weight", tn, shape, raw))
                ct[f"talker.layers.{i}.{cname}"] = w16
    a = W.synth_tensor("talker.norm", (cfg.hidden,), seed=77)
    gg.append(("output_norm.weight", "F32", (cfg.hidden,), a.tobytes()))
    ct["talker.norm"] = a
    raw, e32, _ = pool(fmt).draw(rng, padded, cfg.hidden)
    gg.append(("token_embd.weight", fmt, (padded, cfg.hidden), raw))
    ct["talker.codec_embedding"] = np.ascontiguousarray(e32[:cfg.talker_vocab])
    tn = FORMATS[fmt].get("output", fmt)
    raw, _, h16 = pool(tn).draw(rng, padded, cfg.hidden)
    gg.append(("output.weight", tn, (padded, cfg.hidden), raw))
    ct["talker.codec_head"] = np.ascontiguousarray(h16[:cfg.talker_vocab])
    data, place = R.gguf_bytes(R.qwen3_kvs(layers=cfg.talker_layers), gg)
    return data, place, ct


def _prefix(rng, n, H=1024, scale=0.05):
    return (scale * rng.standard_normal((n, H))).astype(np.float32)


def outputs(llm):
    rng = np.random.default_rng(3)
    h0 = llm.get_hidden(_prefix(rng, 11), keep_history=0)
    h1 = llm.get_hidden(_prefix(rng, 1), keep_history=1)
    lg = llm.codec_head(h1)
    assert np.isfinite(h0).all() and np.isfinite(h1).all() and np.isfinite(lg).all() and np.abs(h1).max() > 0
    return h0, h1, lg


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_gguf_load_equals_the_container_of_the_same_values(gpu_lib, tmp_path, fmt):
    cfg, _ = tiny_config()
    data, _, ct = build_case(fmt)
    g = tmp_path / ("talker_%s.gguf" % fmt.lower())
    g.write_bytes(data)
    c = str(tmp_path / "same_values.q3w")
    W.write_pack(c, cfg.meta(), ct)
    a = LlamaCppModel(c, n_ctx=64)
    b = LlamaCppModel(str(g), n_ctx=64)
    try:
        for x, y in zip(outputs(b), outputs(a)):
            np.testing.assert_array_equal(x, y)
    finally:
        a.destroy()
        b.destroy()


def test_gguf_in_a_directory_and_npy_tables_beside_it(gpu_lib, tmp_path):
    """The deployed layout: a directory holding the one .gguf, and --embeddings_dir with the exact codec tables, which win
    over the GGUF's quantised token_embd / output (wrapper_load_model_aux)."""
    cfg, _ = tiny_config()
    data, _, ct = build_case("Q4_K")
    d = tmp_path / "deployed"
    d.mkdir()
    (d / "qwen3_tts_talker_q4_k_m.gguf").write_bytes(data)
    aux = tmp_path / "embeddings"
    aux.mkdir()
    rng = np.random.default_rng(9)
    emb = (0.02 * rng.standard_normal((cfg.talker_vocab, cfg.hidden))).astype(np.float32)
    head = (0.02 * rng.standard_normal((cfg.talker_vocab, cfg.hidden))).astype(np.float32)
    np.save(aux / "codec_embedding.npy", emb)
    np.save(aux / "codec_head.npy", head)
    c0, c1 = str(tmp_path / "gguf_tables.q3w"), str(tmp_path / "npy_tables.q3w")
    W.write_pack(c0, cfg.meta(), ct)
    W.write_pack(c1, cfg.meta(), dict(ct, **{"talker.codec_embedding": emb, "talker.codec_head": R.f16_sat(head)}))
    models = [LlamaCppModel(c0, n_ctx=64), LlamaCppModel(c1, n_ctx=64), LlamaCppModel(str(d), n_ctx=64),
              LlamaCppModel(str(d), n_ctx=64, embeddings_dir=str(aux))]
    try:
        want0, want1, got_dir, got_aux = [outputs(m) for m in models]
        for x, y in zip(got_dir, want0):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(got_aux, want1):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(got_aux[1], got_dir[1])        # the same hidden states ...
        assert not np.array_equal(got_aux[2], got_dir[2])            # ... under the other head
        # embeddings_dir == NULL is wrapper_load_model
        m = gpu_lib.wrapper_load_model_aux(os.fsencode(str(d)), None, 0)
        assert m
        gpu_lib.wrapper_free_model(m)
    finally:
        for m in models:
            m.destroy()


def test_damaged_and_foreign_gguf_are_refused_and_leave_the_library_usable(gpu_lib, tmp_path):
    cfg, _ = tiny_config()
    data, place, ct = build_case("Q4_K")
    # one non-finite scale: dmin = NaN in a block in the middle of blk.1.ffn_up, d = Inf in one of output's (Q6_K) codec rows
    for name, at, bits in (("blk.1.ffn_up.weight", 144 * 5000 + 2, b"\x01\x7e"), ("output.weight", 210 * 777 + 208, b"\x00\x7c")):
        bad = bytearray(data)
        o = place[name][0] + at
        bad[o:o + 2] = bits
        p = tmp_path / ("nonfinite_%s.gguf" % name.split(".")[-2])
        p.write_bytes(bytes(bad))
        assert not gpu_lib.wrapper_load_model(os.fsencode(str(p)), 0)
        with pytest.raises(RuntimeError):
            LlamaCppModel(str(p), n_ctx=64)
    # a block of output's padding rows (beyond the 3072 codec rows) is never converted: its scale does not matter
    pad = bytearray(data)
    o = place["output.weight"][0] + 210 * (3500 * 4) + 208
    pad[o:o + 2] = b"\x00\x7c"
    p = tmp_path / "nonfinite_padding.gguf"
    p.write_bytes(bytes(pad))
    m = gpu_lib.wrapper_load_model(os.fsencode(str(p)), 0)
    assert m
    gpu_lib.wrapper_free_model(m)
    # another architecture
    head_len = min(o for o, _ in place.values())
    foreign = data[:head_len].replace(R.gstr("general.architecture") + b"\x08\0\0\0" + R.gstr("qwen3"),
                                      R.gstr("general.architecture") + b"\x08\0\0\0" + R.gstr("llama"))
    assert len(foreign) == head_len
    p = tmp_path / "llama.gguf"
    p.write_bytes(foreign + data[head_len:])
    assert not gpu_lib.wrapper_load_model(os.fsencode(str(p)), 0)
    assert not gpu_lib.wrapper_load_model_aux(os.fsencode(str(p)), os.fsencode(str(tmp_path)), 0)
    # the refusals released what they held: the good file still loads and computes
    g = tmp_path / "good.gguf"
    g.write_bytes(data)
    llm = LlamaCppModel(str(g), n_ctx=64)
    try:
        outputs(llm)
    finally:
        llm.destroy()
