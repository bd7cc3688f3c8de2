#!/usr/bin/env python3
"""Generate tests/golden/mimi_encode_golden.npz: outputs of transformers' MimiModel.encode on seeded weights, the
contract of the speech-tokenizer encoder (include/qwen3tts_enc.h).

The reference's scripts/encode_reference_audio.py calls qwen_tts's 12 Hz tokenizer encoder, which is not installable
here; that it is MimiModel.encode(..., num_quantizers=16) is recollection (DESIGN.md "Speech tokenizer encoder").  This
script runs the whole MimiModel (encode and decode halves: the converter must skip the latter) in fp32, eager
attention, on the seeded tensors of tests/enc_common.py and stores, per case:

    <case>.keys        JSON list of [state-dict key, shape] (the seeds regenerate the tensors; <case>.sha guards that)
    <case>.config      JSON MimiConfig.to_dict()
    <case>.lengths     int64 clip lengths (the clips are enc_common.seeded_clip(seed, n))
    <case>.codes{n}    int64 [frames][16]  MimiModel.encode(clip, num_quantizers=16).audio_codes[0].T
    <case>.gap{n}      float64 [frames][16]  second-best minus best distance of every decision, float64, from the stored
                       embedding and the stored ids (the margin a different f32 evaluation may flip a decision within)
    <case>.embedding{n} f32 [hidden][frames]  the pre-quantizer embedding (after the downsample)
    <case>.<stage>     f32 [C][kept columns] activations of the clip lengths[stage_clip] after each stage
                       (columns: enc_common.column_subset; <case>.<stage>.cols holds them)

Usage (transformers + torch on CPU, a few seconds):  python tests/golden/make_mimi_encode_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import enc_common as C  # noqa: E402
from tests import enc_ref  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mimi_encode_golden.npz")


def build(case):
    from transformers import MimiConfig, MimiModel
    cfg = MimiConfig(**case["cfg"])
    cfg._attn_implementation = "eager"
    m = MimiModel(cfg).to(torch.float32).eval()
    key_shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    state = C.seeded_state(case["seed"], key_shapes)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return cfg, m, key_shapes, state


def stages(m, cfg, x):
    """the activations after every stage the encoder program names (weights.enc_program)"""
    out = {}
    h = m.encoder.layers[0](x)
    out["conv_in"] = h
    li, bi = 1, 0
    for _ in cfg.upsampling_ratios:
        for j in range(cfg.num_residual_layers):
            h = m.encoder.layers[li](h)
            out[f"block{bi}_res{j}"] = h
            li += 1
        h = m.encoder.layers[li + 1](m.encoder.layers[li](h))
        out[f"block{bi}_down"] = h
        li += 2
        bi += 1
    h = m.encoder.layers[li + 1](m.encoder.layers[li](h))
    out["seanet_out"] = h
    assert li + 2 == len(m.encoder.layers)
    tf = m.encoder_transformer(h.transpose(1, 2), output_hidden_states=True, return_dict=True)
    for l in range(cfg.num_hidden_layers):
        out[f"tf{l}"] = tf.hidden_states[l + 1].transpose(1, 2)
    emb = m.downsample(tf.last_hidden_state.transpose(1, 2))
    out["embedding"] = emb
    q = m.quantizer
    out["vq_in"] = torch.cat([q.semantic_residual_vector_quantizer.input_proj(emb),
                              q.acoustic_residual_vector_quantizer.input_proj(emb)], 1)
    return {k: v[0].numpy() for k, v in out.items()}


def main():
    torch.manual_seed(0)
    out = {}
    for name, case in C.CASES.items():
        cfg, m, key_shapes, state = build(case)
        out[f"{name}.keys"] = np.frombuffer(json.dumps([[k, list(s)] for k, s in key_shapes]).encode(), np.uint8)
        out[f"{name}.sha"] = np.frombuffer(C.digest(state).encode(), np.uint8)
        out[f"{name}.config"] = np.frombuffer(json.dumps(cfg.to_dict(), default=str).encode(), np.uint8)
        out[f"{name}.lengths"] = np.asarray(case["lengths"], np.int64)
        sem = m.quantizer.semantic_residual_vector_quantizer
        ac = m.quantizer.acoustic_residual_vector_quantizer
        proj = np.concatenate([sem.input_proj.weight.detach().numpy()[:, :, 0], ac.input_proj.weight.detach().numpy()[:, :, 0]], 0)
        books = [sem.layers[0].codebook.embed.detach().numpy()] + \
                [ac.layers[i].codebook.embed.detach().numpy() for i in range(C.N_Q - 1)]
        books = np.stack(books)
        n_mismatch = 0
        for li, n in enumerate(case["lengths"]):
            clip = C.seeded_clip(case["seed"], n)
            x = torch.from_numpy(clip)[None, None, :]
            with torch.no_grad():
                codes = m.encode(x, num_quantizers=C.N_Q, return_dict=True).audio_codes[0].numpy().T   # [frames][16]
                st = stages(m, cfg, x)
                assert codes.shape[0] == int(m.get_encoded_length(torch.tensor(n))), (codes.shape, n)
            emb = st["embedding"]
            z64 = proj.astype(np.float64) @ emb.astype(np.float64)
            _, gap, _ = enc_ref.rvq_encode(z64, books.astype(np.float64), 1, forced=codes)
            # (the float64 ids of the stored embedding agree with Mimi's f32 ones but for near-ties)
            c64, _, _ = enc_ref.rvq_encode(z64, books.astype(np.float64), 1)
            n_mismatch += int((c64 != codes).sum())
            out[f"{name}.codes{n}"] = codes.astype(np.int64)
            out[f"{name}.gap{n}"] = gap
            out[f"{name}.embedding{n}"] = emb.astype(np.float32)
            if li == case["stage_clip"]:
                for k, a in st.items():
                    cols = C.column_subset(a.shape[1])
                    out[f"{name}.{k}"] = a[:, cols].astype(np.float32)
                    out[f"{name}.{k}.cols"] = cols.astype(np.int64)
            print(name, n, "samples ->", codes.shape[0], "frames; distinct ids per group",
                  [len(set(codes[:, g])) for g in range(0, 16, 5)], "min gap %.2e" % gap.min())
        print(name, "float64 ids differing from Mimi's f32 ones:", n_mismatch)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
