#!/usr/bin/env python3
"""What loading the talker costs, by file format: wrapper_load_model of the full 28-layer talker from a Q4_K_M-shaped GGUF
(Q4_K everywhere, Q6_K for attn_v / ffn_down / output), from a Q8_0 GGUF, and from the F16 re-keyed safetensors of the same
shapes.

Synthetic weights (random valid blocks with weight-like scales; the values do not matter to a load), token_embd / output
padded to 4000 rows (the deployed file pads them to the text vocabulary, of which the loader uploads the same 3072 codec
rows).  Every load is a child process of its own under `timeout` (one process on the GPU at a time): it times
wrapper_load_model alone (wall clock, files already in the page cache: they were just written) and the driver reads the
loader's own line about the dequantiser -- launches and their GPU time between HIP events -- from the child's stderr.
--reps loads per format, median with min..max.  Nothing here is a target: nobody had measured a load before.  Writes
profiles/gguf_load.json and profiles/gguf_load.md.

    python scripts/gguf_load.py --commit $(git rev-parse --short HEAD)
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GGML = {"F32": (0, 1, 4), "Q8_0": (8, 32, 34), "Q4_K": (12, 256, 144), "Q6_K": (14, 256, 210)}   # number, block elements, bytes
D_AT = {"Q8_0": ((0, 0.02 / 73),), "Q4_K": ((0, 1e-4), (2, 7.5e-4)), "Q6_K": ((208, 0.02 / 1369),)}
PARTS = (("attn_norm", "input_ln", "input_layernorm"), ("attn_q", "q_proj", "self_attn.q_proj"), ("attn_k", "k_proj", "self_attn.k_proj"),
         ("attn_v", "v_proj", "self_attn.v_proj"), ("attn_output", "o_proj", "self_attn.o_proj"),
         ("attn_q_norm", "q_norm", "self_attn.q_norm"), ("attn_k_norm", "k_norm", "self_attn.k_norm"),
         ("ffn_norm", "post_ln", "post_attention_layernorm"), ("ffn_gate", "gate_proj", "mlp.gate_proj"),
         ("ffn_up", "up_proj", "mlp.up_proj"), ("ffn_down", "down_proj", "mlp.down_proj"))
Q6_IN_MIX = ("attn_v", "ffn_down", "output")
PADDED_ROWS = 4000


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def gstr(s):
    b = s.encode()
    return struct.pack("<Q", len(b)) + b


_POOL = {}


def random_blocks(tname, n, rng, pool=_POOL):
    """n blocks drawn from a pool of 4096 random ones whose scales give weights near N(0, 0.02^2)"""
    if tname not in pool:
        b = rng.integers(0, 256, (4096, GGML[tname][2]), dtype=np.uint8)
        for at, mag in D_AT[tname]:
            bits = (mag * rng.uniform(0.5, 1.5, len(b))).astype(np.float16).view(np.uint16)
            b[:, at], b[:, at + 1] = bits & 0xff, bits >> 8
        pool[tname] = b
    return pool[tname][rng.integers(0, 4096, n)]


def write_gguf(path, cfg, mat, mix, rng):
    """The talker as llama.cpp's converter names it: matrices of type `mat` (mix: Q6_K for Q6_IN_MIX), norms F32."""
    from qwen3_tts_axera_russian_amd import weights as W
    shapes = W.layer_shapes(cfg, cfg.talker_ffn)
    tens = []
    for i in range(cfg.talker_layers):
        for g, c, _ in PARTS:
            tens.append((f"blk.{i}.{g}.weight", shapes[c], "F32" if len(shapes[c]) == 1 else ("Q6_K" if mix and g in Q6_IN_MIX else mat)))
    tens += [("output_norm.weight", (cfg.hidden,), "F32"), ("token_embd.weight", (PADDED_ROWS, cfg.hidden), mat),
             ("output.weight", (PADDED_ROWS, cfg.hidden), "Q6_K" if mix else mat)]
    u32 = lambda k, v: gstr(k) + struct.pack("<II", 4, v)
    f32 = lambda k, v: gstr(k) + struct.pack("<If", 6, v)
    kvs = [gstr("general.architecture") + struct.pack("<I", 8) + gstr("qwen3"), u32("qwen3.block_count", cfg.talker_layers),
           u32("qwen3.embedding_length", cfg.hidden), u32("qwen3.feed_forward_length", cfg.talker_ffn),
           u32("qwen3.attention.head_count", cfg.n_heads), u32("qwen3.attention.head_count_kv", cfg.n_kv_heads),
           u32("qwen3.attention.key_length", cfg.head_dim), f32("qwen3.attention.layer_norm_rms_epsilon", 1e-6),
           f32("qwen3.rope.freq_base", 1e6)]
    head = b"GGUF" + struct.pack("<IQQ", 3, len(tens), len(kvs)) + b"".join(kvs)
    off, sizes = 0, []
    for name, shape, tn in tens:
        num, bs, bb = GGML[tn]
        nb = int(np.prod(shape)) // bs * bb
        head += gstr(name) + struct.pack("<I", len(shape)) + b"".join(struct.pack("<Q", x) for x in reversed(shape)) + struct.pack("<IQ", num, off)
        sizes.append(nb)
        off = (off + nb + 31) // 32 * 32
    with open(path, "wb") as f:
        f.write(head + b"\0" * (-len(head) % 32))
        for (name, shape, tn), nb in zip(tens, sizes):
            if tn == "F32":
                raw = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32).tobytes()
            else:
                raw = random_blocks(tn, nb // GGML[tn][2], rng).tobytes()
            f.write(raw + b"\0" * (-len(raw) % 32))
    return os.path.getsize(path)


def write_safetensors(dirpath, cfg, rng):
    """The re-keyed Qwen3 talker the reference's converter writes before its GGUF step, matrices F16."""
    import torch
    from safetensors.torch import save_file
    from qwen3_tts_axera_russian_amd import weights as W
    shapes = W.layer_shapes(cfg, cfg.talker_ffn)
    pool = (0.02 * rng.standard_normal(1 << 22)).astype(np.float16)

    def mat(shape):   # a random window of the pool
        n = int(np.prod(shape))
        o = int(rng.integers(0, pool.size - n))
        return torch.from_numpy(pool[o:o + n].reshape(shape).copy())

    vec = lambda shape: torch.from_numpy((1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32))
    t = {}
    for i in range(cfg.talker_layers):
        for _, c, hf in PARTS:
            t[f"model.layers.{i}.{hf}.weight"] = vec(shapes[c]) if len(shapes[c]) == 1 else mat(shapes[c])
    t["model.norm.weight"] = vec((cfg.hidden,))
    t["model.embed_tokens.weight"] = mat((PADDED_ROWS, cfg.hidden))
    t["lm_head.weight"] = mat((PADDED_ROWS, cfg.hidden))
    os.makedirs(dirpath, exist_ok=True)
    p = os.path.join(dirpath, "model.safetensors")
    save_file(t, p, metadata={"format": "pt"})
    return os.path.getsize(p)


def worker(a):
    """one load: prints {"load_ms": ..} on stdout; the library's log goes to stderr"""
    from qwen3_tts_axera_russian_amd import hiplib
    lib = hiplib.load()
    if lib.q3_device_count() <= 0:
        raise SystemExit("no HIP device")
    lib.wrapper_backend_init()
    t0 = time.perf_counter()
    m = lib.wrapper_load_model(os.fsencode(a.worker), 0)
    ms = (time.perf_counter() - t0) * 1e3
    if not m:
        raise SystemExit("wrapper_load_model failed")
    lib.wrapper_free_model(m)
    print(json.dumps({"load_ms": ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="(internal) load this path once and report")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--timeout", type=int, default=120, help="seconds, per load")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gguf_load"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    from qwen3_tts_axera_russian_amd import weights as W
    cfg = W.ModelConfig(talker_layers=a.layers)
    tmp = tempfile.mkdtemp(prefix="gguf_load_")
    rows = []
    try:
        rng = np.random.default_rng(1)
        files = [("GGUF Q4_K_M-shaped (Q4_K + Q6_K)", os.path.join(tmp, "talker_q4_k_m.gguf"), lambda p: write_gguf(p, cfg, "Q4_K", True, rng)),
                 ("GGUF Q8_0", os.path.join(tmp, "talker_q8_0.gguf"), lambda p: write_gguf(p, cfg, "Q8_0", False, rng)),
                 ("re-keyed safetensors F16", os.path.join(tmp, "talker_as_qwen3"), lambda p: write_safetensors(p, cfg, rng))]
        for label, path, make in files:
            size = make(path)
            loads, dq = [], None
            for r in range(a.reps):
                p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", path],
                                   capture_output=True, text=True, cwd=ROOT)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-4000:])
                    raise SystemExit(f"{label}: load {r} ended with status {p.returncode}; nothing more is started")
                loads.append(json.loads(p.stdout.strip().splitlines()[-1])["load_ms"])
                m = re.search(r"(\d+) quantised tensors \(([\d.]+) MB of blocks\).*: (\d+) launches, ([\d.]+) ms of GPU time", p.stderr)
                if m:
                    dq = dq or {"tensors": int(m.group(1)), "block_mb": float(m.group(2)), "launches": int(m.group(3)), "gpu_ms": []}
                    dq["gpu_ms"].append(float(m.group(4)))
            if dq:
                dq["gpu_ms"] = spread(dq["gpu_ms"])
            rows.append({"format": label, "file_mb": round(size / 1e6, 1), "load_ms": spread(loads), "dequant": dq})
            print(f"[gguf_load] {label}: {rows[-1]['file_mb']} MB, load {rows[-1]['load_ms']['median']:.1f} ms"
                  + (f", dequant {dq['launches']} launches {dq['gpu_ms']['median']:.3f} ms GPU" if dq else ""), file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res = {"what": "wrapper_load_model of the 28-layer synthetic talker by file format", "commit": a.commit, "layers": a.layers,
           "padded_table_rows": PADDED_ROWS, "reps": a.reps, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(a.out + ".md", "w") as f:
        f.write("# Talker load time by file format\n\n")
        f.write(f"`scripts/gguf_load.py` at {a.commit or '(uncommitted)'}: `wrapper_load_model` of the {a.layers}-layer synthetic talker, each load a fresh "
                f"process, wall clock of the call alone, files in the page cache; median (min..max) of {a.reps}.  The dequantiser's launches and "
                "their GPU time (between HIP events) are the loader's own count.  Recorded, not gated.\n\n")
        f.write("| file | size MB | load ms | dequant launches | dequant GPU ms | blocks uploaded MB |\n|---|---|---|---|---|---|\n")
        for r in rows:
            l, d = r["load_ms"], r["dequant"]
            f.write(f"| {r['format']} | {r['file_mb']} | {l['median']} ({l['min']}..{l['max']}) | "
                    + (f"{d['launches']} | {d['gpu_ms']['median']} ({d['gpu_ms']['min']}..{d['gpu_ms']['max']}) | {d['block_mb']} |\n" if d else "- | - | - |\n"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
