#!/usr/bin/env python3
"""Speech-tokenizer encoder speed -> profiles/encode_speed.json.

enc_encode (default config = MimiConfig() with 16 quantizers, synthetic weights) for 1 x 1 s, 1 x 10 s and 32 x 10 s of
24 kHz audio: wall time of the call (host checks, upload, kernels, download) and its GPU time (enc_last_ms: events around
upload .. codes), after warm-up calls, as the median and min..max of the repeats.  Against transformers' MimiModel.encode
(num_quantizers=16, fp32, torch CPU at 16 threads) on the same shapes.

    python scripts/encode_speed.py [--repeats 10] [--cpu-repeats 3] [--out profiles/encode_speed.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qwen3_tts_axera_russian_amd import weights as W  # noqa: E402
from qwen3_tts_axera_russian_amd.encoder import Encoder  # noqa: E402

SHAPES = [(1, 1.0), (1, 10.0), (32, 10.0)]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def clips(B, sec, seed=0):
    r = np.random.default_rng(seed)
    n = int(24000 * sec)
    t = np.arange(n) / 24000.0
    return [(0.2 * np.sin(2 * np.pi * (120 + 40 * b) * t) + 0.02 * r.standard_normal(n)).astype(np.float32) for b in range(B)]


def gpu_leg(path, repeats, warmup):
    enc = Encoder(path, max_batch=32, max_samples=240000)
    out = {}
    for B, sec in SHAPES:
        xs = clips(B, sec)
        for _ in range(warmup):
            enc.encode(xs)
        wall, gpu = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            codes = enc.encode(xs)
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu.append(enc.last_ms())
        out[f"{B}x{sec:g}s"] = {"clips": B, "seconds_each": sec, "frames_each": int(codes[0].shape[0]),
                                "wall_ms": spread(wall), "gpu_ms": spread(gpu),
                                "audio_seconds_per_wall_second": B * sec / (statistics.median(wall) / 1e3)}
        print(f"GPU {B} x {sec:g} s: wall {statistics.median(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}), "
              f"GPU {statistics.median(gpu):.2f} ms", flush=True)
    enc.close()
    return out


def cpu_leg(repeats, threads):
    import torch
    from transformers import MimiConfig, MimiModel
    torch.set_num_threads(threads)
    m = MimiModel(MimiConfig()).eval()
    out = {}
    for B, sec in SHAPES:
        x = torch.from_numpy(np.stack(clips(B, sec)))[:, None, :]
        reps = repeats if B == 1 else 1
        with torch.no_grad():
            m.encode(x[:, :, :24000], num_quantizers=16)            # warm-up
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                m.encode(x, num_quantizers=16)
                ts.append((time.perf_counter() - t0) * 1e3)
        out[f"{B}x{sec:g}s"] = {"wall_ms": spread(ts)}
        print(f"CPU {B} x {sec:g} s: {statistics.median(ts):.1f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_speed.json"))
    a = ap.parse_args()
    ec = W.EncConfig()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "enc.q3w")
        W.write_synthetic_enc(path, ec, seed=7)
        gpu = gpu_leg(path, a.repeats, a.warmup)
    cpu = cpu_leg(a.cpu_repeats, a.threads)
    res = {"what": "enc_encode, default encoder config (MimiConfig() + 16 quantizers), synthetic weights, exact fp32",
           "gpu": gpu, "cpu_mimi_encode": cpu, "cpu_threads": a.threads,
           "speedup_wall_median": {k: cpu[k]["wall_ms"]["median"] / gpu[k]["wall_ms"]["median"] for k in gpu},
           "torch_cpu": "transformers MimiModel.encode, num_quantizers=16, fp32"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["speedup_wall_median"]))


if __name__ == "__main__":
    main()
