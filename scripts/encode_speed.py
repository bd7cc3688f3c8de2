#!/usr/bin/env python3
"""Speech-tokenizer encoder speed -> profiles/encode_speed.json.

enc_encode (default config = MimiConfig() with 16 quantizers, synthetic weights) for 1 x 1 s, 1 x 10 s and 32 x 10 s of
24 kHz audio: wall time of the call (host checks, upload, kernels, download) and its GPU time (enc_last_ms: events around
upload .. codes), after warm-up calls, as the median and min..max of the repeats.  Against transformers' MimiModel.encode
(num_quantizers=16, fp32, torch CPU at 16 threads) on the same shapes.

    python scripts/encode_speed.py [--repeats 10] [--cpu-repeats 3] [--out profiles/encode_speed.json]

--stream measures the streaming encode instead (enc_stream_*, the same config and method) -> profiles/encode_stream.json:
wall and GPU ms (enc_stream_last_ms) and the launch count per push of 1 frame, 8 frames and 1 s at 1 and 32 streams, and a
10 s clip streamed in 1 s pushes beside enc_encode of the same clip in the same run.

    python scripts/encode_speed.py --stream [--repeats 10] [--stream-out profiles/encode_stream.json]
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


def stream_leg(path, repeats, warmup):
    """Steady-state pushes: every stream is one second in (the attention window is part full, as in live use) and keeps
    running; each timed push gives every stream the same number of new samples."""
    enc = Encoder(path, max_batch=32, max_samples=240000)
    out = {"push": {}}
    for S in (1, 32):
        st = enc.stream(S, 24000)
        xs = clips(S, 30.0, seed=1)
        for label, n in (("1_frame", 1920), ("8_frames", 8 * 1920), ("1_s", 24000)):
            for k in range(S):
                st.reset(k)
            st.push([(k, xs[k][:24000], False) for k in range(S)])
            at = 24000
            wall, gpu, frames = [], [], 0
            for r in range(warmup + repeats):
                entries = [(k, xs[k][at:at + n], False) for k in range(S)]
                t0 = time.perf_counter()
                got = st.push(entries)
                dt = (time.perf_counter() - t0) * 1e3
                at += n
                if r >= warmup:
                    wall.append(dt)
                    gpu.append(st.last_ms)
                    frames = int(got[0].shape[0])
            out["push"][f"{S}x{label}"] = {"streams": S, "samples_each": n, "frames_each": frames, "launches": st.last_launches,
                                           "wall_ms": spread(wall), "gpu_ms": spread(gpu)}
            print(f"stream {S} x {label}: wall {statistics.median(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}), "
                  f"GPU {statistics.median(gpu):.2f} ms, {st.last_launches} launches", flush=True)
        out[f"state_bytes_per_stream"] = st.state_bytes
        out[f"device_bytes_{S}_streams"] = st.device_bytes()
        st.close()
    # a 10 s clip: streamed in 1 s pushes beside enc_encode, same run
    x = clips(1, 10.0)[0]
    st = enc.stream(1, 24000)
    whole, streamed, one = [], [], None
    for r in range(warmup + repeats):
        t0 = time.perf_counter()
        ref = enc.encode([x])[0]
        t1 = time.perf_counter()
        st.reset(0)
        parts = [st.push([(0, x[a:a + 24000], a + 24000 >= x.size)])[0] for a in range(0, x.size, 24000)]
        t2 = time.perf_counter()
        one = np.concatenate(parts)
        if r >= warmup:
            whole.append((t1 - t0) * 1e3)
            streamed.append((t2 - t1) * 1e3)
    st.close()
    enc.close()
    out["clip_10s"] = {"enc_encode_wall_ms": spread(whole), "streamed_1s_pushes_wall_ms": spread(streamed), "pushes": 10,
                       "frames": int(one.shape[0]), "ids_differing_from_enc_encode": int((one != ref).sum())}
    print(f"10 s clip: enc_encode {statistics.median(whole):.2f} ms, streamed in 1 s pushes {statistics.median(streamed):.2f} ms, "
          f"{int((one != ref).sum())} of {one.size} ids differ", flush=True)
    p1 = out["push"]["32x1_frame"]["wall_ms"]["median"]
    out["frame_period_ms"] = 80.0
    out["one_frame_push_32_streams_share_of_frame_period"] = p1 / 80.0
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
    ap.add_argument("--stream", action="store_true", help="measure the streaming encode instead (profiles/encode_stream.json)")
    ap.add_argument("--stream-out", default=os.path.join(ROOT, "profiles", "encode_stream.json"))
    a = ap.parse_args()
    ec = W.EncConfig()
    if a.stream:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "enc.q3w")
            W.write_synthetic_enc(path, ec, seed=7)
            res = stream_leg(path, a.repeats, a.warmup)
        res["what"] = ("enc_stream_push, default encoder config (MimiConfig() + 16 quantizers), synthetic weights, exact fp32; "
                       "median and min..max of the repeats after warm-up pushes")
        os.makedirs(os.path.dirname(a.stream_out), exist_ok=True)
        with open(a.stream_out, "w") as f:
            json.dump(res, f, indent=1)
        return
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
