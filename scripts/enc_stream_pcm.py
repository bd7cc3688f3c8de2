#!/usr/bin/env python3
"""The streaming encode's PCM front-end -> profiles/enc_stream_pcm.json and .md.  Nothing is asserted.

One stream of the default encoder config (MimiConfig() + 16 quantizers, synthetic weights, exact fp32), one second in and
running.  Per rate (16, 44.1, 48 kHz; mono s16), each timed push brings one second of audio:

    push_pcm    enc_stream_push_pcm of the second's own frames: GPU ms (enc_stream_last_ms: payload upload .. codes), wall ms
                of the call, kernel launches
    push        enc_stream_push of the same second, resampled on the host beforehand: the same three figures
    host        scipy.signal.resample_poly (float32) of that second: the wall time push_pcm replaces

One process, warm-up pushes first, medians and min..max of the repeats.

    python scripts/enc_stream_pcm.py [--repeats 9] [--warmup 3] [--out-dir profiles]
"""
import argparse
import json
import math
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

RATES = (16000, 44100, 48000)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def host_resample(x, rate):
    from scipy.signal import resample_poly
    g = math.gcd(rate, 24000)
    return resample_poly(x, 24000 // g, rate // g).astype(np.float32)


def measure(path, repeats, warmup):
    enc = Encoder(path, max_batch=1, max_samples=24000)
    st = enc.stream(2, 24000 + 64)
    out = {}
    for rate in RATES:
        seconds = 1 + warmup + repeats
        r = np.random.default_rng(rate)
        t = np.arange(seconds * rate) / rate
        x = ((0.2 * np.sin(2 * np.pi * 150 * t) + 0.02 * r.standard_normal(t.size)) * 32767).astype(np.int16)
        assert st.pcm_max_frames_in(rate) >= rate
        st.reset(0)
        st.reset(1)
        st.push_pcm([(0, x[:rate], False)], rate)
        st.push([(1, host_resample(x[:rate].astype(np.float32) / 32768.0, rate), False)])
        rows = {k: {"gpu_ms": [], "wall_ms": []} for k in ("push_pcm", "push")}
        host, launches, frames = [], {}, 0
        for i in range(warmup + repeats):
            sec = x[(1 + i) * rate:(2 + i) * rate]
            t0 = time.perf_counter()
            got = st.push_pcm([(0, sec, False)], rate)
            t1 = time.perf_counter()
            pcm_ms, launches["push_pcm"] = st.last_ms, st.last_launches
            f = sec.astype(np.float32) / 32768.0
            t2 = time.perf_counter()
            y = host_resample(f, rate)
            t3 = time.perf_counter()
            st.push([(1, y, False)])
            t4 = time.perf_counter()
            launches["push"] = st.last_launches
            if i >= warmup:
                rows["push_pcm"]["gpu_ms"].append(pcm_ms)
                rows["push_pcm"]["wall_ms"].append((t1 - t0) * 1e3)
                rows["push"]["gpu_ms"].append(st.last_ms)
                rows["push"]["wall_ms"].append((t4 - t3) * 1e3)
                host.append((t3 - t2) * 1e3)
                frames = int(got[0].shape[0])
        out[str(rate)] = {"frames_per_push": frames,
                          "push_pcm": {"gpu_ms": spread(rows["push_pcm"]["gpu_ms"]), "wall_ms": spread(rows["push_pcm"]["wall_ms"]),
                                       "launches": launches["push_pcm"]},
                          "push": {"gpu_ms": spread(rows["push"]["gpu_ms"]), "wall_ms": spread(rows["push"]["wall_ms"]),
                                   "launches": launches["push"]},
                          "host_resample_poly_wall_ms": spread(host)}
        print(f"{rate} Hz: push_pcm GPU {statistics.median(rows['push_pcm']['gpu_ms']):.3f} ms ({launches['push_pcm']} launches), "
              f"push GPU {statistics.median(rows['push']['gpu_ms']):.3f} ms ({launches['push']} launches), "
              f"host resample_poly {statistics.median(host):.3f} ms", flush=True)
    out["pcm_device_bytes"] = st.pcm_device_bytes()
    out["stream_device_bytes"] = st.device_bytes()
    st.close()
    enc.close()
    return out


def table(res):
    def cell(s):
        return f"{s['median']:.3f} ({s['min']:.3f}..{s['max']:.3f})"
    lines = ["# enc_stream_push_pcm: one second of mono s16 per push, one stream",
             "",
             res["what"],
             "",
             "| rate | push_pcm GPU ms | launches | push GPU ms | launches | push_pcm wall ms | push wall ms | host resample_poly wall ms |",
             "|---|---|---|---|---|---|---|---|"]
    for rate in RATES:
        v = res[str(rate)]
        lines.append(f"| {rate} | {cell(v['push_pcm']['gpu_ms'])} | {v['push_pcm']['launches']} | {cell(v['push']['gpu_ms'])} | "
                     f"{v['push']['launches']} | {cell(v['push_pcm']['wall_ms'])} | {cell(v['push']['wall_ms'])} | "
                     f"{cell(v['host_resample_poly_wall_ms'])} |")
    lines += ["", f"Front-end device memory: {res['pcm_device_bytes']} B beside the object's {res['stream_device_bytes']} B.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "enc.q3w")
        W.write_synthetic_enc(path, W.EncConfig(), seed=7)
        res = measure(path, max(a.repeats, 7), a.warmup)
    res["what"] = ("Default encoder config (MimiConfig() + 16 quantizers), synthetic weights, exact fp32, MI355X; the stream is one "
                   f"second in; median (min..max) of {max(a.repeats, 7)} pushes after {a.warmup} warm-up pushes, one process.")
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "enc_stream_pcm.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out_dir, "enc_stream_pcm.md"), "w") as f:
        f.write(table(res))


if __name__ == "__main__":
    main()
