#!/usr/bin/env python3
"""Frame step of a per-slot batch (q3e_open / q3e_admit) with every slot an ordinary utterance: milliseconds per step.

bench.py's synthetic 0.6B-architecture weights and workload, EOS off, greedy.  One process measures one library
(QWEN3TTS_LIB picks it), so two builds are compared by alternating processes in one session.  --reserve N calls
q3e_text_reserve(N) first (the text-stream kernels then read one more per-row counter) and --hold, with it, q3e_text_hold
(the sampler then reads that counter too and every arg-max launch a per-row flag; no slot is held: all are ordinary);
libraries older than these calls must run without them.  Prints one JSON line: the median and every run of --runs timed q3e_run(--frames) calls.

    python scripts/slot_step_ms.py --batch 32 --runs 5
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reserve", type=int, default=0)
    ap.add_argument("--hold", action="store_true", help="with --reserve: q3e_text_hold(1) before the batch opens")
    ap.add_argument("--label", default="")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--cache", default=os.environ.get("Q3_BENCH_CACHE", "/tmp/q3_bench_cache"))
    a = ap.parse_args()
    import bench
    from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
    path, _ = bench.make_pack(a.cache, a.seed, 0, lambda: None)
    prefixes, n_text, pad = bench.workload(a.batch, 0, a.seed)
    budget = a.frames * (a.runs + 1) + 8
    eng = FrameEngine(path, max_batch=a.batch, n_ctx=max(p.shape[0] for p in prefixes) + budget + 8, max_frames=budget)
    eng.set_pad_embed(pad)
    if a.reserve:
        eng.reserve_text(a.reserve)
    if a.hold:
        eng.hold_text()
    eng.open(a.batch, ignore_eos=True)
    eng.admit(list(range(a.batch)), prefixes, n_text, [SlotParams(max_frames=budget)] * a.batch)
    assert eng.run(8) == 8                       # eager frame + capture
    assert eng.run(a.frames) == a.frames         # untimed pass
    ms = []
    for _ in range(a.runs):
        assert eng.run(a.frames) == a.frames
        ms.append(eng.last_run_ms / a.frames)
    eng.destroy()
    print(json.dumps({"label": a.label, "lib": os.environ.get("QWEN3TTS_LIB", "default"), "batch": a.batch, "reserve": a.reserve, "hold": bool(a.hold),
                      "ms_per_step_median": round(float(np.median(ms)), 4), "ms_per_step": [round(x, 4) for x in ms]}))


if __name__ == "__main__":
    main()
