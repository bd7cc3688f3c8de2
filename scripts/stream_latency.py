#!/usr/bin/env python3
"""First and last audio of one batch request: the streaming chunk walk against the generate-then-vocode reply.

One request of U utterances (bench.py's synthetic 0.6B-architecture weights, its workload and its full vocoder table) runs two
ways in one process, alternating, `--repeats` times after one untimed pass of each:

  stream  the frame loop (FrameEngine.generate_queue, check every 8 frames) hands every slot's new frames to voc_stream_push on
          ONE worker thread with the per-CU vocoder grid (voc_set_max_workgroups(-1)), at most one push in flight -- what the
          batch server does for {"stream": true};
  batch   the current reply: the frame loop to the end (q3e_start + q3e_run), then one voc_synthesize_batch call (uncapped grid).

  incremental  (--incremental) the stream leg with the carry-state decode (voc_incr_push) in place of the chunk walk: every
          check's new frames become samples at once -- what the batch server does for {"stream": true, "vocoder": "incremental"}.
          Its joined PCM is checked against Vocoder.synthesize_incremental per utterance, bit for bit.  --arithmetic picks its
          convolutions: exact (the default; leg "incremental"), split (voc_incr_set_arithmetic; leg "incremental_split") or
          both, side by side in the same process.

Both exact fp32, int16 out.  Per utterance: time from the request's start to its first and to its last final sample (batch: the
reply goes out once everything is done, so both are the request's end).  Fixed lengths (EOS off, --frames frames) and natural
lengths (EOS on).  The joined streamed PCM of every utterance is checked against the batch reply, bit for bit.

    python scripts/stream_latency.py --out profiles/stream_latency.json
    python scripts/stream_latency.py --incremental --arithmetic both --out profiles/stream_latency_incremental.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from qwen3_tts_axera_russian_amd import hiplib  # noqa: E402
from qwen3_tts_axera_russian_amd.engine import FrameEngine  # noqa: E402
from qwen3_tts_axera_russian_amd.vocoder import Vocoder  # noqa: E402


def pct(xs):
    xs = np.asarray(xs, np.float64)
    return {"p50": round(float(np.median(xs)), 1), "max": round(float(xs.max()), 1)} if len(xs) else None


def run_stream(eng, vs, pool, prefixes, n_text, frames, ignore_eos):
    U = len(prefixes)
    first, last = [None] * U, [None] * U
    pcm = [[] for _ in range(U)]
    stats = {"pushes": 0, "decode_calls": 0, "chunks": 0, "launches": 0, "split_launches": 0, "redone": 0, "push_gpu_ms": 0.0,
             "push_wall_ms": 0.0, "loop_wait_ms": 0.0}
    slot_utt, pushed = [None] * eng.max_batch, [0] * eng.max_batch
    fut = [None]
    t0 = time.perf_counter()

    def push(resets, entries):
        ts = time.perf_counter()
        for b in resets:
            vs.reset(b)
        got = vs.push([e[0] for e in entries], [e[2] for e in entries], [e[3] for e in entries])
        now = (time.perf_counter() - t0) * 1e3
        for k, (_, u, _, f) in enumerate(entries):
            if len(got[k]):
                pcm[u].append(got[k])
                if first[u] is None:
                    first[u] = now
            if f:
                last[u] = now
        stats["pushes"] += 1
        stats["decode_calls"] += getattr(vs, "last_decodes", 0)      # (the chunk walk's counters)
        stats["chunks"] += getattr(vs, "last_chunks", 0)
        stats["launches"] += getattr(vs, "last_launches", 0)         # (the incremental decode's)
        stats["split_launches"] += getattr(vs, "last_split_launches", 0)
        stats["redone"] += getattr(vs, "last_redone", 0)
        stats["push_gpu_ms"] += vs.last_ms
        stats["push_wall_ms"] += (time.perf_counter() - ts) * 1e3

    def on_frames(codes, per, owner, ended):
        resets, entries = [], []
        for b, o in enumerate(owner):
            if o is None:
                continue
            if slot_utt[b] != o:
                slot_utt[b], pushed[b] = o, 0
                resets.append(b)
            n, f = int(per[b]), b in ended
            if n > pushed[b] or f:
                entries.append((b, o, np.ascontiguousarray(codes[pushed[b]:n, b, :]), f))
                pushed[b] = n
        if not entries:
            return
        tw = time.perf_counter()
        if fut[0] is not None:
            fut[0].result()
        stats["loop_wait_ms"] += (time.perf_counter() - tw) * 1e3
        fut[0] = pool.submit(push, resets, entries)

    got = eng.generate_queue(prefixes, n_text, frames, ignore_eos=ignore_eos, check_every=8, on_frames=on_frames)
    t_loop = (time.perf_counter() - t0) * 1e3
    if fut[0] is not None:
        fut[0].result()
    wall = (time.perf_counter() - t0) * 1e3
    for u in range(U):            # an utterance whose first decision is EOS has no audio: its first sample is its end
        first[u] = last[u] if first[u] is None else first[u]
    out = [np.concatenate(p) if p else np.zeros(0, np.int16) for p in pcm]
    return got, out, first, last, wall, t_loop, stats


def run_batch(eng, voc, prefixes, n_text, frames, ignore_eos):
    U = len(prefixes)
    t0 = time.perf_counter()
    eng.start(prefixes, n_text, ignore_eos=ignore_eos, max_frames=frames)
    eng.run(frames)
    codes, per = eng.codes()
    cs = [np.ascontiguousarray(codes[:int(per[b]), b, :]) for b in range(U)]
    t_loop = (time.perf_counter() - t0) * 1e3
    out = voc.synthesize_batch(cs)
    wall = (time.perf_counter() - t0) * 1e3
    chunks, ms = voc.last_batch()
    stats = {"decode_calls": None, "chunks": chunks, "vocoder_gpu_ms": round(ms, 1)}
    return cs, out, [wall] * U, [wall] * U, wall, t_loop, stats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--cache", default=os.environ.get("Q3_BENCH_CACHE", "/tmp/q3_bench_cache"))
    ap.add_argument("--incremental", action="store_true", help="add the carry-state incremental leg (voc_incr_push)")
    ap.add_argument("--arithmetic", choices=("exact", "split", "both"), default="exact",
                    help="--incremental: the convolutions of the incremental leg(s)")
    ap.add_argument("--out", default=None, help="write the JSON result here too")
    a = ap.parse_args()
    lib = hiplib.load()
    if lib.q3_device_count() <= 0:
        raise SystemExit("stream_latency.py: no HIP device")
    path, _ = bench.make_pack(a.cache, a.seed, 0, lambda: None)
    voc_path = bench.make_voc_pack(a.cache, a.seed, 0, lambda: None)
    prefixes, n_text, pad = bench.workload(a.utts, 0, a.seed)
    U = a.utts
    eng = FrameEngine(path, max_batch=U, n_ctx=max(p.shape[0] for p in prefixes) + a.frames + 8, max_frames=a.frames)
    eng.set_pad_embed(pad)
    lib.voc_set_exact_fp32(1)
    voc = Vocoder(voc_path, 64, min(U, 32))
    vs = voc.stream(U)
    incr = {}        # leg name -> (IncrementalStream, arithmetic)
    if a.incremental:
        for arith in (("exact", "split") if a.arithmetic == "both" else (a.arithmetic,)):
            incr["incremental" if arith == "exact" else "incremental_split"] = (voc.incremental(U, arith), arith)
    pool = ThreadPoolExecutor(max_workers=1)
    result = {"what": "first / last final sample per utterance of one request, streaming chunk walk vs generate-then-vocode",
              "utterances": U, "max_frames": a.frames, "repeats": a.repeats, "vocoder": "full table, exact fp32, int16 out",
              "legs": {}}
    try:
        for leg, ignore_eos in (("fixed", True), ("natural", False)):
            runs = {"stream": [], "batch": []}
            for name in incr:
                runs[name] = []
            for rep in range(a.repeats + 1):
                for mode in runs:
                    if mode != "batch":
                        lib.voc_set_max_workgroups(-1)
                        r = run_stream(eng, vs if mode == "stream" else incr[mode][0], pool, prefixes, n_text, a.frames, ignore_eos)
                    else:
                        lib.voc_set_max_workgroups(0)
                        r = run_batch(eng, voc, prefixes, n_text, a.frames, ignore_eos)
                    if rep > 0:
                        runs[mode].append(r)
            # the two paths give the same codes and the same PCM, bit for bit
            sc, sp = runs["stream"][-1][0], runs["stream"][-1][1]
            bc, bp = runs["batch"][-1][0], runs["batch"][-1][1]
            identical = all(np.array_equal(x, y) for x, y in zip(sc, bc)) and all(np.array_equal(x, y) for x, y in zip(sp, bp))
            frames_total = int(sum(len(c) for c in bc))
            out = {"frames_total": frames_total, "frames_min_max": [int(min(len(c) for c in bc)), int(max(len(c) for c in bc))],
                   "bit_identical": bool(identical)}
            for name, (_, arith) in incr.items():
                ic, ip = runs[name][-1][0], runs[name][-1][1]
                lib.voc_set_max_workgroups(0)
                out[f"{name}_bit_identical_to_synthesize_incremental"] = bool(
                    all(np.array_equal(x, y) for x, y in zip(ic, bc)) and
                    all(np.array_equal(p, voc.synthesize_incremental(c, int16=True, arithmetic=arith)) for c, p in zip(ic, ip)))
            for mode, rs in runs.items():
                walls = [r[4] for r in rs]
                out[mode] = {
                    "first_audio_ms": pct([x for r in rs for x in r[2]]),
                    "last_audio_ms": pct([x for r in rs for x in r[3]]),
                    "wall_ms": pct(walls),
                    "frame_loop_ms": pct([r[5] for r in rs]),
                    "frames_per_s": round(frames_total / (float(np.median(walls)) / 1e3), 1),
                    "per_repeat_wall_ms": [round(w, 1) for w in walls],
                }
                st = rs[-1][6]
                if mode == "stream":
                    out[mode].update({"pushes": st["pushes"], "decode_calls": st["decode_calls"], "chunks": st["chunks"],
                                      "chunks_per_call": round(st["chunks"] / max(st["decode_calls"], 1), 2),
                                      "push_gpu_ms": round(st["push_gpu_ms"], 1), "push_wall_ms": round(st["push_wall_ms"], 1),
                                      "frame_loop_wait_for_push_ms": round(st["loop_wait_ms"], 1)})
                elif mode in incr:
                    out[mode].update({"arithmetic": incr[mode][1], "pushes": st["pushes"], "launches": st["launches"],
                                      "launches_per_push": round(st["launches"] / max(st["pushes"], 1), 1),
                                      "split_conv_launches": st["split_launches"], "entries_redone_exactly": st["redone"],
                                      "push_gpu_ms": round(st["push_gpu_ms"], 1),
                                      "push_gpu_ms_per_push": round(st["push_gpu_ms"] / max(st["pushes"], 1), 2),
                                      "push_wall_ms": round(st["push_wall_ms"], 1),
                                      "frame_loop_wait_for_push_ms": round(st["loop_wait_ms"], 1)})
                else:
                    out[mode].update({"chunks": st["chunks"], "decode_calls_min": -(-st["chunks"] // min(U, 32)),
                                      "vocoder_gpu_ms": st["vocoder_gpu_ms"]})
            result["legs"][leg] = out
            print(json.dumps({leg: out}), flush=True)
    finally:
        pool.shutdown()
        lib.voc_set_max_workgroups(0)
        lib.voc_set_exact_fp32(0)
        voc.close()
        eng.destroy()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
