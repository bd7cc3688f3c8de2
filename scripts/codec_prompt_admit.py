#!/usr/bin/env python3
"""Cost of a per-slot admission with a codec prompt (q3e_admit_prompted), as a miss and as a prefix-cache hit.

bench.py's synthetic 0.6B-architecture weights (28 talker + 5 code-predictor layers), a per-slot batch of 32 open
(q3e_open), 24 of its slots running ordinary utterances, the admissions going into one of the others.  A 16-row prefix and a
prompt of T frames, T in --frames; for each T it times, in ONE process:

    plain   q3e_admit_prompted, no key                      the prompt launch and one prefill over 16 + T rows
    miss    ..., a key the cache has not seen               the same, then the store into the pool
    hit     ..., a key it holds                             the prompt launch (ring only), the copy launch, the final norm

and records q3e_last_prefill_ms (HIP events on the engine's stream around the call's device work) and the wall time of
FrameEngine.admit -- medians of --reps calls after one untimed call -- and, for context, the per-step time of the same
engine right after (q3e_last_run_ms / steps, 32 rows stepping): what teacher-forcing the same T frames through the frame
loop, one step each, would cost is T times that.

The driver (no --worker) runs the measurement as a child process under its own `timeout` and stops at the first failure;
then it writes profiles/codec_prompt.json and profiles/codec_prompt.md.

    python scripts/codec_prompt_admit.py --commit $(git rev-parse --short HEAD)
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, BUSY, ROWS, STEPS = 32, 24, 16, 16


def worker(a):
    import bench
    from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
    frames = [int(x) for x in a.frames.split(",")]
    path, _ = bench.make_pack(a.cache, a.seed, 0, lambda: None)
    prefixes, n_text, pad = bench.workload(BATCH, 0, a.seed)
    budget = 64
    longest = ROWS + max(frames)
    eng = FrameEngine(path, max_batch=BATCH, n_ctx=max(max(p.shape[0] for p in prefixes), longest) + budget + 8, max_frames=budget)
    eng.set_pad_embed(pad)
    eng.prefix_cache(2, longest)
    eng.open(BATCH, ignore_eos=True)
    busy = [SlotParams(max_frames=budget)] * BUSY
    eng.admit(list(range(BUSY)), prefixes[:BUSY], n_text[:BUSY], busy)
    assert eng.run(8) == 8                       # eager frame + capture: the batch is running
    rng = np.random.default_rng(a.seed)
    prefix = (0.03 * rng.standard_normal((ROWS, 1024))).astype(np.float32)
    slot, params = [BATCH - 1], [SlotParams(max_frames=budget)]
    serial = [0]

    def fresh_key():
        serial[0] += 1
        return int(serial[0]).to_bytes(8, "little") + b"prompt~~"

    out = []
    for T in frames:
        P = rng.integers(0, 2048, size=(T, 16)).astype(np.int32)
        held = fresh_key()

        def call(key, want_hit):
            eng.release(slot)
            t = time.perf_counter()
            hit = eng.admit(slot, [prefix], [30], params, keys=None if key is None else [key], prompts=[P])
            wall = (time.perf_counter() - t) * 1e3
            if key is not None:
                assert bool(hit[0]) == want_hit, (T, hit)
            return eng.last_prefill_ms, wall

        res = {}
        for name in ("plain", "miss", "hit"):
            if name == "hit":
                call(held, False)                # brings the entry
            samples = []
            for i in range(a.reps + 1):          # (the first call is untimed)
                samples.append(call(None if name == "plain" else held if name == "hit" else fresh_key(), name == "hit"))
            dev, wall = zip(*samples[1:])
            res[name] = {"prefill_ms": round(float(np.median(dev)), 4), "wall_ms": round(float(np.median(wall)), 4),
                         "prefill_ms_all": [round(x, 4) for x in dev], "wall_ms_all": [round(x, 4) for x in wall]}
        # the frame loop with the prompted utterance live, every other slot as it was: the running ones are re-admitted when
        # their budget is used up, so that 32 rows step as they do in a server under load
        done, per = eng.done()
        if int(per[:BUSY].max()) + STEPS > budget:
            eng.admit(list(range(BUSY)), prefixes[:BUSY], n_text[:BUSY], busy)
        assert eng.run(STEPS) == STEPS
        step_ms = eng.last_run_ms / STEPS
        out.append({"prompt_frames": T, "rows": ROWS + T, **res, "step_ms": round(step_ms, 4)})
        print(f"[codec_prompt_admit] T {T:3d}: " + ", ".join(f"{k} {v['prefill_ms']:.3f} / {v['wall_ms']:.3f} ms" for k, v in res.items()) +
              f", step {step_ms:.3f} ms", file=sys.stderr, flush=True)
    stats = eng.prefix_stats()
    eng.destroy()
    json.dump({"rows": out, "stats": stats, "batch": BATCH, "busy_slots": BUSY, "prefix_rows": ROWS, "reps": a.reps, "steps": STEPS},
              open(a.out, "w"), indent=1)


def table(res):
    lines = ["| prompt frames T | rows prefilled | plain: device / wall ms | miss: device / wall ms | hit: device / wall ms | step ms | T x step ms | T x step / miss (device) |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in res["rows"]:
        f = lambda k: f"{r[k]['prefill_ms']:.3f} / {r[k]['wall_ms']:.3f}"
        forced = r["prompt_frames"] * r["step_ms"]
        lines.append(f"| {r['prompt_frames']} | {r['rows']} | {f('plain')} | {f('miss')} | {f('hit')} | {r['step_ms']:.3f} | {forced:.1f} | "
                     f"{forced / r['miss']['prefill_ms']:.1f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="0,25,125,375")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--cache", default=os.environ.get("Q3_BENCH_CACHE", "/tmp/q3_bench_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_prompt.json"))
    ap.add_argument("--commit", default=None, help="the commit the measured tree is (default: git rev-parse)")
    ap.add_argument("--step_timeout", type=int, default=420, help="seconds the measurement process may take")
    ap.add_argument("--worker", action="store_true", help="(internal) the measurement itself")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True).strip()
        except Exception:      # noqa: BLE001 -- a tree without its history
            commit = "unknown"
    tmp = a.out + ".part"
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--frames", a.frames,
           "--reps", str(a.reps), "--seed", str(a.seed), "--cache", a.cache, "--out", tmp]
    rc = subprocess.call(cmd)
    if rc != 0:
        print(f"[codec_prompt_admit] the measurement ended with status {rc}: nothing written", file=sys.stderr)
        return rc
    res = json.load(open(tmp))
    os.remove(tmp)
    res["commit"] = commit
    json.dump(res, open(a.out, "w"), indent=1)
    md = os.path.splitext(a.out)[0] + ".md"
    with open(md, "w") as f:
        f.write(f"""# Codec prompts: a prompted per-slot admission as a miss and as a prefix-cache hit

Produced by `scripts/codec_prompt_admit.py` from commit `{commit}` on one MI355X; the numbers are in `{os.path.basename(a.out)}`.

bench.py's synthetic 0.6B-architecture weights (28 talker + 5 code-predictor layers), a per-slot batch of {res['batch']} open,
{res['busy_slots']} slots running, the admissions into another.  The utterance has a {res['prefix_rows']}-row prefix and a codec prompt of T frames
(`q3e_admit_prompted`); one process measured everything; each figure is the median of {res['reps']} calls after one untimed call.
"device" is `q3e_last_prefill_ms` (HIP events around the call's work on the engine's stream: the prompt launch, the prefill
over {res['prefix_rows']} + T rows or the copy launch and the final norm, then the codec head over the batch), "wall" the time of
`FrameEngine.admit` with its numpy packing.

- plain: no key.
- miss: a key the cache has not seen: the prompt launch (rows and ring), the prefill, then the store (one launch).
- hit: a key it holds: the prompt launch (ring only), one copy launch over all layers, the one-row final norm.
- step: `q3e_last_run_ms / {res['steps']}` of the same engine right after, {res['batch']} rows stepping.  "T x step" is what feeding the same
  T frames through the frame loop one step each (`q3e_set_forced_codes`, the only way before this change, and not available
  to a per-slot batch) would take at that step time; the last column is that against the measured miss.

{table(res)}

Nothing here is a target: the table states what was measured.  Counters of the run: {res['stats']}.
""")
    print(open(md).read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
