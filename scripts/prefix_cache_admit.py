#!/usr/bin/env python3
"""Cost of a per-slot admission with and without the prefix cache (q3e_admit_keyed): miss against hit.

bench.py's synthetic 0.6B-architecture weights, a per-slot batch of 32 open (q3e_open), 24 of its slots running ordinary
utterances, the admissions going into the other 8.  For n_rows in --rows and --utts utterances per call it times, in ONE
process (a hit is judged against the miss of the same run):

    plain   q3e_admit (no key)                              one prefill per utterance
    miss    q3e_admit_keyed, keys the cache has not seen    the prefill, then the store into the pool
    hit     q3e_admit_keyed, keys it holds                  the copy launch and the final norm

and records q3e_last_prefill_ms (HIP events on the engine's stream around the call's device work) and the wall time of
FrameEngine.admit (its numpy packing included, the same for all three) -- medians of --reps calls after one untimed call.

The driver (no --worker) runs the measurement as a child process under its own `timeout` and stops at the first failure;
then it writes profiles/prefix_cache.json and profiles/prefix_cache.md.

    python scripts/prefix_cache_admit.py --commit $(git rev-parse --short HEAD)
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

BATCH, BUSY = 32, 24


def worker(a):
    import bench
    from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
    rows_list = [int(x) for x in a.rows.split(",")]
    utts_list = [int(x) for x in a.utts.split(",")]
    assert max(utts_list) <= BATCH - BUSY
    path, _ = bench.make_pack(a.cache, a.seed, 0, lambda: None)
    prefixes, n_text, pad = bench.workload(BATCH, 0, a.seed)
    budget = 64
    eng = FrameEngine(path, max_batch=BATCH, n_ctx=max(max(p.shape[0] for p in prefixes), max(rows_list)) + budget + 8, max_frames=budget)
    eng.set_pad_embed(pad)
    eng.prefix_cache(2 * max(utts_list), max(rows_list))
    eng.open(BATCH, ignore_eos=True)
    eng.admit(list(range(BUSY)), prefixes[:BUSY], n_text[:BUSY], [SlotParams(max_frames=budget)] * BUSY)
    assert eng.run(8) == 8                       # eager frame + capture: the batch is running
    rng = np.random.default_rng(a.seed)
    serial = [0]

    def fresh_keys(n):
        serial[0] += n
        return [int(serial[0] - i).to_bytes(8, "little") + b"prefix~~" for i in range(n)]

    out = []
    for n_rows in rows_list:
        for n_utt in utts_list:
            slots = list(range(BUSY, BUSY + n_utt))
            pre = [(0.03 * rng.standard_normal((n_rows, 1024))).astype(np.float32) for _ in range(n_utt)]
            params = [SlotParams(max_frames=8)] * n_utt
            held = fresh_keys(n_utt)

            def call(keys, want_hit):
                eng.release(slots)
                t = time.perf_counter()
                hit = eng.admit(slots, pre, [30] * n_utt, params, keys=keys)
                wall = (time.perf_counter() - t) * 1e3
                if keys is not None:
                    assert bool(hit.all()) == want_hit and bool(hit.any()) == want_hit, (n_rows, n_utt, hit)
                return eng.last_prefill_ms, wall

            res = {}
            for name in ("plain", "miss", "hit"):
                if name == "hit":
                    call(held, False)            # brings the entries
                samples = []
                for i in range(a.reps + 1):      # (the first call is untimed)
                    samples.append(call(None if name == "plain" else held if name == "hit" else fresh_keys(n_utt), name == "hit"))
                dev, wall = zip(*samples[1:])
                res[name] = {"prefill_ms": round(float(np.median(dev)), 4), "wall_ms": round(float(np.median(wall)), 4),
                             "prefill_ms_all": [round(x, 4) for x in dev], "wall_ms_all": [round(x, 4) for x in wall]}
            out.append({"n_rows": n_rows, "utterances": n_utt, **res})
            print(f"[prefix_cache_admit] rows {n_rows:3d} x {n_utt}: " +
                  ", ".join(f"{k} {v['prefill_ms']:.3f} / {v['wall_ms']:.3f} ms" for k, v in res.items()), file=sys.stderr, flush=True)
    assert eng.run(8) == 8                       # the running slots go on
    stats = eng.prefix_stats()
    eng.destroy()
    json.dump({"rows": out, "stats": stats, "batch": BATCH, "busy_slots": BUSY, "reps": a.reps}, open(a.out, "w"), indent=1)


def table(res):
    lines = ["| prefix rows | utterances per call | plain: device / wall ms | miss: device / wall ms | hit: device / wall ms | hit / miss (device) | hit / miss (wall) |",
             "|---:|---:|---:|---:|---:|---:|---:|"]
    for r in res["rows"]:
        f = lambda k: f"{r[k]['prefill_ms']:.3f} / {r[k]['wall_ms']:.3f}"
        lines.append(f"| {r['n_rows']} | {r['utterances']} | {f('plain')} | {f('miss')} | {f('hit')} | "
                     f"{r['hit']['prefill_ms'] / r['miss']['prefill_ms']:.2f} | {r['hit']['wall_ms'] / r['miss']['wall_ms']:.2f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8,16,40")
    ap.add_argument("--utts", default="1,8")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--cache", default=os.environ.get("Q3_BENCH_CACHE", "/tmp/q3_bench_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_cache.json"))
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
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--rows", a.rows,
           "--utts", a.utts, "--reps", str(a.reps), "--seed", str(a.seed), "--cache", a.cache, "--out", tmp]
    rc = subprocess.call(cmd)
    if rc != 0:
        print(f"[prefix_cache_admit] the measurement ended with status {rc}: nothing written", file=sys.stderr)
        return rc
    res = json.load(open(tmp))
    os.remove(tmp)
    res["commit"] = commit
    json.dump(res, open(a.out, "w"), indent=1)
    md = os.path.splitext(a.out)[0] + ".md"
    with open(md, "w") as f:
        f.write(f"""# Prefix cache: a per-slot admission as a miss and as a hit

Produced by `scripts/prefix_cache_admit.py` from commit `{commit}` on one MI355X; the numbers are in `{os.path.basename(a.out)}`.

bench.py's synthetic 0.6B-architecture weights (28 talker layers, 8 KV heads: 114 688 B of K and V per prefix row), a per-slot
batch of {res['batch']} open, {res['busy_slots']} slots running, the admissions into the others.  One process measured all three paths;
each figure is the median of {res['reps']} calls after one untimed call.  "device" is `q3e_last_prefill_ms` (HIP events around the
call's work on the engine's stream: per utterance the prefill, or the copy launch and the final norm; then the codec head over
the batch), "wall" the time of `FrameEngine.admit` with its numpy packing of the rows, which a hit pays too.

- plain: `q3e_admit`, no key.
- miss: `q3e_admit_keyed` with keys the cache has not seen: the prefill, then the store (one launch).
- hit: `q3e_admit_keyed` with keys it holds: one copy launch over all layers and the one-row final norm.

{table(res)}

Counters of the run: {res['stats']}.
""")
    print(open(md).read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
