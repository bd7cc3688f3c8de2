#!/usr/bin/env python3
"""A/B of the per-slot frame step with and without the per-decision log-probabilities: ms per replayed frame step at B = 32
(bench.workload's prompts on the 0.6B synthetic weights, EOS suppressed, greedy, device events around the run), one fresh
process per sample, the variants alternating round after round, in the way of scripts/ab_sampler_rules.py:

    parent    the tree given with --parent (a checkout of the parent commit with its library built), per-slot mode
    none      this tree, no reservation (q3e_scores_reserve never called): the kernels and the graph the parent captures
    scores    this tree, q3e_scores_reserve(1): the frame's 16 sampling launches are the *_scores kernels

The spread of a variant over the rounds is the run-to-run spread the differences are read against.  Every sample also reports
the node count of the captured frame (this tree only: the parent has no q3e_graph_nodes).

    python scripts/ab_scores.py --parent DIR [--steps 200] [--rounds 4] [--out FILE.md] [--json FILE.json]"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("parent", "none", "scores")


def child(a):
    sys.path.insert(0, a.root)
    import bench
    from qwen3_tts_axera_russian_amd import engine as E
    path, cfg = bench.make_pack(a.cache, 1234, 0, lambda: None)
    B = 32
    prefixes, n_text, pad = bench.workload(B, 0, 1234)
    frames = a.warmup + a.steps
    eng = E.FrameEngine(path, max_batch=B, n_ctx=max(p.shape[0] for p in prefixes) + frames + 8, max_frames=frames)
    eng.set_pad_embed(pad)
    if a.child == "scores":
        eng.scores_reserve()
    eng.open(B, ignore_eos=True)
    eng.admit(list(range(B)), prefixes, n_text, [E.SlotParams(max_frames=frames)] * B)
    assert eng.run(a.warmup) == a.warmup          # the eager step, the capture, and replays
    assert eng.run(a.steps) == a.steps
    ms = eng.last_run_ms / a.steps
    codes, per = eng.codes()
    out = {"variant": a.child, "ms_per_step": ms, "codes_sum": int(codes.sum()), "frames": int(per.min()),
           "graph_nodes": getattr(eng, "graph_nodes", None)}
    if a.child == "scores":
        sc, _ = eng.scores()
        out["mean_logprob_code0"] = float(sc[:, :, 0].mean())
    eng.destroy()
    print(json.dumps(out), flush=True)


def median(x):
    x = sorted(x)
    return x[len(x) // 2] if len(x) % 2 else 0.5 * (x[len(x) // 2 - 1] + x[len(x) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a tree of the parent commit with its library built (omit: no parent variant)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cache", default=os.environ.get("Q3_BENCH_CACHE", "/tmp/q3_bench_cache"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds one sample may take")
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = [v for v in VARIANTS if v != "parent" or a.parent]
    res = {v: [] for v in variants}
    sums, nodes = {}, {}
    for rnd in range(a.rounds):
        for v in variants:
            root = a.parent if v == "parent" else HERE
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--root", os.path.abspath(root), "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--cache", a.cache]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:                       # nothing more is started after a failed sample
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"variant {v} failed with status {r.returncode} in round {rnd}")
            out = json.loads(r.stdout.strip().splitlines()[-1])
            res[v].append(out["ms_per_step"])
            sums.setdefault(v, set()).add(out["codes_sum"])
            nodes.setdefault(v, set()).add(out["graph_nodes"])
            print(f"round {rnd} {v}: {out['ms_per_step']:.4f} ms/step, {out['graph_nodes']} nodes", flush=True)
    lines = ["| variant | ms per frame step (median) | min | max | spread (max - min) | graph nodes | samples |", "|---|---|---|---|---|---|---|"]
    summary = {}
    for v in variants:
        x = sorted(res[v])
        n = sorted(nodes[v], key=str)
        summary[v] = {"median_ms": median(x), "min_ms": x[0], "max_ms": x[-1], "spread_ms": x[-1] - x[0], "samples_ms": res[v],
                      "graph_nodes": n[0] if len(n) == 1 else n}
        lines.append(f"| {v} | {median(x):.4f} | {x[0]:.4f} | {x[-1]:.4f} | {x[-1] - x[0]:.4f} | "
                     f"{'n/a' if n == [None] else ' '.join(str(k) for k in n)} | {' '.join(f'{y:.4f}' for y in res[v])} |")
    same = {v: len(s) == 1 for v, s in sums.items()}
    agree = len({next(iter(sums[v])) for v in variants}) == 1
    base = "parent" if a.parent else "none"
    cost = summary["scores"]["median_ms"] - summary[base]["median_ms"]
    lines += ["", f"B = 32, {a.steps} replayed steps after {a.warmup} warm-up steps, {a.rounds} rounds, one process per sample.",
              f"Every sample of a variant decoded the same codes: {same}; every variant decoded the same codes: {agree}.",
              f"scores - {base} (medians): {cost:+.4f} ms per step = {100.0 * cost / summary[base]['median_ms']:+.2f} % of the step."]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"batch": 32, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "variants": summary,
                       "same_codes_every_variant": agree, "scores_minus_base_ms": cost, "base": base}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
