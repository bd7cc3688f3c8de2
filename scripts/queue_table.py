#!/usr/bin/env python3
"""Which hardware queue every kernel ran on, and which stream every copy belongs to, from a rocprofv3 trace.

    Q3_NO_GRAPH=1 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o bench -- \\
        python bench.py --steps 2 --warmup 1 --no-b1
    python scripts/queue_table.py DIR            # markdown tables on stdout

The trace is split at the first `talker_sample` kernel: what starts before it is loading (weights, tables, zeroing), what
starts at or after it is the steady state (warm-up and timed steps).  A kernel row carries the id of the hardware queue
its packet went through; a copy row carries the stream it was issued on (copies run on the DMA engines or on a blit
kernel of the stream's queue -- the latter shows up among the kernels).
"""
import collections
import csv
import glob
import os
import sys


def rows(d, suffix):
    out = []
    for p in sorted(glob.glob(os.path.join(d, "**", f"*{suffix}"), recursive=True)):
        with open(p, newline="") as f:
            out += list(csv.DictReader(f))
    return out


def short(name, n=48):
    name = name.split("(")[0].replace("void ", "").replace("q3::", "").replace("(anonymous namespace)::", "")
    return name if len(name) <= n else name[:n - 1] + "~"


def table(title, items, key_names, label, t0, split):
    """items: dicts with Start_Timestamp / End_Timestamp; grouped by the columns key_names."""
    print(f"\n### {title}\n")
    if not items:
        print("(none)")
        return
    for phase, sel in (("load", lambda r: int(r["Start_Timestamp"]) < split), ("steady state", lambda r: int(r["Start_Timestamp"]) >= split)):
        part = [r for r in items if sel(r)]
        groups = collections.defaultdict(list)
        for r in part:
            groups[tuple(r.get(k, "?") for k in key_names)].append(r)
        print(f"**{phase}**: {len(part)} records on {len(groups)} distinct {' / '.join(key_names)}\n")
        if not groups:
            continue
        print("| " + " | ".join(key_names) + " | records | busy ms | first s | last s | what (count) |")
        print("|" + "---|" * (len(key_names) + 5))
        for k, rs in sorted(groups.items(), key=lambda kv: -len(kv[1])):
            busy = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rs) / 1e6
            first = (min(int(r["Start_Timestamp"]) for r in rs) - t0) / 1e9
            last = (max(int(r["End_Timestamp"]) for r in rs) - t0) / 1e9
            names = collections.Counter(label(r) for r in rs).most_common(6)
            what = ", ".join(f"{n} ({c})" for n, c in names)
            print("| " + " | ".join(k) + f" | {len(rs)} | {busy:.1f} | {first:.2f} | {last:.2f} | {what} |")
        print()


def main():
    d = sys.argv[1]
    kern = rows(d, "kernel_trace.csv")
    cop = rows(d, "memory_copy_trace.csv")
    if not kern:
        sys.exit(f"no *kernel_trace.csv under {d}")
    t0 = min(int(r["Start_Timestamp"]) for r in kern + cop)
    frames = [int(r["Start_Timestamp"]) for r in kern if "talker_sample" in r["Kernel_Name"]]
    split = min(frames) if frames else t0
    print(f"kernel records: {len(kern)}, copy records: {len(cop)}; steady state starts {(split - t0) / 1e9:.2f} s after the first record")
    print(f"kernel trace columns: {', '.join(kern[0].keys())}")
    if cop:
        print(f"copy trace columns: {', '.join(cop[0].keys())}")
    kkeys = [k for k in ("Queue_Id", "Stream_Id") if k in kern[0]]
    table("Kernels by hardware queue", kern, kkeys, lambda r: short(r["Kernel_Name"]), t0, split)
    if cop:
        ckeys = [k for k in ("Queue_Id", "Stream_Id") if k in cop[0]] or ["Direction"]
        table("Copies", cop, ckeys, lambda r: r.get("Direction", "?"), t0, split)


if __name__ == "__main__":
    main()
