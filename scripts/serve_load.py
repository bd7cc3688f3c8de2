#!/usr/bin/env python3
"""Load test of batch_server: N single-text clients against --concurrent and against the sequential mode.

Synthetic Qwen3-TTS-0.6B weights as in bench.py (talker, code predictor; a 4096-entry text table, which only the host
front end reads) and bench.py's whole synthetic vocoder.  Client i sends ONE text of bench.PROMPT_TOKENS[i % 32] token
ids (seeded) as a streamed request, greedy decode with EOS (natural lengths, capped at --max_tokens).  The clients connect
at once (--rate 0) or at a fixed arrival rate.  Per mode and N: aggregate codec frames/s (all frames over the wall time from
the first connect to the last record), requests/s, time to first and to last audio (p50, p95), and the frame steps the
engine ran.  The server runs in this process (its own accept, engine and vocoder threads); one warm-up request first.

    python scripts/serve_load.py --clients 1,8,32,128 --out profiles/serve_load.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_packs(cache, seed):
    from qwen3_tts_axera_russian_amd import weights as W
    os.makedirs(cache, exist_ok=True)
    V = 4096
    cfg = W.ModelConfig(text_vocab=V, tts_pad=V - 3, tts_bos=V - 2, tts_eos=V - 1, im_start=V - 4, assistant=V - 5, newline=V - 6)
    main = os.path.join(cache, f"qwen3tts06b_synth_text4k_s{seed}.q3w")
    if not os.path.exists(main):
        t = time.time()
        W.write_synthetic(main, cfg, seed=seed, parts=("talker", "cp", "text"))
        print(f"[serve_load] wrote {main} in {time.time() - t:.0f}s", file=sys.stderr, flush=True)
    voc = os.path.join(cache, f"qwen3tts_voc_whole_s{seed}.q3w")
    if not os.path.exists(voc):
        W.write_pack(voc, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.VocConfig(), seed=seed))
    return main, voc, cfg


def texts(n, seed, vocab):
    from bench import PROMPT_TOKENS
    return [np.random.default_rng(seed + i).integers(0, vocab - 8, PROMPT_TOKENS[i % len(PROMPT_TOKENS)]).tolist()
            for i in range(n)]


def one_client(sock, ids, max_tokens, t_start, out, i):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    first = None
    frames = 0
    try:
        for rec in bs.synthesize_batch_stream(sock, token_ids=[ids], max_tokens=max_tokens):
            if rec[0] == "audio" and first is None:
                first = time.perf_counter()
            elif rec[0] == "end":
                frames += rec[2].shape[0]
        last = time.perf_counter()
        out[i] = {"t0": t_start, "first": (first or last) - t_start, "last": last - t_start, "frames": frames}
    except Exception as e:      # noqa: BLE001 -- counted as a failed request
        out[i] = {"error": repr(e)}


def run_load(sock, srv, reqs, max_tokens, rate):
    out = [None] * len(reqs)
    steps0 = srv.eng.frame_steps
    ths = []
    t_begin = time.perf_counter()
    for i, ids in enumerate(reqs):
        if rate > 0:
            time.sleep(max(0.0, t_begin + i / rate - time.perf_counter()))
        t = threading.Thread(target=one_client, args=(sock, ids, max_tokens, time.perf_counter(), out, i), daemon=True)
        t.start()
        ths.append(t)
    for t in ths:
        t.join(timeout=3600)
    wall = time.perf_counter() - t_begin
    ok = [o for o in out if o and "error" not in o]
    frames = sum(o["frames"] for o in ok)
    pct = lambda k, q: float(np.percentile([o[k] for o in ok], q)) * 1e3 if ok else None
    return {"clients": len(reqs), "ok": len(ok), "failed": len(reqs) - len(ok), "wall_s": round(wall, 3), "frames": frames,
            "frames_per_s": round(frames / wall, 1), "requests_per_s": round(len(ok) / wall, 2),
            "first_audio_ms_p50": pct("first", 50), "first_audio_ms_p95": pct("first", 95),
            "last_audio_ms_p50": pct("last", 50), "last_audio_ms_p95": pct("last", 95),
            "frame_steps": srv.eng.frame_steps - steps0,
            "errors": sorted({o["error"] for o in out if o and "error" in o})[:3]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clients", default="1,8,32,128")
    ap.add_argument("--modes", default="concurrent,sequential")
    ap.add_argument("--rate", type=float, default=0.0, help="arrivals per second (0: every client connects at once)")
    ap.add_argument("--max_batch", type=int, default=32)
    ap.add_argument("--max_tokens", type=int, default=200)
    ap.add_argument("--n_ctx", type=int, default=320)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cache", default=os.environ.get("Q3_BENCH_CACHE", "/tmp/q3_bench_cache"))
    ap.add_argument("--sock_dir", default="/tmp")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    a = ap.parse_args()
    from qwen3_tts_axera_russian_amd import batch_server as bs
    main_pack, voc, cfg = make_packs(a.cache, a.seed)
    ns = [int(x) for x in a.clients.split(",")]
    reqs = texts(max(ns), a.seed, cfg.text_vocab)
    results = {"config": {"max_batch": a.max_batch, "max_tokens": a.max_tokens, "n_ctx": a.n_ctx, "rate": a.rate,
                          "decode": "greedy, EOS on", "request": "one text per client, streamed", "weights": "synthetic 0.6B"},
               "runs": []}
    for mode in a.modes.split(","):
        sock = os.path.join(a.sock_dir, f"q3_serve_load_{os.getpid()}_{mode}.sock")
        srv = bs.BatchSynthesisServer(main_pack, voc, sock, max_batch=a.max_batch, n_ctx=a.n_ctx, max_tokens=a.max_tokens,
                                      temperature=0.0, cp_temperature=0.0, install_signal_handlers=False,
                                      concurrent=(mode == "concurrent"))
        th = threading.Thread(target=srv.serve, daemon=True)
        th.start()
        while not os.path.exists(sock):
            time.sleep(0.05)
        try:
            run_load(sock, srv, reqs[:1], a.max_tokens, 0.0)          # warm-up: graph capture, vocoder streams
            for n in ns:
                r = dict(mode=mode, **run_load(sock, srv, reqs[:n], a.max_tokens, a.rate))
                print(json.dumps(r), flush=True)
                results["runs"].append(r)
        finally:
            srv._running = False
            th.join(timeout=120)
            srv.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
