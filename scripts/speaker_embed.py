#!/usr/bin/env python3
"""What a speaker embedding costs: spk_embed beside enc_encode of the same clips, and beside a running frame loop.

Synthetic weights of the product's shapes (the speaker encoder at the recollected 0.6B checkpoint geometry, weights.SpkConfig:
mel 128, channels 512/512/512/512/1536, dim 1024; the default speech-tokenizer encoder config; the 0.6B-architecture talker /
code predictor and whole vocoder of scripts/serve_load.py), one process, two parts:

  embed      spk_last_ms (HIP events, upload to embedding), spk_last_launches and the wall time of SpeakerEncoder.embed for clips
             of 3 s and 10 s at B = 1 and B = 8, and enc_last_ms of Encoder.encode of the same clips in the same run: --reps
             calls after two untimed ones.
  bystander  a long streamed request runs on a --concurrent --encoder --speaker_encoder server while 10 s clips are embedded
             back to back under the server's encoder lock (what a "speaker": "only" request does on the accept thread): the
             frame loop's wall and device ms per step (FrameEngine.run, q3e_last_run_ms) of the run calls that overlap an
             embed against those that do not.

Every figure is a median with min..max beside it.  Nothing here is a target: nobody had measured an embed before.  The driver
(no --worker) runs the measurement as a child process under its own `timeout`, then writes profiles/speaker_encoder.json and
profiles/speaker_encoder.md.

    python scripts/speaker_embed.py --commit $(git rev-parse --short HEAD)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def clip(sec, seed):
    """24 kHz mono float32 inside [-1, 1]"""
    r = np.random.default_rng(seed)
    t = np.arange(int(sec * 24000)) / 24000.0
    x = 0.2 * np.sin(2 * np.pi * (110 + 7 * seed % 90) * t) + 0.1 * np.sin(2 * np.pi * 640 * t + seed) + 0.02 * r.standard_normal(t.size)
    return x.astype(np.float32)


def embed_part(a, spk, enc):
    rows = []
    for sec in (3.0, 10.0):
        for B in (1, 8):
            clips = [clip(sec, 10 * B + b) for b in range(B)]
            gpu, wall, ref = [], [], []
            for i in range(a.reps + 2):
                t0 = time.perf_counter()
                emb = spk.embed(clips)
                t1 = time.perf_counter()
                if i >= 2:
                    gpu.append(spk.last_ms())
                    wall.append((t1 - t0) * 1e3)
            for i in range(a.reps + 2):
                enc.encode(clips)
                if i >= 2:
                    ref.append(enc.last_ms())
            assert np.isfinite(emb).all()
            rows.append({"seconds": sec, "batch": B, "frames": spk.frames(clips[0].size), "launches": spk.last_launches(),
                         "spk_last_ms": spread(gpu), "embed_wall_ms": spread(wall), "enc_encode_gpu_ms": spread(ref)})
            print(f"[speaker_embed] {sec:g} s x {B}: spk {rows[-1]['spk_last_ms']['median']:.3f} ms ({rows[-1]['launches']} launches), "
                  f"wall {rows[-1]['embed_wall_ms']['median']:.3f} ms, enc_encode {rows[-1]['enc_encode_gpu_ms']['median']:.3f} ms",
                  file=sys.stderr, flush=True)
    return rows


def worker(a):
    import serve_load
    from qwen3_tts_axera_russian_amd import batch_server as bs
    from qwen3_tts_axera_russian_amd import weights as W
    main_pack, voc_pack, cfg = serve_load.make_packs(a.cache, a.seed)
    enc_pack = os.path.join(a.cache, "enc_full_s7.q3w")
    if not os.path.exists(enc_pack):
        W.write_synthetic_enc(enc_pack, W.EncConfig(), seed=7)
    spk_pack = os.path.join(a.cache, "spk_full_s7.q3w")
    if not os.path.exists(spk_pack):
        W.make_synthetic_spk(spk_pack, W.SpkConfig(), seed=7)
    sock = os.path.join(a.cache, f"speaker_embed_{os.getpid()}.sock")
    # (the server's handles take min(max_batch, 4) clips per call: the embed part opens its own pair for B = 8)
    from qwen3_tts_axera_russian_amd.encoder import Encoder
    from qwen3_tts_axera_russian_amd.speaker import SpeakerEncoder
    spk, enc = SpeakerEncoder(spk_pack, max_batch=8, max_samples=240000), Encoder(enc_pack, max_batch=8, max_samples=240000)
    out = {"geometry": "mel 128, channels 512/512/512/512/1536, Res2Net scale 8, SE 128, attention 128, dim 1024",
           "embed": embed_part(a, spk, enc)}
    spk.close()
    enc.close()
    json.dump(out, open(a.out, "w"), indent=1)       # (kept if the second part fails)
    srv = bs.BatchSynthesisServer(main_pack, voc_pack, sock, max_batch=8, n_ctx=a.max_tokens + 64 + 160, max_tokens=a.max_tokens,
                                  temperature=0.0, cp_temperature=0.0, install_signal_handlers=False, concurrent=True,
                                  encoder=enc_pack, speaker_encoder=spk_pack, prompt_audio_seconds=10.0)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(600):
        if os.path.exists(sock) and srv.sched is not None:
            break
        time.sleep(0.05)
    try:
        ids = serve_load.texts(1, a.seed, cfg.text_vocab)
        eng = srv.eng
        run0 = eng.run
        runs, embeds = [], []

        def run(n):
            t0 = time.perf_counter()
            k = run0(n)
            if k:
                runs.append((t0, time.perf_counter(), k, eng.last_run_ms))
            return k
        eng.run = run
        done = threading.Event()

        def bystander():
            for _ in bs.synthesize_batch_stream(sock, token_ids=ids, max_tokens=a.max_tokens):
                pass
            done.set()
        for _ in bs.synthesize_batch_stream(sock, token_ids=ids, max_tokens=16):      # untimed: the graph is captured
            pass
        srv.speaker.embed([clip(10.0, 999)])
        runs.clear()
        for phase in ("alone", "beside"):
            done.clear()
            t = threading.Thread(target=bystander)
            t.start()
            k = 0
            while phase == "beside" and not done.is_set():
                x = clip(10.0, 1000 + k)
                with srv._encoder_lock:
                    t0 = time.perf_counter()
                    srv.speaker.embed([x])
                    embeds.append((t0, time.perf_counter()))
                k += 1
            t.join()
        eng.run = run0
        over = lambda r: any(r[0] < e1 and e0 < r[1] for e0, e1 in embeds)
        groups = {"beside_an_embed": [r for r in runs if over(r)], "no_embed": [r for r in runs if not over(r)]}
        out["bystander"] = {"embeds": len(embeds), "embed_wall_ms": spread([(e1 - e0) * 1e3 for e0, e1 in embeds])}
        for name, rs in groups.items():
            if rs:
                out["bystander"][name] = {"run_calls": len(rs), "wall_ms_per_step": spread([(r[1] - r[0]) * 1e3 / r[2] for r in rs]),
                                          "device_ms_per_step": spread([r[3] / r[2] for r in rs])}
        print(f"[speaker_embed] bystander: {out['bystander']}", file=sys.stderr, flush=True)
    finally:
        srv._running = False
        th.join(timeout=60)
        srv.close()
    json.dump(out, open(a.out, "w"), indent=1)


def markdown(res, commit, name):
    s = lambda d: f"{d['median']:.3f} ({d['min']:.3f}..{d['max']:.3f})"
    lines = ["# Speaker encoder: what an embed costs", "",
             f"Produced by `scripts/speaker_embed.py` from commit `{commit}` on one MI355X; the numbers are in `{name}`.  Synthetic",
             f"weights at the recollected checkpoint geometry ({res['geometry']}); every figure is a median with min..max of",
             "the repeats beside it.  Nothing here is a target: nobody had measured an embed before, the tables state what was measured.",
             "", "## spk_embed against enc_encode of the same clips (same run)", "",
             "| clips | log-mel frames | launches | spk_last_ms (GPU) | embed, wall ms | enc_encode, GPU ms |", "|---|---:|---:|---:|---:|---:|"]
    for r in res["embed"]:
        lines.append(f"| {r['batch']} x {r['seconds']:g} s | {r['frames']} | {r['launches']} | {s(r['spk_last_ms'])} | {s(r['embed_wall_ms'])} | "
                     f"{s(r['enc_encode_gpu_ms'])} |")
    lines += ["", "The parent's record for `enc_encode` of one 3 s / 10 s clip is 5.7 / 7.7 ms (`profiles/prompt_audio.md`)."]
    b = res.get("bystander")
    if b:
        lines += ["", "## A bystander's frame step while clips are embedded", "",
                  f"{b['embeds']} embeds of 10 s clips (wall ms each: {s(b['embed_wall_ms'])}) back to back beside one streamed request.", "",
                  "| run calls of the frame loop | calls | wall ms / step | device ms / step |", "|---|---:|---:|---:|"]
        for k in ("no_embed", "beside_an_embed"):
            if k in b:
                lines.append(f"| {k} | {b[k]['run_calls']} | {s(b[k]['wall_ms_per_step'])} | {s(b[k]['device_ms_per_step'])} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--max_tokens", type=int, default=160)
    ap.add_argument("--cache", default=os.environ.get("Q3_BENCH_CACHE", "/tmp/q3_bench_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speaker_encoder.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--step_timeout", type=int, default=540)
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
    rc = subprocess.call(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps),
                          "--seed", str(a.seed), "--max_tokens", str(a.max_tokens), "--cache", a.cache, "--out", tmp])
    if rc != 0:
        print(f"[speaker_embed] the measurement ended with status {rc}: nothing written", file=sys.stderr)
        return rc
    res = json.load(open(tmp))
    os.remove(tmp)
    res["commit"] = commit
    json.dump(res, open(a.out, "w"), indent=1)
    md = os.path.splitext(a.out)[0] + ".md"
    with open(md, "w") as f:
        f.write(markdown(res, commit, os.path.basename(a.out)))
    print(open(md).read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
