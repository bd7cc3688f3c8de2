#!/usr/bin/env python3
"""What an audio prompt costs: the PCM front-end beside the encoder, and a "prompt_audio" request beside "prompt_codes".

Synthetic weights of the product's shapes (the 0.6B-architecture talker / code predictor and whole vocoder of
scripts/serve_load.py, the default speech-tokenizer encoder config), one process, three parts:

  encode     GPU ms (enc_last_ms) of enc_encode_pcm on a mono s16 clip of 3 s and 10 s at 16 and 44.1 kHz, against enc_encode of
             the same clip prepared on the host (scipy.signal.resample_poly in float32, the CLI's host path, whose own wall time is
             listed too): --reps calls after two untimed ones.
  first      a streamed "vocoder": "incremental" request of one utterance on a --concurrent --encoder server: wall ms from
             connect to the first audio record with "prompt_codes" (the ids the encoder gives the clip: the path the parent
             commit has), with "prompt_audio" as a miss (a clip the cache has not seen) and as a hit.
  bystander  a long streamed request runs while register-only requests with 10 s clips nobody has sent (every one an encode)
             arrive back to back: the frame loop's wall and device ms per step (FrameEngine.run, q3e_last_run_ms) of the run
             calls that overlap an encode against those that do not.  The Python entry points export one hardware queue, so the
             encode's launches queue between frame steps.

Every figure is a median with min..max beside it.  The driver (no --worker) runs the measurement as a child process under its
own `timeout`, then writes profiles/prompt_audio.json and profiles/prompt_audio.md.

    python scripts/prompt_audio_admit.py --commit $(git rev-parse --short HEAD)
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


def clip(sec, rate, seed):
    r = np.random.default_rng(seed)
    t = np.arange(int(sec * rate)) / rate
    x = 0.2 * np.sin(2 * np.pi * (110 + 7 * seed % 90) * t) + 0.1 * np.sin(2 * np.pi * 640 * t + seed) + 0.02 * r.standard_normal(t.size)
    return (x * 32767).astype(np.int16)


def encode_part(a, enc):
    from qwen3_tts_axera_russian_amd.encode_reference_audio import resample
    rows = []
    for sec in (3.0, 10.0):
        for rate in (16000, 44100):
            x = clip(sec, rate, 1)
            host_ms, dev, ref = [], [], []
            for i in range(a.reps + 2):
                ids = enc.encode_pcm([x], rate)[0]
                if i >= 2:
                    dev.append(enc.last_ms())
            for i in range(a.reps + 2):
                t0 = time.perf_counter()
                y = resample(x.astype(np.float32) / 32768.0, rate, 24000)
                t1 = time.perf_counter()
                ids_host = enc.encode([y])[0]
                if i >= 2:
                    host_ms.append((t1 - t0) * 1e3)
                    ref.append(enc.last_ms())
            rows.append({"seconds": sec, "rate": rate, "frames": int(ids.shape[0]), "enc_encode_pcm_gpu_ms": spread(dev),
                         "enc_encode_gpu_ms": spread(ref), "host_resample_wall_ms": spread(host_ms),
                         "ids_equal_to_host_path": float((ids == ids_host).mean())})
            print(f"[prompt_audio] encode {sec:g} s @ {rate}: pcm {rows[-1]['enc_encode_pcm_gpu_ms']['median']:.3f} ms, "
                  f"enc_encode {rows[-1]['enc_encode_gpu_ms']['median']:.3f} ms", file=sys.stderr, flush=True)
    return rows


def first_audio(sock, **req):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    t0 = time.perf_counter()
    first = None
    for rec in bs.synthesize_batch_stream(sock, vocoder="incremental", **req):
        if rec[0] == "audio" and first is None:
            first = (time.perf_counter() - t0) * 1e3
    return first


def worker(a):
    import serve_load
    from qwen3_tts_axera_russian_amd import batch_server as bs
    from qwen3_tts_axera_russian_amd import weights as W
    main_pack, voc_pack, cfg = serve_load.make_packs(a.cache, a.seed)
    enc_pack = os.path.join(a.cache, "enc_full_s7.q3w")
    if not os.path.exists(enc_pack):
        W.write_synthetic_enc(enc_pack, W.EncConfig(), seed=7)
    sock = os.path.join(a.cache, f"prompt_audio_{os.getpid()}.sock")
    srv = bs.BatchSynthesisServer(main_pack, voc_pack, sock, max_batch=8, n_ctx=a.max_tokens + 64 + 160, max_tokens=a.max_tokens,
                                  temperature=0.0, cp_temperature=0.0, install_signal_handlers=False, concurrent=True,
                                  encoder=enc_pack, prompt_audio_seconds=10.0, prompt_audio_cache=4, max_voices=4)
    out = {"encode": encode_part(a, srv.encoder)}
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(600):
        if os.path.exists(sock) and srv.sched is not None:
            break
        time.sleep(0.05)
    try:
        ids = serve_load.texts(1, a.seed, cfg.text_vocab)
        base = dict(token_ids=ids, max_tokens=32)
        held = clip(3.0, 16000, 2)
        codes = srv.encoder.encode_pcm([held], 16000)[0]
        res = {"prompt_codes": [], "prompt_audio_miss": [], "prompt_audio_hit": []}
        for i in range(a.reps + 1):
            got = {"prompt_codes": first_audio(sock, prompt_codes=codes, **base),
                   "prompt_audio_miss": first_audio(sock, prompt_audio=(clip(3.0, 16000, 100 + i), 16000), **base),
                   "prompt_audio_hit": first_audio(sock, prompt_audio=(held, 16000), **base)}
            if i:                                   # (the first round is untimed: it also brings `held` into the cache)
                for k, v in got.items():
                    res[k].append(v)
        out["first_audio_ms"] = {k: spread(v) for k, v in res.items()}
        out["first_audio_ms"]["clip"] = "3 s, 16 kHz mono s16, %d frames" % len(codes)
        print(f"[prompt_audio] first audio: {out['first_audio_ms']}", file=sys.stderr, flush=True)
        # bystander: the frame loop's run calls, and when an encode was in flight
        eng, enc = srv.eng, srv.encoder
        run0, pcm0 = eng.run, enc.encode_pcm
        runs, encodes = [], []

        def run(n):
            t0 = time.perf_counter()
            k = run0(n)
            if k:
                runs.append((t0, time.perf_counter(), k, eng.last_run_ms))
            return k

        def encode_pcm(*args, **kw):
            t0 = time.perf_counter()
            r = pcm0(*args, **kw)
            encodes.append((t0, time.perf_counter()))
            return r
        eng.run, enc.encode_pcm = run, encode_pcm
        done = threading.Event()

        def bystander():
            for _ in bs.synthesize_batch_stream(sock, token_ids=ids, max_tokens=a.max_tokens):
                pass
            done.set()
        for phase in ("alone", "beside"):
            done.clear()
            t = threading.Thread(target=bystander)
            t.start()
            k = 0
            while phase == "beside" and not done.is_set():
                bs.synthesize_batch(sock, texts=[], prompt_audio=(clip(10.0, 44100, 1000 + k), 44100), register_voice="v%d" % (k % 4))
                k += 1
            t.join()
        eng.run, enc.encode_pcm = run0, pcm0
        over = lambda r: any(r[0] < e1 and e0 < r[1] for e0, e1 in encodes)
        groups = {"beside_an_encode": [r for r in runs if over(r)], "no_encode": [r for r in runs if not over(r)]}
        out["bystander"] = {"encodes": len(encodes), "encode_wall_ms": spread([(e1 - e0) * 1e3 for e0, e1 in encodes])}
        for name, rs in groups.items():
            if rs:
                out["bystander"][name] = {"run_calls": len(rs), "wall_ms_per_step": spread([(r[1] - r[0]) * 1e3 / r[2] for r in rs]),
                                          "device_ms_per_step": spread([r[3] / r[2] for r in rs])}
        print(f"[prompt_audio] bystander: {out['bystander']}", file=sys.stderr, flush=True)
    finally:
        srv._running = False
        th.join(timeout=60)
        srv.close()
    json.dump(out, open(a.out, "w"), indent=1)


def markdown(res, commit, name):
    s = lambda d: f"{d['median']:.3f} ({d['min']:.3f}..{d['max']:.3f})"
    lines = [f"# Audio prompts: the PCM front-end and the \"prompt_audio\" request", "",
             f"Produced by `scripts/prompt_audio_admit.py` from commit `{commit}` on one MI355X; the numbers are in `{name}`.  Synthetic",
             "weights of the product's shapes; every figure is a median with min..max of the repeats beside it.  Nothing here is a",
             "target: the tables state what was measured.", "", "## enc_encode_pcm against enc_encode of host-prepared samples (GPU ms)", "",
             "| clip | frames | enc_encode_pcm | enc_encode (24 kHz f32 from the host) | front-end's share | host resample_poly, wall ms |",
             "|---|---:|---:|---:|---:|---:|"]
    for r in res["encode"]:
        d = r["enc_encode_pcm_gpu_ms"]["median"] - r["enc_encode_gpu_ms"]["median"]
        lines.append(f"| {r['seconds']:g} s, {r['rate']} Hz mono s16 | {r['frames']} | {s(r['enc_encode_pcm_gpu_ms'])} | {s(r['enc_encode_gpu_ms'])} | "
                     f"{d:+.3f} | {s(r['host_resample_wall_ms'])} |")
    lines += ["", "The host path's ids are not the device path's where the two resamplers' float32 results differ in a decisive bit: "
              "share of equal ids per row: " + ", ".join(f"{r['ids_equal_to_host_path']:.3f}" for r in res["encode"]) + ".", "",
              "## First audio of a streamed request (wall ms, connect to the first audio record)", "",
              f"One utterance, \"vocoder\": \"incremental\", clip: {res['first_audio_ms']['clip']}.", "",
              "| request | first audio ms |", "|---|---:|"]
    for k in ("prompt_codes", "prompt_audio_miss", "prompt_audio_hit"):
        lines.append(f"| {k} | {s(res['first_audio_ms'][k])} |")
    b = res["bystander"]
    lines += ["", "## A bystander's frame step while clips are encoded", "",
              f"{b['encodes']} encodes of 10 s 44.1 kHz clips (wall ms each: {s(b['encode_wall_ms'])}) back to back beside one streamed request.", "",
              "| run calls of the frame loop | calls | wall ms / step | device ms / step |", "|---|---:|---:|---:|"]
    for k in ("no_encode", "beside_an_encode"):
        if k in b:
            lines.append(f"| {k} | {b[k]['run_calls']} | {s(b[k]['wall_ms_per_step'])} | {s(b[k]['device_ms_per_step'])} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--max_tokens", type=int, default=160)
    ap.add_argument("--cache", default=os.environ.get("Q3_BENCH_CACHE", "/tmp/q3_bench_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_audio.json"))
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
        print(f"[prompt_audio] the measurement ended with status {rc}: nothing written", file=sys.stderr)
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
