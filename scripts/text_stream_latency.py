#!/usr/bin/env python3
"""Time to first audio when the text arrives token by token: a "text_stream" request against waiting for the whole text.

One text of --tokens token ids becomes available at a fixed rate (--rate tokens/s, e.g. a language model writing it), the
first token at t0.  Two clients of one in-process batch_server --concurrent (scripts/serve_load.py's packs: synthetic
Qwen3-TTS-0.6B talker and code predictor, a 4096-entry text table, bench.py's whole vocoder; --tiny: the 2-layer packs of the
tests), alternating, --repeats times after one untimed pass of each:

  streamed  a "text_stream" request goes out at t0 with the first token; token i follows as a text record at t0 + i / rate,
            then the end-of-text record (batch_server.synthesize_text_stream);
  whole     the client waits until the last token exists (t0 + (tokens - 1) / rate) and sends an ordinary streamed request.

Both greedy, streamed audio with --vocoder (default incremental: audio from the first check on).  Reported per leg: time from
t0 to the first audio record and to the end of the reply (ms), frames; for the streamed leg also the checks that ran no frame
because the slot waited for text (the frame loop is faster than the text, so it starves between tokens -- and with it every
other slot of the batch: DESIGN.md section 11).

    python scripts/text_stream_latency.py --out profiles/text_stream_latency.json

--bystander: what a text client that PAUSES costs another request.  One ordinary streamed request (the bystander, --tokens
token ids, whole text) starts together with one text-stream client whose tokens come at --rate but which stops for
--pause_ms after every --pause_every tokens (a language model that stalls); one server without and one with --text_hold
(batch_server; q3e_text_hold), --repeats times each after one untimed pass.  Reported per server: the bystander's time to
its last audio record and the longest gap between two of its audio records, the text client's time to its first audio
record, the frame steps text slots were held for and the checks that ran no frame.  Held steps are not free: a held row
still computes, so the frame loop runs steps that emit nothing for it.

    python scripts/text_stream_latency.py --bystander --out profiles/text_hold_bystander.json

--voice DIR (as encode_reference_audio --output_dir writes it) or --prompt_frames T (T synthetic prompt frames): streamed
text in a cloned voice.  One server with --text_voice, three clients alternating, --repeats times after one untimed pass:

  voiced_streamed  the streamed leg above, carrying the codec prompt (a text slot that continues a prompt);
  streamed         the same text stream without a voice;
  voiced_whole     the whole leg above, carrying the codec prompt (an ordinary prompted request once the text is complete).

Reported per leg: time from t0 to the first audio record and to the end of the reply, frames.  No target: the table states
what was measured.  --frame_step FILE (JSON lines of scripts/slot_step_ms.py, labelled "parent" and "change", one line per
process) adds the frame-step comparison to the .md written beside --out.

    python scripts/text_stream_latency.py --prompt_frames 75 --out profiles/text_voice_latency.json

--voice_warm N (with --prompt_frames T): the vocoder's warm-up per voice, cached (batch_server --voice_warm).  The voiced legs
run against a server without the flag and then against one with it, in the same process: "off", "on/miss" (new random prompt
codes every request) and "on/hit" (the prompt of the untimed pass).  Then, on the server's vocoder shape and one stream, the
warm-up pushes of a prompt of --restore_frames frames (summed voc_incr_last_ms) beside voc_incr_last_restore_ms of the restore
that replaces them.  No target: the tables state what was measured.

    python scripts/text_stream_latency.py --prompt_frames 75 --voice_warm 4 --repeats 5 --out profiles/voice_warm.json
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def tiny_packs(cache):
    from qwen3_tts_axera_russian_amd import weights as W
    os.makedirs(cache, exist_ok=True)
    cfg = W.tiny_config(2, 2, text_vocab=512)
    cfg.text_dim = 64
    main, voc = os.path.join(cache, "tsl_tiny_t2c2.q3w"), os.path.join(cache, "tsl_voc_tiny.q3w")
    if not os.path.exists(main):
        W.write_synthetic(main, cfg, seed=1234, parts=("talker", "cp", "text"))
    if not os.path.exists(voc):
        W.write_pack(voc, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    return main, voc, cfg


def one(sock, ids, rate, max_tokens, vocoder, streamed, **prompt):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    t0 = time.perf_counter()

    def pieces():
        for i, t in enumerate(ids):
            time.sleep(max(0.0, t0 + i / rate - time.perf_counter()))
            yield [t]
    if streamed:
        recs = bs.synthesize_text_stream(sock, pieces(), max_tokens=max_tokens, vocoder=vocoder, **prompt)
    else:
        time.sleep(max(0.0, t0 + (len(ids) - 1) / rate - time.perf_counter()))
        recs = bs.synthesize_batch_stream(sock, token_ids=[ids], max_tokens=max_tokens, vocoder=vocoder, **prompt)
    first, frames, samples = None, 0, 0
    for rec in recs:
        if rec[0] == "audio":
            first = first if first is not None else time.perf_counter()
            samples += len(rec[2])
        else:
            frames = rec[2].shape[0]
    return {"first_audio_ms": round(1e3 * (first - t0), 1), "done_ms": round(1e3 * (time.perf_counter() - t0), 1),
            "frames": frames, "samples": samples}


def bystander_pair(sock, ids, a):
    """The bystander and the pausing text client, started together -> their figures."""
    from qwen3_tts_axera_russian_amd import batch_server as bs
    out = {}
    t0 = time.perf_counter()

    def pieces():
        due = t0
        for i, t in enumerate(ids):
            if i:
                due += 1.0 / a.rate + (a.pause_ms / 1e3 if i % a.pause_every == 0 else 0.0)
            time.sleep(max(0.0, due - time.perf_counter()))
            yield [t]

    def text_client():
        first = None
        for rec in bs.synthesize_text_stream(sock, pieces(), max_tokens=a.max_tokens, vocoder=a.vocoder):
            if rec[0] == "audio" and first is None:
                first = time.perf_counter()
        out["text_first_audio_ms"] = round(1e3 * (first - t0), 1)
        out["text_done_ms"] = round(1e3 * (time.perf_counter() - t0), 1)

    th = threading.Thread(target=text_client)
    th.start()
    stamps, frames = [], 0
    for rec in bs.synthesize_batch_stream(sock, token_ids=[ids], max_tokens=a.max_tokens, vocoder=a.vocoder):
        if rec[0] == "audio":
            stamps.append(time.perf_counter())
        else:
            frames = rec[2].shape[0]
    th.join()
    gaps = np.diff(np.array([t0] + stamps))
    out.update({"bystander_last_audio_ms": round(1e3 * (stamps[-1] - t0), 1), "bystander_longest_gap_ms": round(1e3 * float(gaps.max()), 1),
                "bystander_frames": frames, "bystander_audio_records": len(stamps)})
    return out


def bystander(a, main_pack, voc_pack, cfg, ids):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    legs = {}
    for hold in (False, True):
        name = "text_hold" if hold else "default"
        sock = os.path.join(a.cache, f"tsl_{os.getpid()}_{int(hold)}.sock")
        srv = bs.BatchSynthesisServer(main_pack, voc_pack, sock, max_batch=a.max_batch, n_ctx=a.max_tokens + 64, max_tokens=a.max_tokens,
                                      temperature=0.0, cp_temperature=0.0, install_signal_handlers=False, concurrent=True,
                                      text_wait_ms=max(a.text_wait_ms, 4.0 * a.pause_ms), text_hold=hold)
        th = threading.Thread(target=srv.serve, daemon=True)
        th.start()
        while not (os.path.exists(sock) and srv.sched is not None):
            time.sleep(0.05)
        runs = []
        try:
            for rep in range(a.repeats + 1):
                s0, h0, f0 = srv.sched.starved_checks, srv.sched.held_steps, srv.sched.frame_steps
                r = bystander_pair(sock, ids, a)
                r.update({"starved_checks": srv.sched.starved_checks - s0, "held_steps": srv.sched.held_steps - h0,
                          "frame_steps": srv.sched.frame_steps - f0})
                if rep:
                    runs.append(r)
                print(f"[text_stream_latency] bystander {name} {'warm-up' if not rep else rep}: {r}", file=sys.stderr, flush=True)
        finally:
            srv._running = False
            th.join(timeout=60)
            srv.close()
        keys = [k for k in runs[0]]
        legs[name] = {"runs": runs, "median": {k: float(np.median([r[k] for r in runs])) for k in keys}}
    out = {"what": "an ordinary streamed request beside a text-stream client that pauses: without and with --text_hold",
           "packs": "tiny (2 + 2 layers)" if a.tiny else "synthetic Qwen3-TTS-0.6B architecture", "rate_tokens_per_s": a.rate,
           "tokens": a.tokens, "pause_ms": a.pause_ms, "pause_every": a.pause_every, "max_tokens": a.max_tokens, "vocoder": a.vocoder,
           "max_batch": a.max_batch, "repeats": a.repeats, "legs": legs}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def frame_step_table(path):
    """JSON lines of scripts/slot_step_ms.py (one per process, labelled "parent" / "change") -> (summary dict, .md lines)."""
    rows = [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]
    by = {}
    for r in rows:
        by.setdefault(r["label"], []).append(r["ms_per_step_median"])
    out = {k: {"processes": len(v), "ms_per_step_median_of_medians": round(float(np.median(v)), 4), "min": min(v), "max": max(v),
               "medians": v} for k, v in by.items()}
    md = ["## Frame step of an engine with a text reservation", "",
          "`scripts/slot_step_ms.py --batch %d --reserve %d%s`: q3e_last_run_ms per step, every slot an ordinary utterance (no text "
          "slot live), one process per figure, the two libraries alternating in one session; with q3e_text_hold, and without it "
          "(no hold)." %
          (rows[0]["batch"], rows[0]["reserve"], " [--hold]"), "",
          "| library | processes | median of medians (ms/step) | min | max |", "|---|---|---|---|---|"]
    for k, v in out.items():
        md.append("| %s | %d | %.4f | %.4f | %.4f |" % (k, v["processes"], v["ms_per_step_median_of_medians"], v["min"], v["max"]))
    for suffix in sorted({k[len("parent"):] for k in by if k.startswith("parent")}):   # ("", " (no hold)", ..)
        if "change" + suffix not in by:
            continue
        par, chg = out["parent" + suffix], out["change" + suffix]
        spread = par["max"] - par["min"]
        diff = chg["ms_per_step_median_of_medians"] - par["ms_per_step_median_of_medians"]
        chg["parent_spread_ms"], chg["minus_parent_ms"] = round(spread, 4), round(diff, 4)
        md += ["", "parent%s: its own spread over its processes (max - min) is %.4f ms; the change's median differs from the parent's "
               "by %+.4f ms: %s." % (suffix, spread, diff, "inside that spread" if abs(diff) <= spread else
                                     "OUTSIDE that spread -- the sampler reads two more words of the row's SlotParams entry")]
    return out, md


def voiced(a, main_pack, voc_pack, cfg, ids):
    """--voice / --prompt_frames: first audio of a voiced text stream, of the same stream unvoiced, and of the voiced request
    with the whole text up front."""
    from qwen3_tts_axera_russian_amd import batch_server as bs
    head = []
    if a.voice:
        codes, text = bs.load_voice(a.voice)
        codes = np.asarray(codes, np.int32)
        if text:
            print("[text_stream_latency] the voice's text is not used (no tokenizer here): the prompt has no text", file=sys.stderr)
    else:
        codes = np.random.default_rng(a.seed + 1).integers(0, 2048, size=(a.prompt_frames, 16)).astype(np.int32)
    T = len(codes)
    sock = os.path.join(a.cache, f"tsl_{os.getpid()}_v.sock")
    srv = bs.BatchSynthesisServer(main_pack, voc_pack, sock, max_batch=a.max_batch, n_ctx=a.max_tokens + 64 + T, max_tokens=a.max_tokens,
                                  temperature=0.0, cp_temperature=0.0, install_signal_handlers=False, concurrent=True,
                                  text_wait_ms=a.text_wait_ms, text_voice=True)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    while not (os.path.exists(sock) and srv.sched is not None):
        time.sleep(0.05)
    prompt = dict(prompt_codes=codes, prompt_token_ids=head or None)
    plan = {"voiced_streamed": (True, prompt), "streamed": (True, {}), "voiced_whole": (False, prompt)}
    legs = {k: [] for k in plan}
    try:
        for rep in range(a.repeats + 1):
            for leg, (streamed, kw) in plan.items():
                r = one(sock, ids, a.rate, a.max_tokens, a.vocoder, streamed, **kw)
                if rep:
                    legs[leg].append(r)
                print(f"[text_stream_latency] {'warm-up' if not rep else rep} {leg}: {r}", file=sys.stderr, flush=True)
    finally:
        srv._running = False
        th.join(timeout=60)
        srv.close()
    med = lambda leg, k: float(np.median([r[k] for r in legs[leg]]))
    out = {"what": "time from the first text token to the first audio record: a text stream in a cloned voice, the same stream "
                   "without a voice, and the voiced request once the whole text exists",
           "packs": "tiny (2 + 2 layers)" if a.tiny else "synthetic Qwen3-TTS-0.6B architecture", "rate_tokens_per_s": a.rate,
           "tokens": a.tokens, "text_ready_ms": round(1e3 * (a.tokens - 1) / a.rate, 1), "prompt_frames": T,
           "prompt": a.voice or "synthetic", "max_tokens": a.max_tokens, "vocoder": a.vocoder, "max_batch": a.max_batch,
           "check_every": srv.check_every, "repeats": a.repeats, "runs": legs,
           "median": {leg: {k: med(leg, k) for k in ("first_audio_ms", "done_ms", "frames")} for leg in legs}}
    md = ["# Streamed text in a cloned voice: time to first audio", "",
          "`scripts/text_stream_latency.py %s`, one run on one MI355X: %s packs, %d text tokens at %g tokens/s (the whole text exists "
          "after %.0f ms), a codec prompt of %d frames (%s), vocoder %s, %d slots, %d timed repeats after one untimed pass.  Medians; "
          "no target is set." % (" ".join(sys.argv[1:]), out["packs"], a.tokens, a.rate, out["text_ready_ms"], T, out["prompt"], a.vocoder,
                                 a.max_batch, a.repeats), "",
          "| leg | first audio (ms) | reply done (ms) | frames |", "|---|---|---|---|"]
    for leg in plan:
        m = out["median"][leg]
        md.append("| %s | %.1f | %.1f | %d |" % (leg, m["first_audio_ms"], m["done_ms"], m["frames"]))
    md += ["", "voiced_streamed: a \"text_stream\" request with the prompt (--text_voice); streamed: the same without a prompt; "
           "voiced_whole: an ordinary streamed request with the prompt, sent once the last token exists.  The synthetic weights say "
           "nothing about how the audio sounds; the layout is a recollection of the model's in-context mode (DESIGN.md section 11)."
           "  The voiced legs prefill the prompt's frames behind the prefix and, with the incremental vocoder, push them through the utterance's stream before the first generated frame (their samples are dropped): that work is what separates their first audio from the unvoiced stream's.  The legs end at different frame counts because the EOS rules count the prompt's frames and, for voiced_whole, see the text length from the first frame."]
    if a.frame_step:
        out["frame_step"], more = frame_step_table(a.frame_step)
        md += [""] + more
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        with open(os.path.splitext(a.out)[0] + ".md", "w") as f:
            f.write("\n".join(md) + "\n")


def restore_table(a, voc_pack):
    """One stream on the server's vocoder shape: per prompt length T the warm-up pushes (chunk_tokens pieces, summed
    voc_incr_last_ms and launches) beside the one restore launch that replaces them (voc_incr_last_restore_ms)."""
    from qwen3_tts_axera_russian_amd.vocoder import Vocoder
    voc = Vocoder(voc_pack, 64, min(a.max_batch, 32))
    voc.snapshots(1)
    rows = []
    try:
        st = voc.incremental(1, "exact")
        rng = np.random.default_rng(a.seed + 2)
        for T in a.restore_frames:
            codes = rng.integers(0, 2048, size=(T, 16)).astype(np.int64)
            push_ms, restore_ms, launches = [], [], 0
            for rep in range(a.repeats + 1):
                st.reset(0)
                ms, launches = 0.0, 0
                for f in range(0, T, voc.chunk_tokens):
                    st.push([0], [codes[f:f + voc.chunk_tokens]], [False])
                    ms += st.last_ms
                    launches += st.last_launches
                st.save(0, 0)
                st.restore([0], [0])
                if rep:
                    push_ms.append(ms)
                    restore_ms.append(st.last_restore_ms)
            rows.append({"prompt_frames": T, "pushes": -(-T // voc.chunk_tokens), "push_launches": launches,
                         "push_ms": [round(x, 4) for x in push_ms], "restore_ms": [round(x, 4) for x in restore_ms],
                         "push_ms_median": round(float(np.median(push_ms)), 4), "restore_ms_median": round(float(np.median(restore_ms)), 4)})
            print(f"[text_stream_latency] restore table: {rows[-1]}", file=sys.stderr, flush=True)
        state = st.state_bytes
    finally:
        voc.close()
    return {"state_bytes": state, "rows": rows}


def voice_warm(a, main_pack, voc_pack, cfg, ids):
    """--voice_warm N with --prompt_frames T: the voiced legs against one server without the flag and one with it, in one
    session.  With the flag, "miss" requests carry a prompt the server has not seen (new random codes every time), "hit" requests
    the prompt of the untimed pass."""
    from qwen3_tts_axera_russian_amd import batch_server as bs
    T = a.prompt_frames
    rng = np.random.default_rng(a.seed + 1)
    fresh = lambda: rng.integers(0, 2048, size=(T, 16)).astype(np.int32)
    known = fresh()
    plan = {"voiced_streamed": True, "voiced_whole": False}
    legs = {}
    for flag in (0, a.voice_warm):
        sock = os.path.join(a.cache, f"tsl_{os.getpid()}_w{flag}.sock")
        srv = bs.BatchSynthesisServer(main_pack, voc_pack, sock, max_batch=a.max_batch, n_ctx=a.max_tokens + 64 + T, max_tokens=a.max_tokens,
                                      temperature=0.0, cp_temperature=0.0, install_signal_handlers=False, concurrent=True,
                                      text_wait_ms=a.text_wait_ms, text_voice=True, voice_warm=flag)
        th = threading.Thread(target=srv.serve, daemon=True)
        th.start()
        while not (os.path.exists(sock) and srv.sched is not None):
            time.sleep(0.05)
        cases = {"off": lambda: known} if not flag else {"on/miss": fresh, "on/hit": lambda: known}
        try:
            for rep in range(a.repeats + 1):
                for case, codes in cases.items():
                    for leg, streamed in plan.items():
                        h0, m0 = srv.voice_warm_hits, srv.voice_warm_misses
                        r = one(sock, ids, a.rate, a.max_tokens, a.vocoder, streamed, prompt_codes=codes())
                        r["hits"], r["misses"] = srv.voice_warm_hits - h0, srv.voice_warm_misses - m0
                        if rep:
                            legs.setdefault(f"{leg} {case}", []).append(r)
                        print(f"[text_stream_latency] {'warm-up' if not rep else rep} {leg} {case}: {r}", file=sys.stderr, flush=True)
        finally:
            srv._running = False
            th.join(timeout=60)
            srv.close()
    for name, runs in legs.items():      # the legs are what they are called
        want = {"off": (0, 0), "on/miss": (0, 1), "on/hit": (1, 0)}[name.split(" ")[1]]
        assert all((r["hits"], r["misses"]) == want for r in runs), (name, runs)
    med = lambda leg, k: float(np.median([r[k] for r in legs[leg]]))
    table = restore_table(a, voc_pack)
    out = {"what": "time from the first text token to the first audio record of a request that continues a codec prompt, with the "
                   "incremental vocoder: --voice_warm off, on with an unknown prompt (miss), on with a known one (hit); and one "
                   "stream's warm-up pushes beside the restore launch that replaces them",
           "packs": "tiny (2 + 2 layers)" if a.tiny else "synthetic Qwen3-TTS-0.6B architecture", "rate_tokens_per_s": a.rate,
           "tokens": a.tokens, "text_ready_ms": round(1e3 * (a.tokens - 1) / a.rate, 1), "prompt_frames": T, "max_tokens": a.max_tokens,
           "vocoder": a.vocoder, "max_batch": a.max_batch, "voice_warm": a.voice_warm, "repeats": a.repeats, "runs": legs,
           "median": {leg: {k: med(leg, k) for k in ("first_audio_ms", "done_ms", "frames")} for leg in legs}, "restore": table}
    md = ["# Voice warm-up cache: time to first audio, and the restore launch", "",
          "`scripts/text_stream_latency.py %s`, one run on one MI355X: %s packs, %d text tokens at %g tokens/s (the whole text exists "
          "after %.0f ms), a synthetic codec prompt of %d frames, vocoder %s, %d slots, %d timed repeats after one untimed pass, the "
          "server without the flag first and the one with `--voice_warm %d` after it in the same process.  Medians; no target is set."
          % (" ".join(sys.argv[1:]), out["packs"], a.tokens, a.rate, out["text_ready_ms"], T, a.vocoder, a.max_batch, a.repeats,
             a.voice_warm), "",
          "| leg | --voice_warm | first audio (ms) | reply done (ms) | frames |", "|---|---|---|---|---|"]
    for name in legs:
        m = out["median"][name]
        md.append("| %s | %s | %.1f | %.1f | %d |" % (*name.split(" "), m["first_audio_ms"], m["done_ms"], m["frames"]))
    md += ["", "voiced_streamed: a \"text_stream\" request with the prompt (--text_voice), first audio from the first token; "
           "voiced_whole: an ordinary streamed request with the prompt, sent once the last token exists (first audio counts from the "
           "first token all the same).  off: the parent's code path.  on/miss: a prompt the server has not seen (new random codes "
           "every request): the warm-up pushes as before, then a save.  on/hit: the prompt of the untimed pass: no prompt push, one "
           "restore launch.  The prefix cache is off in all of them, so every request still prefills its prompt's rows.", "",
           "## One stream: the warm-up pushes and the restore that replaces them", "",
           "The server's vocoder shape (chunk_tokens 64), exact arithmetic, one stream, state %d B; per prompt length the summed "
           "voc_incr_last_ms of the pushes and voc_incr_last_restore_ms of the restore, medians of %d repeats after one untimed pass "
           "(GPU time between HIP events on the vocoder's stream; the host's share of a push -- staging, one synchronisation per "
           "launch group -- is not in it)." % (table["state_bytes"], a.repeats), "",
           "| prompt frames | pushes | launches | pushes (ms) | restore (ms) |", "|---|---|---|---|---|"]
    for r in table["rows"]:
        md.append("| %d | %d | %d | %.3f | %.4f |" % (r["prompt_frames"], r["pushes"], r["push_launches"], r["push_ms_median"], r["restore_ms_median"]))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        with open(os.path.splitext(a.out)[0] + ".md", "w") as f:
            f.write("\n".join(md) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=50.0, help="text tokens per second")
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--max_tokens", type=int, default=120)
    ap.add_argument("--vocoder", default="incremental", choices=["walk", "incremental"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max_batch", type=int, default=32)
    ap.add_argument("--text_wait_ms", type=float, default=200.0)
    ap.add_argument("--tiny", action="store_true", help="the tests' 2-layer packs instead of the 0.6B architecture")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--cache", default=os.environ.get("Q3_BENCH_CACHE", "/tmp/q3_bench_cache"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--bystander", action="store_true", help="an ordinary request beside a pausing text client, without / with --text_hold")
    ap.add_argument("--pause_ms", type=float, default=150.0, help="--bystander: the text client's pause")
    ap.add_argument("--pause_every", type=int, default=8, help="--bystander: tokens between two pauses")
    ap.add_argument("--voice", default=None, metavar="DIR", help="a codec prompt as encode_reference_audio --output_dir writes it")
    ap.add_argument("--prompt_frames", type=int, default=0, help="instead of --voice: this many synthetic prompt frames")
    ap.add_argument("--frame_step", default=None, metavar="FILE",
                    help="--voice / --prompt_frames: JSON lines of scripts/slot_step_ms.py (labels parent / change) for the .md")
    ap.add_argument("--voice_warm", type=int, default=0,
                    help="--prompt_frames: the voiced legs against a server without the flag and one with --voice_warm N, and the "
                         "restore table")
    ap.add_argument("--restore_frames", type=int, nargs="*", default=[25, 75, 125, 375],
                    help="--voice_warm: prompt lengths of the restore table (profiles/codec_prompt.md's)")
    a = ap.parse_args()
    if a.voice_warm and (a.voice or a.prompt_frames <= 0 or a.vocoder != "incremental"):
        ap.error("--voice_warm measures synthetic prompts with the incremental vocoder: give --prompt_frames T")
    from qwen3_tts_axera_russian_amd import batch_server as bs
    if a.tiny:
        main_pack, voc_pack, cfg = tiny_packs(a.cache)
    else:
        import serve_load
        main_pack, voc_pack, cfg = serve_load.make_packs(a.cache, a.seed)
    ids = np.random.default_rng(a.seed).integers(0, cfg.text_vocab - 8, a.tokens).tolist()
    if a.bystander:
        return bystander(a, main_pack, voc_pack, cfg, ids)
    if a.voice_warm:
        return voice_warm(a, main_pack, voc_pack, cfg, ids)
    if a.voice or a.prompt_frames > 0:
        return voiced(a, main_pack, voc_pack, cfg, ids)
    sock = os.path.join(a.cache, f"tsl_{os.getpid()}.sock")
    srv = bs.BatchSynthesisServer(main_pack, voc_pack, sock, max_batch=a.max_batch, n_ctx=a.max_tokens + 64, max_tokens=a.max_tokens,
                                  temperature=0.0, cp_temperature=0.0, install_signal_handlers=False, concurrent=True,
                                  text_wait_ms=a.text_wait_ms)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    while not (os.path.exists(sock) and srv.sched is not None):
        time.sleep(0.05)
    legs = {"streamed": [], "whole": []}
    try:
        for rep in range(a.repeats + 1):
            for leg in ("streamed", "whole"):
                s0 = srv.sched.starved_checks
                r = one(sock, ids, a.rate, a.max_tokens, a.vocoder, leg == "streamed")
                if leg == "streamed":
                    r["starved_checks"] = srv.sched.starved_checks - s0
                if rep:
                    legs[leg].append(r)
                print(f"[text_stream_latency] {'warm-up' if not rep else rep} {leg}: {r}", file=sys.stderr, flush=True)
    finally:
        srv._running = False
        th.join(timeout=60)
        srv.close()
    med = lambda leg, k: float(np.median([r[k] for r in legs[leg]]))
    out = {"what": "time from the first text token to the first audio record: text streamed into the utterance vs the whole text first",
           "packs": "tiny (2 + 2 layers)" if a.tiny else "synthetic Qwen3-TTS-0.6B architecture", "rate_tokens_per_s": a.rate,
           "tokens": a.tokens, "text_ready_ms": round(1e3 * (a.tokens - 1) / a.rate, 1), "max_tokens": a.max_tokens,
           "vocoder": a.vocoder, "max_batch": a.max_batch, "check_every": srv.check_every, "text_wait_ms": a.text_wait_ms,
           "repeats": a.repeats, "runs": legs,
           "median": {leg: {k: med(leg, k) for k in ("first_audio_ms", "done_ms", "frames")} for leg in legs},
           "median_starved_checks": med("streamed", "starved_checks")}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
