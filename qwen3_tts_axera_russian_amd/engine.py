"""Host side of the fused on-device frame loop (include/qwen3tts_engine.h).

Stands where the reference's client closes the loop over sockets (dual_npu/tts_client.py:144-215);
the per-frame work (talker step, 15-group code predictor, feedback sum) stays on the GPU."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

from . import hiplib


@dataclass(frozen=True)
class SlotParams:
    """One utterance's settings in a per-slot batch (FrameEngine.open / admit; q3e_slot_params).  The draw stream is
    mix(seed, utt): the same utterance with the same seed samples the same codes in any slot."""
    max_frames: int
    temperature: float = 0.0
    top_k: int = 50
    top_p: float = 1.0
    cp_temperature: float = 0.0
    cp_top_k: int = 50
    seed: int = 0
    utt: int = 0
    text_stream: bool = False      # a text slot: its text arrives row by row (FrameEngine.push_text); n_text is ignored
    text_after_prompt: bool = False    # a text slot that may continue a codec prompt (admit(prompts=...)): its text rows
                                       # are counted from its first generated frame; needs text_stream

    def check(self, max_frames):
        """Raises ValueError unless every field is in range for an engine of `max_frames` frames per utterance."""
        for name in ("temperature", "cp_temperature"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
                raise ValueError(f"{name} must be finite and >= 0 (got {v!r})")
        if not (isinstance(self.top_p, (int, float)) and 0 < self.top_p <= 1):
            raise ValueError(f"top_p must be in (0, 1] (got {self.top_p!r})")
        for name in ("max_frames", "top_k", "cp_top_k", "seed", "utt"):
            if isinstance(getattr(self, name), bool) or not isinstance(getattr(self, name), (int, np.integer)):
                raise ValueError(f"{name} must be an integer (got {getattr(self, name)!r})")
        if not 1 <= self.max_frames <= max_frames:
            raise ValueError(f"max_frames must be in 1..{max_frames} (got {self.max_frames})")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"seed must fit in a u64 (got {self.seed})")
        if not 0 <= self.utt < 1 << 31:
            raise ValueError(f"utt must be in 0..2**31-1 (got {self.utt})")
        if not (-(1 << 31) <= self.top_k < 1 << 31 and -(1 << 31) <= self.cp_top_k < 1 << 31):
            raise ValueError("top_k / cp_top_k must fit in an i32")
        if self.text_after_prompt and not self.text_stream:
            raise ValueError("text_after_prompt needs text_stream (a codec prompt under streamed text is a text slot's)")


@dataclass(frozen=True)
class SlotRules:
    """One utterance's sampler rules in a per-slot batch (FrameEngine.rules / admit(rules=...); q3e_slot_rules).  The
    defaults are the reference's constants (llamacpp_talker_server.py:163-206): a default SlotRules changes nothing."""
    rep_penalty: float = 1.2       # >= 1; 1 = none
    rep_window: int = 30           # 1..30 last ids; 0 = every id the utterance has emitted
    eos_boost: float = 15.0        # >= 0: ceiling of the adaptive EOS boost
    eos_force: float = 2.0         # progress above which EOS is forced; 0 = never
    min_frames: int = 0            # generated frames before EOS may be chosen
    cp_top_p: float = 1.0          # (0, 1]: the code predictor's nucleus cut; 1 = none

    def check(self):
        """Raises ValueError unless every field is in the range q3e_admit_ruled accepts."""
        def f32(v):
            # the value as the engine sees it: a float rounds to f32 on its way into q3e_slot_rules (1e39 is inf there,
            # 1e-50 is 0); None for anything that is not a finite number
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                return None
            with np.errstate(over="ignore"):
                v = float(np.float32(v))
            return v if math.isfinite(v) else None
        if not (f32(self.rep_penalty) is not None and f32(self.rep_penalty) >= 1):
            raise ValueError(f"rep_penalty must be finite (as an f32) and >= 1 (got {self.rep_penalty!r})")
        for name in ("eos_boost", "eos_force"):
            v = getattr(self, name)
            if not (f32(v) is not None and f32(v) >= 0):
                raise ValueError(f"{name} must be finite (as an f32) and >= 0 (got {v!r})")
        if not (f32(self.cp_top_p) is not None and 0 < f32(self.cp_top_p) <= 1):
            raise ValueError(f"cp_top_p must be in (0, 1] as an f32 (got {self.cp_top_p!r})")
        for name in ("rep_window", "min_frames"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an integer (got {v!r})")
        if not 0 <= self.rep_window <= 30:
            raise ValueError(f"rep_window must be in 0..30 (got {self.rep_window})")
        if not 0 <= self.min_frames < 1 << 31:
            raise ValueError(f"min_frames must be in 0..2**31-1 (got {self.min_frames})")

    def is_default(self):
        return self == SlotRules()

    def to_c(self):
        return hiplib.SlotRulesC(float(self.rep_penalty), int(self.rep_window), float(self.eos_boost), float(self.eos_force),
                                 int(self.min_frames), float(self.cp_top_p), (ctypes.c_int32 * 2)(0, 0))


class FrameEngine:
    def __init__(self, weights_path, max_batch=32, n_ctx=512, max_frames=256):
        self._lib = hiplib.load()
        self.h = self._lib.q3e_create(str(weights_path).encode(), max_batch, n_ctx, max_frames)
        if not self.h:
            raise RuntimeError(f"q3e_create failed: {weights_path}")
        self.max_batch, self.n_ctx, self.max_frames = max_batch, n_ctx, max_frames
        self.B = 0
        self.frame_steps = 0       # frame steps run() has executed over the engine's life

    def set_sampling(self, talker_temperature=0.0, talker_top_k=50, talker_top_p=0.95, cp_temperature=0.0,
                     cp_top_k=50, seed=0):
        if self._lib.q3e_set_sampling(self.h, float(talker_temperature), int(talker_top_k), float(talker_top_p),
                                      float(cp_temperature), int(cp_top_k), int(seed)) != 0:
            raise RuntimeError("q3e_set_sampling failed")

    def set_chains(self, n):
        if self._lib.q3e_set_chains(self.h, int(n)) != 0:
            raise RuntimeError("q3e_set_chains failed")

    def set_pad_embed(self, pad):
        pad = np.ascontiguousarray(pad, dtype=np.float32).reshape(-1)
        if self._lib.q3e_set_pad_embed(self.h, hiplib.fptr(pad)) != 0:
            raise RuntimeError("q3e_set_pad_embed failed")

    def start(self, prefixes, n_text, ignore_eos=False, max_frames=0):
        """prefixes: list of [n_b, hidden] f32 prefix matrices (llamacpp_talker_server.py:121-161)."""
        n_rows = np.array([p.shape[0] for p in prefixes], np.int32)
        cat = np.ascontiguousarray(np.concatenate(prefixes, axis=0), dtype=np.float32)
        nt = np.ascontiguousarray(n_text, dtype=np.int32)
        self.B = len(prefixes)
        rc = self._lib.q3e_start(self.h, self.B, hiplib.fptr(cat), hiplib.iptr(n_rows), hiplib.iptr(nt),
                                 int(bool(ignore_eos)), int(max_frames))
        if rc != 0:
            raise RuntimeError(f"q3e_start failed: {rc}")

    def set_forced_codes(self, forced):
        """Teacher forcing (after start()): forced[f][B][16] int32, entries < 0 free-running; None = off."""
        if forced is None:
            rc = self._lib.q3e_set_forced_codes(self.h, None, 0)
        else:
            f = np.ascontiguousarray(forced, dtype=np.int32)
            assert f.ndim == 3 and f.shape[1] == self.B and f.shape[2] == 16
            rc = self._lib.q3e_set_forced_codes(self.h, hiplib.iptr(f), f.shape[0])
        if rc != 0:
            raise RuntimeError("q3e_set_forced_codes failed")

    def run(self, n_frames):
        rc = self._lib.q3e_run(self.h, int(n_frames))
        if rc < 0:
            raise RuntimeError(f"q3e_run failed: {rc}")
        self.frame_steps += rc
        return rc

    @property
    def graph_nodes(self):
        """Nodes of the captured frame (q3e_graph_nodes; 0 before the first capture)."""
        return int(self._lib.q3e_graph_nodes(self.h))

    @property
    def last_run_ms(self):
        return float(self._lib.q3e_last_run_ms(self.h))

    @property
    def last_prefill_ms(self):
        return float(self._lib.q3e_last_prefill_ms(self.h))

    @property
    def step_weight_bytes(self):
        return float(self._lib.q3e_step_weight_bytes(self.h))

    def codes(self):
        """-> (codes[frames][B][16] int32, frames emitted per utterance)."""
        out = np.full((self.max_frames, self.B, 16), -1, np.int32)
        per = np.zeros(self.B, np.int32)
        nf = self._lib.q3e_get_codes(self.h, hiplib.iptr(out), self.max_frames, hiplib.iptr(per))
        if nf < 0:
            raise RuntimeError("q3e_get_codes failed")
        return out[:nf], per

    def scores_reserve(self, on=True):
        """Reserve (or release) the per-decision log-probabilities (q3e_scores_reserve; before open()): scores() then
        returns them.  The codes are the same bits with or without.  Raises ValueError when the engine refuses (a per-slot
        batch is open): nothing changes."""
        rc = self._lib.q3e_scores_reserve(self.h, int(bool(on)))
        if rc != 0:
            raise ValueError(f"q3e_scores_reserve refused: {rc}")

    def scores(self):
        """-> (scores[frames][B][16] float32, frames emitted per utterance): beside every id of codes(), the model's
        log-probability at temperature 1 of the id the stream continued with (the forced id under teacher forcing); 0.0
        in the frames of an utterance at or past its count.  Needs scores_reserve()."""
        out = np.zeros((self.max_frames, self.B, 16), np.float32)
        per = np.zeros(self.B, np.int32)
        nf = self._lib.q3e_get_scores(self.h, hiplib.fptr(out), self.max_frames, hiplib.iptr(per))
        if nf < 0:
            raise RuntimeError("q3e_get_scores failed (no scores_reserve()?)")
        return out[:nf], per

    def score(self, prefixes, n_text, codes, ignore_eos=True):
        """Teacher-forced log-likelihood of given ids: starts a batch of the prefixes, forces codes[f][B][16], runs
        len(codes) frames -> scores[len(codes)][B][16] float32 (scores()).  Needs scores_reserve()."""
        forced = np.ascontiguousarray(codes, dtype=np.int32)
        assert forced.ndim == 3 and forced.shape[1] == len(prefixes) and forced.shape[2] == 16
        self.start(prefixes, n_text, ignore_eos=ignore_eos, max_frames=forced.shape[0])
        self.set_forced_codes(forced)
        self.run(forced.shape[0])
        return self.scores()[0]

    def done(self):
        """-> (done[B] bool: the utterance has ended (EOS or its frame budget), frames emitted per utterance)."""
        d = np.zeros(self.B, np.int32)
        per = np.zeros(self.B, np.int32)
        if self._lib.q3e_get_done(self.h, hiplib.iptr(d), hiplib.iptr(per)) != 0:
            raise RuntimeError("q3e_get_done failed")
        return d.astype(bool), per

    def refill(self, slots, prefixes, n_text):
        """Continuous batching: put new utterances into `slots` of the running batch (q3e_refill); the other slots go on
        untouched.  Fetch the codes of a finished utterance before refilling its slot."""
        slots = np.ascontiguousarray(np.asarray(slots, np.int32))
        assert len(slots) == len(prefixes) == len(n_text) and len(slots) > 0
        cat = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32) for p in prefixes], axis=0))
        n_rows = np.array([p.shape[0] for p in prefixes], np.int32)
        nt = np.ascontiguousarray(np.asarray(n_text, np.int32))
        rc = self._lib.q3e_refill(self.h, len(slots), hiplib.iptr(slots), hiplib.fptr(cat), hiplib.iptr(n_rows), hiplib.iptr(nt))
        if rc != 0:
            raise RuntimeError(f"q3e_refill failed: {rc}")

    def generate_queue(self, prefixes, n_text, max_frames, ignore_eos=False, check_every=8, on_done=None, on_frames=None):
        """Continuous batching over a queue of utterances: the first max_batch of them start together; every
        `check_every` frames the finished slots hand over their codes and take the next utterance of the queue
        (q3e_refill), so the frame loop never steps a batch of mostly finished rows.  -> list of int32 [frames][16] in
        queue order.  on_done(index, codes) is called as each utterance finishes (e.g. to hand it to the vocoder).
        on_frames(codes, per, owner, ended) is called at every check, before the finished slots are handed over and
        refilled: codes[f][slot][16] and per[slot] as codes() returns them, owner[slot] = queue index of the utterance in
        the slot (None: the slot is idle), ended = the slots whose utterance has ended at this check (e.g. to stream its
        frames to the vocoder as they come)."""
        n = len(prefixes)
        assert n == len(n_text) and n > 0
        B = min(self.max_batch, n)
        out = [None] * n
        owner = list(range(B))                    # queue index of the utterance in each slot
        nxt = B
        self.start(prefixes[:B], n_text[:B], ignore_eos=ignore_eos, max_frames=max_frames)
        while any(o is not None for o in owner):
            ran = self.run(check_every)
            done, per = self.done()
            # an utterance that used its whole frame budget without an EOS has ended too (q3e_get_done reports it)
            fin = [b for b in range(B) if owner[b] is not None and (done[b] or per[b] >= max_frames)]
            codes = None
            if on_frames is not None:
                codes, _ = self.codes()
                on_frames(codes, per, list(owner), fin)
            if not fin:
                if ran == 0:
                    raise RuntimeError("generate_queue: the engine ran no frame and no utterance finished")
                continue
            if codes is None:
                codes, _ = self.codes()
            for b in fin:
                res = np.ascontiguousarray(codes[:int(per[b]), b, :])
                out[owner[b]] = res
                if on_done is not None:
                    on_done(owner[b], res)
                owner[b] = None
            take = [b for b in fin if nxt + fin.index(b) < n]
            if take:
                idx = [nxt + i for i in range(len(take))]
                self.refill(take, [prefixes[i] for i in idx], [n_text[i] for i in idx])
                for b, i in zip(take, idx):
                    owner[b] = i
                nxt += len(take)
        return out

    def open(self, B=None, ignore_eos=False):
        """Per-slot mode (q3e_open): B (default max_batch) idle slots; utterances come in with admit() and leave when they
        end or with release()."""
        B = self.max_batch if B is None else int(B)
        if self._lib.q3e_open(self.h, B, int(bool(ignore_eos))) != 0:
            raise RuntimeError("q3e_open failed")
        self.B = B

    def prefix_cache(self, n_entries, max_rows=64):
        """Reserve a device pool of `n_entries` prefix entries of up to `max_rows` rows each for admit(keys=...)
        (q3e_prefix_cache; 0 entries releases it).  Drops every entry.  Raises ValueError when the engine refuses."""
        if self._lib.q3e_prefix_cache(self.h, int(n_entries), int(max_rows)) != 0:
            raise ValueError(f"q3e_prefix_cache({n_entries}, {max_rows}) refused")

    def prefix_stats(self):
        """-> dict: hits, misses, stores, evictions, too_long, in_use of the prefix cache (q3e_prefix_stats)."""
        out = np.zeros(6, np.int64)
        if self._lib.q3e_prefix_stats(self.h, out.ctypes.data_as(hiplib.i64p)) != 0:
            raise RuntimeError("q3e_prefix_stats failed")
        return dict(zip(("hits", "misses", "stores", "evictions", "too_long", "in_use"), (int(v) for v in out)))

    def rules(self, on=True):
        """Reserve (or release) the per-slot sampler rules and emitted-id sets (q3e_rules_reserve; before open()): admit()
        then takes rules=.  Raises ValueError when the engine refuses (a per-slot batch is open): nothing changes."""
        rc = self._lib.q3e_rules_reserve(self.h, int(bool(on)))
        if rc != 0:
            raise ValueError(f"q3e_rules_reserve refused: {rc}")

    def admit(self, slots, prefixes, n_text, params, keys=None, prompts=None, rules=None):
        """Per-slot mode: put new utterances into `slots` (q3e_admit), each with its SlotParams (checked here first).
        keys (q3e_admit_keyed): one 16-byte key per utterance, or None for an utterance that is not cached -- a digest of
        everything that determines its prefix rows; an utterance whose key the prefix cache holds takes its KV rows and
        frame-0 state from there instead of a prefill, bit for bit the same.
        prompts (q3e_admit_prompted): one [T][16] int array of codec ids per utterance, or None for an utterance without
        one -- frames the utterance counts as already emitted: they are prefilled behind its prefix, the sampler's history
        starts with them, and codes() / done() / max_frames count the generated frames only.  A key must digest the prompt.
        A text slot takes a prompt only with SlotParams.text_after_prompt; its pushed row i then rides on generated frame i.
        rules (q3e_admit_ruled; after rules()): one SlotRules per utterance, or None for the defaults (checked here first).
        -> None, or with keys the hit flags (bool [n])."""
        slots = np.ascontiguousarray(np.asarray(slots, np.int32))
        assert len(slots) == len(prefixes) == len(n_text) == len(params) and len(slots) > 0
        for p in params:
            p.check(self.max_frames)
        cat = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32) for p in prefixes], axis=0))
        n_rows = np.array([p.shape[0] for p in prefixes], np.int32)
        nt = np.ascontiguousarray(np.asarray(n_text, np.int32))
        arr = (hiplib.SlotParamsC * len(params))(*[
            hiplib.SlotParamsC(int(p.max_frames), float(p.temperature), int(p.top_k), float(p.top_p), float(p.cp_temperature),
                               int(p.cp_top_k), int(p.seed), int(p.utt),
                               (1 if p.text_stream else 0) | (2 if p.text_after_prompt else 0)) for p in params])
        rarr = None
        if rules is not None:
            assert len(rules) == len(slots)
            rules = [SlotRules() if r is None else r for r in rules]
            for r in rules:
                r.check()
            rarr = (hiplib.SlotRulesC * len(rules))(*[r.to_c() for r in rules])
        if keys is None and prompts is None and rarr is None:
            rc = self._lib.q3e_admit(self.h, len(slots), hiplib.iptr(slots), hiplib.fptr(cat), hiplib.iptr(n_rows),
                                     hiplib.iptr(nt), arr)
            if rc != 0:
                raise RuntimeError(f"q3e_admit failed: {rc}")
            return None
        kk = hit = None
        if keys is not None:
            assert len(keys) == len(slots)
            kk = np.zeros((len(slots), 2), np.uint64)
            for u, k in enumerate(keys):
                if k is None:
                    continue
                if not isinstance(k, (bytes, bytearray)) or len(k) != 16:
                    raise ValueError(f"a prefix key is 16 bytes or None (got {k!r})")
                kk[u] = np.frombuffer(bytes(k), "<u8")
            hit = np.zeros(len(slots), np.int32)
        kptr = kk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if kk is not None else None
        hptr = hiplib.iptr(hit) if hit is not None else None
        if prompts is None and rarr is None:
            rc = self._lib.q3e_admit_keyed(self.h, len(slots), hiplib.iptr(slots), hiplib.fptr(cat), hiplib.iptr(n_rows),
                                           hiplib.iptr(nt), arr, kptr, hptr)
            if rc != 0:
                raise RuntimeError(f"q3e_admit_keyed failed: {rc}")
            return hit.astype(bool)
        if prompts is None:
            prompts = [None] * len(slots)
        assert len(prompts) == len(slots)
        pcs = []
        for pr in prompts:
            pr = np.zeros((0, 16), np.int32) if pr is None else np.asarray(pr)
            if pr.ndim != 2 or pr.shape[1] != 16 or not np.issubdtype(pr.dtype, np.integer):
                raise ValueError(f"a codec prompt is an integer array [T][16] or None (got shape {pr.shape}, {pr.dtype})")
            if pr.size and (pr.min() < -(1 << 31) or pr.max() >= 1 << 31):
                raise ValueError("codec prompt ids must fit in an i32")
            pcs.append(pr.astype(np.int32))
        frames = np.array([len(pr) for pr in pcs], np.int32)
        pcat = np.ascontiguousarray(np.concatenate(pcs, axis=0)) if frames.sum() else np.zeros((1, 16), np.int32)
        if rarr is not None:
            rc = self._lib.q3e_admit_ruled(self.h, len(slots), hiplib.iptr(slots), hiplib.fptr(cat), hiplib.iptr(n_rows),
                                           hiplib.iptr(nt), arr, kptr, hptr, hiplib.iptr(pcat), hiplib.iptr(frames), rarr)
            if rc != 0:
                raise RuntimeError(f"q3e_admit_ruled failed: {rc}")
            return None if hit is None else hit.astype(bool)
        rc = self._lib.q3e_admit_prompted(self.h, len(slots), hiplib.iptr(slots), hiplib.fptr(cat), hiplib.iptr(n_rows),
                                          hiplib.iptr(nt), arr, kptr, hptr, hiplib.iptr(pcat), hiplib.iptr(frames))
        if rc != 0:
            raise RuntimeError(f"q3e_admit_prompted failed: {rc}")
        return None if hit is None else hit.astype(bool)

    def reserve_text(self, max_rows):
        """Room for `max_rows` streamed text rows per slot (q3e_text_reserve; before open(); 0 releases it)."""
        if self._lib.q3e_text_reserve(self.h, int(max_rows)) != 0:
            raise RuntimeError(f"q3e_text_reserve({max_rows}) failed")

    def hold_text(self, on=True):
        """Hold a starved text slot inside the frame instead of stalling the batch (q3e_text_hold; after reserve_text(),
        before open()).  run() then steps the other slots on while a live text slot has no row for its next frame, and
        returns 0 only when every live slot is held (or a text slot without a frame has no row yet).  Raises ValueError
        when the engine refuses (no reservation, or a per-slot batch is open): nothing changes."""
        rc = self._lib.q3e_text_hold(self.h, int(bool(on)))
        if rc != 0:
            raise ValueError(f"q3e_text_hold refused: {rc}")

    def held_steps(self):
        """-> int64 [B]: frame steps each slot's utterance was held for since its admission (q3e_text_held)."""
        held = np.zeros(self.B, np.int64)
        if self._lib.q3e_text_held(self.h, held.ctypes.data_as(hiplib.i64p)) != 0:
            raise RuntimeError("q3e_text_held failed")
        return held

    def push_text(self, slot, rows, final=False, n_text=0):
        """Append rows ([n, hidden] f32, n >= 0) to the text of the text slot `slot` (q3e_push_text).  final ends the text:
        the slot's EOS mask is lifted and its text length becomes n_text.  Row i is consumed at the slot's frame i; run()
        never steps a slot past its rows while its text is not final.  Raises ValueError when the engine refuses the
        push (not a live text slot, after the final push, beyond the reservation, a non-finite value): nothing is written."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        rows = rows.reshape(-1, rows.shape[-1]) if rows.size else rows.reshape(0, 1024)
        if rows.shape[1] != 1024:
            raise ValueError(f"text rows are [n, 1024] (got {rows.shape})")
        rc = self._lib.q3e_push_text(self.h, int(slot), hiplib.fptr(rows) if len(rows) else None, len(rows),
                                     int(bool(final)), int(n_text))
        if rc != 0:
            raise ValueError(f"q3e_push_text refused the push to slot {slot}: {rc}")

    def text_state(self):
        """-> (rows pushed per slot, starved[B] bool: the live text slots the next step waits for)."""
        rows = np.zeros(self.B, np.int32)
        starved = np.zeros(self.B, np.int32)
        if self._lib.q3e_text_state(self.h, hiplib.iptr(rows), hiplib.iptr(starved)) != 0:
            raise RuntimeError("q3e_text_state failed")
        return rows, starved.astype(bool)

    def release(self, slots):
        """Per-slot mode: end the utterances in `slots` now (q3e_release; cancellation)."""
        slots = np.ascontiguousarray(np.asarray(slots, np.int32))
        if len(slots) and self._lib.q3e_release(self.h, len(slots), hiplib.iptr(slots)) != 0:
            raise RuntimeError("q3e_release failed")

    def hidden(self):
        out = np.empty((self.B, 1024), np.float32)
        if self._lib.q3e_get_hidden(self.h, hiplib.fptr(out)) != 0:
            raise RuntimeError("q3e_get_hidden failed")
        return out

    def destroy(self):
        if self.h:
            self._lib.q3e_free(self.h)
            self.h = None
