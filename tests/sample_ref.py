"""Plain-numpy reference of every device sampling decision -- TEST INFRASTRUCTURE ONLY.

Written from the contracts (the comments above block_sample_topk, TalkerSampleArgs, CpArgmaxArgs and SlotParams in
csrc/q3_kernels.h and csrc/q3_sample.hip; oracle/frontend.py's restatement of the reference servers), not from the kernels' code.

The draw is a counter-based integer hash and a decision is a pure function of (logits, state, parameters, u), so the
device is graded exactly: processed logits, state and gathered rows bit for bit; a stochastic pick against the SET of
picks that fp32 round-off of the device's serial sums can reach (one element, except where a comparison falls inside
the error bound gamma, see acceptable_picks).

tests/test_sample_reference.py pins this file against oracle/frontend.py and hand-worked values.
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
RING = 32          # ring of emitted code_0 per row
WINDOW = 30        # the repetition penalty looks at the last 30 of them
GREEDY_T = np.float32(1e-6)
NORM_PRE = 0.0625  # xh = fp16((h * gamma) * NORM_PRE)


def uniform01(seed: int, row: int, frame: int, group: int) -> float:
    """splitmix64 finaliser over seed + golden * (1 + row + frame * 2^20 + group * 2^44); the top 24 bits as [0, 1)."""
    ctr = (1 + int(row) + (int(frame) << 20) + (int(group) << 44)) & M64
    z = (int(seed) + 0x9E3779B97F4A7C15 * ctr) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 40) / 2.0 ** 24


def is_greedy(temperature) -> bool:
    """temperature <= 1e-6 (as float32, the device's type) is the arg-max limit."""
    return not (np.float32(temperature) > GREEDY_T)


def nan_as_inf(l):
    l = np.array(l, dtype=np.float32, copy=True)
    l[np.isnan(l)] = np.inf
    return l


def window_ids(past, n_past):
    """The last min(n_past, 30) emitted ids of a 32-entry ring whose next write goes to slot n_past % 32."""
    return [int(past[(n_past - 1 - i) % RING]) for i in range(min(int(n_past), WINDOW))]


def process_talker(logits, past, n_past, n_text, audio_vocab=2048, eos=2150, ignore_eos=False, rep_penalty=1.2):
    """llamacpp_talker_server.py:167-189 in np.float32, operation for operation: mask, adaptive EOS boost, repetition
    penalty, in that order.  -> (processed logits f32, forced) with forced = progress > 2 (the caller honours
    ignore_eos).  NaN orders as +inf (numpy's arg-max lets a NaN win)."""
    l = nan_as_inf(logits)
    ids = np.arange(len(l))
    l[(ids >= audio_vocab) & (ids != eos)] = np.float32(-1e10)
    forced = False
    if ignore_eos:
        l[eos] = np.float32(-1e10)
    if n_text > 0:
        progress = int(n_past) / (int(n_text) * 3)            # python floats: doubles
        if progress > 0.8 and not ignore_eos:
            boost = min((progress - 0.8) / 0.7, 1.0) * 15.0
            l[eos] = l[eos] + np.float32(boost)               # numpy >= 2 adds the python float as a float32
        forced = progress > 2.0
    pen = np.float32(rep_penalty)
    for t in set(window_ids(past, n_past)):
        if 0 <= t < len(l):
            l[t] = l[t] / pen if l[t] > 0 else l[t] * pen
    return l, forced


def first_argmax(l) -> int:
    """Arg-max with the lowest index on ties, NaN as +inf; 0 when nothing is above -inf."""
    return int(np.argmax(nan_as_inf(l)))


def kept_order(l, top_k):
    """Indices the sampler keeps, in its order: descending key, ASCENDING index on ties (the device's documented rule;
    oracle/frontend.sample_talker's argsort breaks ties the other way -- the device's rule is the one under test),
    the first top_k of them (<= 0 or > n: all), entries at -inf never."""
    key = nan_as_inf(l).astype(np.float64)
    n = len(key)
    k_eff = n if (top_k <= 0 or top_k > n) else int(top_k)
    order = np.lexsort((np.arange(n), -key))[:k_eff]
    return order[key[order] > -np.inf], key


def acceptable_picks(l, top_k, temperature, top_p, u) -> set:
    """Every index a correct fp32 implementation may draw from processed logits l with the uniform u.

    float64: weights exp((l - max) / max(T, 1e-6)) over kept_order; the top-p prefix searchsorted(cumsum, top_p) + 1
    (only for 0 < top_p < 1); inverse CDF = the first k with u * sum < C[k].  A top entry that is not finite is
    returned without a draw; nothing above -inf: index 0.

    The device accumulates in fp32, serially, on one thread.  Two serial fp32 sums of m terms plus 4 ulp for expf and
    the divide are off by at most gamma(m) = (m + 4) * 2^-23 relative to the sum, so a comparison (C[k] >= top_p * S,
    u * S < C[k]) within gamma * S of equality may fall either way: both outcomes are accepted there.  Everywhere else
    the set has one element."""
    order, key = kept_order(l, top_k)
    if len(order) == 0:
        return {0}
    top = key[order[0]]
    if not np.isfinite(top):
        return {int(order[0])}
    T = max(float(np.float32(temperature)), 1e-6)
    w = np.exp((key[order] - top) / T)
    C = np.cumsum(w)
    nk = len(order)
    S = C[-1]
    keeps = [nk]
    top_p = float(np.float32(top_p))
    if 0.0 < top_p < 1.0:
        g = (nk + 4) * 2.0 ** -23 * S
        lo = int(np.argmax(C >= top_p * S - g))                       # exists: C[-1] = S
        above = C > top_p * S + g
        hi = int(np.argmax(above)) if above.any() else nk - 1
        keeps = list(range(lo + 1, hi + 2))
    picks = set()
    for keep in keeps:
        S2 = C[keep - 1]
        g = (keep + 4) * 2.0 ** -23 * S2
        t = u * S2
        lo = int(np.argmax(C[:keep] >= t - g))                        # exists: u < 1
        above = C[:keep] > t + g
        hi = int(np.argmax(above)) if above.any() else keep - 1
        picks.update(int(i) for i in order[lo:hi + 1])
    return picks


def kept_exact(l, top_k, temperature, top_p):
    """The kept entries in sampling order and their probabilities, in float64 without an error band (what
    acceptable_picks draws from wherever nothing is ambiguous).  For rows with a finite top entry."""
    order, key = kept_order(l, top_k)
    w = np.exp((key[order] - key[order[0]]) / max(float(np.float32(temperature)), 1e-6))
    top_p = float(np.float32(top_p))
    if 0.0 < top_p < 1.0:
        keep = int(np.searchsorted(np.cumsum(w / w.sum()), top_p)) + 1
        order, w = order[:keep], w[:keep]
    return order, w / w.sum()


def pick_set(l, temperature, top_k, top_p, u) -> set:
    return {first_argmax(l)} if is_greedy(temperature) else acceptable_picks(l, top_k, temperature, top_p, u)


# ---- parameters of a row: the launch's scalars, or the row's SlotParams entry ------------------------------------
def _row_params(cfg, r, talker):
    slots = cfg.get("slots")
    if slots is not None:
        s = slots[r]
        return dict(temperature=s["t_temp"] if talker else s["c_temp"], top_k=s["t_top_k"] if talker else s["c_top_k"],
                    top_p=s["t_top_p"], max_frames=s["max_frames"], seed=s["seed"], row_key=0 if s["no_row"] else r)
    sp = cfg.get("seed_ptr")
    return dict(temperature=cfg.get("temperature", 0.0), top_k=cfg.get("top_k", 50), top_p=cfg.get("top_p", 0.95),
                max_frames=cfg.get("max_frames", 0), seed=int(sp[r]) if sp is not None else cfg.get("seed", 0), row_key=r)


# ---- talker: decision + state transition -------------------------------------------------------------------------
def slot_flags(cfg, r) -> int:
    """SlotParams::flags of row r (per-slot mode only): bit 0 a text slot, bit 1 its EOS is masked."""
    slots = cfg.get("slots")
    return int(slots[r].get("flags", 0)) if slots is not None else 0


def talker_held(st, cfg, r) -> bool:
    """TalkerSampleArgs (csrc/q3_kernels.h): with text_avail given, in per-slot mode, a row is held in this step when
    its slot is a text slot whose text has not ended (flags 3), the row has not ended, and 1 <= n_past < its budget
    while n_past >= text_avail[r]."""
    ta = cfg.get("text_avail")
    if ta is None or cfg.get("slots") is None:
        return False
    n_past = int(st["n_past"][r])
    return (slot_flags(cfg, r) & 3) == 3 and not st["done"][r] and 1 <= n_past < cfg["slots"][r]["max_frames"] and \
        n_past >= int(ta[r])


def talker_held_after(st, cfg):
    """held[] after the launch: 1 on a held row, 0 on every other row of the launch, rows outside it as they were;
    without text_avail nothing is written."""
    held = np.array(st["held"], copy=True)
    if cfg.get("text_avail") is not None:
        for r in range(cfg["row0"], cfg["row0"] + cfg["R"]):
            held[r] = int(talker_held(st, cfg, r))
    return held


def talker_sets(logits, st, cfg):
    """-> {row: (set of acceptable decisions, processed logits)} for rows row0 .. row0 + R - 1.  A decision is the id
    after the forced-EOS rule (progress > 2 and not ignore_eos: EOS whatever was drawn).  A slot whose EOS is masked
    (flags & 2) is a row under ignore_eos: EOS at -1e10, no boost, no forced EOS.  A held row (talker_held) decides
    nothing and has no entry."""
    out = {}
    for r in range(cfg["row0"], cfg["row0"] + cfg["R"]):
        if talker_held(st, cfg, r):
            continue
        p = _row_params(cfg, r, True)
        ign = bool(cfg.get("ignore_eos", False)) or bool(slot_flags(cfg, r) & 2)
        l, forced = process_talker(logits[r], st["past"][r], int(st["n_past"][r]), int(st["n_text"][r]),
                                   cfg["audio_vocab"], cfg["eos"], ign, cfg.get("rep_penalty", 1.2))
        if forced and not ign:
            s = {cfg["eos"]}
        else:
            u = uniform01(p["seed"], p["row_key"], int(st["n_frames"][r]), 0)
            s = pick_set(l, p["temperature"], p["top_k"], p["top_p"], u)
        out[r] = (s, l)
    return out


def talker_apply_row(st, cfg, r, code):
    """State of row r after the launch decided `code`, in place (integers only).

    The row ends (done = 1, code_0 = -1) when it was done already, on EOS, on an id >= audio_vocab, or once n_past
    reached the frame budget; a frame at or beyond frame_cap is not recorded and ends the row too.  Otherwise code_0
    is recorded, the ring takes the id the stream continues with (the forced one under teacher forcing), and pos is
    the position of the talker step that follows.  The frame counter counts every launch, except that in per-slot mode
    an ended row's counter stops at frame_cap + 1."""
    p = _row_params(cfg, r, True)
    cap, npast, f = cfg["frame_cap"], int(st["n_past"][r]), int(st["n_frames"][r])
    fin = bool(st["done"][r]) or code == cfg["eos"] or code >= cfg["audio_vocab"] or \
        (p["max_frames"] > 0 and npast >= p["max_frames"])
    if cfg.get("slots") is None or not fin or f <= cap:
        st["n_frames"][r] = f + 1
    keep = f < cap
    if fin or not keep:
        st["done"][r] = 1
        if keep:
            st["codes"][f, r, 0] = -1
        return
    used = code
    forced = cfg.get("forced")
    if forced is not None and forced[f, r, 0] >= 0:
        used = int(forced[f, r, 0])
    st["codes"][f, r, 0] = code
    st["past"][r, npast % RING] = used
    st["n_past"][r] = npast + 1
    st["pos"][r] = int(st["pos0"][r]) + npast


def copy_state(st):
    return {k: np.array(v, copy=True) for k, v in st.items()}


# ---- code predictor: decision + state transition -----------------------------------------------------------------
def cp_frame(n_frames_r, frame_cap):
    """-> (frame the row's codes are read from, recorded?): frame n_frames - 1 (n_frames = 0 clamps to 0); a frame
    beyond frame_cap is not recorded and reads the last one."""
    f = max(int(n_frames_r) - 1, 0)
    return (f, True) if f < frame_cap else (frame_cap - 1, False)


def cp_held(cfg, r) -> bool:
    """CpArgmaxArgs::held: per-slot mode, held[r] != 0."""
    held = cfg.get("held")
    return held is not None and cfg.get("slots") is not None and int(held[r]) != 0


def cp_sets(logits, n_frames, cfg):
    """-> {row: set of acceptable decisions}.  No top-p; the draw key's group is 1 + group, its frame n_frames[r].
    A held row decides nothing and has no entry."""
    out = {}
    for r in range(cfg["row0"], cfg["row0"] + cfg["R"]):
        if cp_held(cfg, r):
            continue
        p = _row_params(cfg, r, False)
        u = uniform01(p["seed"], p["row_key"], int(n_frames[r]), 1 + cfg["group"])
        out[r] = pick_set(logits[r], p["temperature"], p["top_k"], 0.0, u)
    return out


def cp_apply_row(codes, n_frames, cfg, r, code):
    """Records the decision in column group + 1 (in place) and returns the id the stream continues with: the forced
    one when teacher forcing names one for a recorded frame.  A held row (cp_held; `code` is ignored) stores nothing
    and continues with the id its frame records in that column, 0 when that is no id of the vocabulary; teacher
    forcing overrides afterwards as for any row."""
    f, keep = cp_frame(n_frames[r], cfg["frame_cap"])
    used = code
    if cp_held(cfg, r):
        used = int(codes[f, r, 1 + cfg["group"]])
        if not 0 <= used < cfg["V"]:
            used = 0
    elif keep:
        codes[f, r, 1 + cfg["group"]] = code
    if keep:
        forced = cfg.get("forced")
        if forced is not None and forced[f, r, 1 + cfg["group"]] >= 0:
            used = int(forced[f, r, 1 + cfg["group"]])
    return used


# ---- gather / feedback epilogue ----------------------------------------------------------------------------------
def gather_row(table, tok):
    """table[tok], zeros when tok is out of range or negative."""
    if 0 <= tok < table.shape[0]:
        return np.array(table[tok], dtype=np.float32, copy=True)
    return np.zeros(table.shape[1], np.float32)


def feedback_row(codes16, talker_emb, cp_tables, pad):
    """tts_client.py:199-208: the talker row of code_0, += row of table g for g = 0 .. 14 in order, += pad; sequential
    np.float32 adds, so the result is bit-defined.  Ids out of range or negative embed as zeros."""
    buf = gather_row(talker_emb, int(codes16[0]))
    for g, tab in enumerate(cp_tables):
        t = int(codes16[1 + g])
        if 0 <= t < tab.shape[0]:
            buf += tab[t]
    if pad is not None:
        buf += pad
    return buf


def feedback_last(pad, text_rows, text_avail, n_frames_r):
    """The last addend of the feedback sum of a row whose frame counter is n_frames_r (CpArgmaxArgs::text_rows): row
    n_frames_r - 1 of the slot's text_rows [text_cap][H] while that is a frame (>= 0) below text_avail, else pad (which
    may be None: nothing is added).  The frame is counted from the slot's start and is not clamped to frame_cap."""
    f = int(n_frames_r) - 1
    if text_rows is not None and 0 <= f < int(text_avail):
        return text_rows[f]
    return pad


def cp_feedback_codes(codes, n_frames, cfg, r, used):
    """The 16 ids the feedback sum of row r embeds: its frame's codes with this launch's group replaced by `used`, and
    teacher-forced ids (>= 0, recorded frames only) in place of the other decisions; a forced code_0 does not revive
    a finished row (code_0 = -1)."""
    f, keep = cp_frame(n_frames[r], cfg["frame_cap"])
    ids = [int(x) for x in codes[f, r]]
    forced = cfg.get("forced") if keep else None
    if forced is not None:
        fz = forced[f, r]
        if fz[0] >= 0 and ids[0] >= 0:
            ids[0] = int(fz[0])
        for g in range(len(ids) - 1):
            if fz[1 + g] >= 0:
                ids[1 + g] = int(fz[1 + g])
    ids[1 + cfg["group"]] = int(used)
    return ids


def ssq_parts(row):
    """What a producer stores beside a residual row: the sum of squares of each block of 16 elements (float64)."""
    x = np.asarray(row, np.float64)
    return (x * x).reshape(-1, 16).sum(axis=1)


def xh_row(row, gamma):
    """The consumer's pre-scaled fp16 GEMM input, (h * gamma) / 16 saturated to the fp16 range (float64)."""
    return np.clip(np.asarray(row, np.float64) * np.asarray(gamma, np.float64) * NORM_PRE, -65504.0, 65504.0)


def fp16_ulp(x):
    """Spacing of fp16 at |x|: 2^(e - 10) with e the exponent of |x|, not below the subnormal spacing 2^-24."""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)
