"""What the streaming encode (enc_stream_*, include/qwen3tts_enc_stream.h) rests on, checked without a GPU.

1. The hand-out rule is an identity of the table: every op is causal, so the first floor(n / hop) frames of the encode of
   clip[:n] are those of the whole clip (tests/enc_ref.py on both cases of tests/golden/mimi_encode_golden.npz).  This pins
   the replicate-padded downsample's left edge too: a prefix sees the same first column.
2. The host arithmetic of a push (csrc/q3_enc.h enc_stream_plan, through the test library; no device call) against a
   column-by-column brute force, for every total in 0..3 hop at both cases' ratios.
3. The built library exports every enc_stream_* symbol the header declares, and no test hook."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import weights as W
from tests import enc_common as C
from tests.enc_ref import enc_reference, rvq_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mimi_encode_golden.npz")
HEADER = os.path.join(ROOT, "include", "qwen3tts_enc_stream.h")
EMB_TOL = 1e-5        # tests/test_mimi_encode_golden.py's bound on the embedding
GAP_TOL = 1e-4        # a float64 near-tie (tests/test_gpu_encoder.py's rule for a frame that parts from the fixture)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def case_table(gold, name):
    keys = json.loads(bytes(gold[f"{name}.keys"]).decode())
    state = C.seeded_state(C.CASES[name]["seed"], [(k, tuple(s)) for k, s in keys])
    assert C.digest(state) == bytes(gold[f"{name}.sha"]).decode()
    return W.state_to_enc(state, json.loads(bytes(gold[f"{name}.config"]).decode()), 16)


def levels(ec):
    """(taps, stride) of the strided ops, in order"""
    return [(int(r[3]), int(r[4])) for r in W.enc_program(ec)[0] if r[0] == W.EOP_CONV_S]


@pytest.mark.parametrize("name", list(C.CASES))
def test_prefix_frames_are_the_whole_clips(gold, name):
    case = C.CASES[name]
    ec, t, _ = case_table(gold, name)
    hop = W.enc_hop(ec)
    prog = np.asarray(t["enc.program"])
    emb_ops = dict(W.enc_program(ec)[2])["embedding"]
    N = max(case["lengths"])
    clip = C.seeded_clip(case["seed"], N)
    whole_emb, _ = enc_reference(t, clip, emb_ops)
    whole_codes, _ = enc_reference(t, clip)
    proj = np.asarray(t[f"enc.op{len(prog) - 2}.weight"], np.float64)[:, :, 0]
    books = np.asarray(t[f"enc.op{len(prog) - 1}.codebook"], np.float64)
    _, gap, _ = rvq_encode(proj @ whole_emb.astype(np.float64), books, int(prog[-1][6]))
    scale = max(1.0, float(np.abs(whole_emb).max()))
    assert ec.window < whole_emb.shape[1] * ec.ds_stride        # the clip crosses the attention window
    for n in (hop, hop + 1, 2 * hop - 1, 3 * hop + 7, 5 * hop + hop // 2, (N // hop) * hop, N - 1):
        f = n // hop
        assert 1 <= f <= N // hop
        emb, _ = enc_reference(t, clip[:n], emb_ops)
        codes, _ = enc_reference(t, clip[:n])
        assert codes.shape[0] == W.enc_frames(ec, n) >= f
        err = float(np.abs(emb[:, :f] - whole_emb[:, :f]).max())
        assert err <= EMB_TOL * scale, f"{name} n={n}: prefix embedding off by {err:.2e}"
        diff = codes[:f] != whole_codes[:f]
        for fr in np.nonzero(diff.any(1))[0]:
            q = int(np.argmax(diff[fr]))
            assert gap[fr, q] < GAP_TOL, f"{name} n={n} frame {fr} group {q}: differs and is not a near-tie"


def brute(lv, total_max):
    """Column by column: per total, the columns every level has taken and every strided op has produced while the stream runs."""
    nl = len(lv)
    T, D = [0] * (nl + 1), [0] * nl
    out = [(list(T), list(D))]
    for _ in range(total_max):
        T[0] += 1
        for l, (k, s) in enumerate(lv):
            while (D[l] + 1) * s <= T[l]:     # output u reads inputs below (u + 1) * s
                D[l] += 1
                T[l + 1] += 1
        out.append((list(T), list(D)))
    return out


def brute_finish(lv, T, D):
    """the finish: every level pads its leftover columns into one more output"""
    T, D = list(T), list(D)
    for l, (k, s) in enumerate(lv):
        if T[l] > D[l] * s:
            D[l] += 1
            T[l + 1] += 1
        assert T[l] <= D[l] * s
    return T


@pytest.mark.parametrize("name", list(C.CASES))
def test_level_arithmetic_against_brute_force(gold, name):
    from qwen3_tts_axera_russian_amd import build, hiplib
    build.build()
    tl = hiplib.load_test()
    ec = W.enc_config_from_mimi(json.loads(bytes(gold[f"{name}.config"]).decode()), 16)
    lv = levels(ec)
    nl, hop = len(lv), W.enc_hop(ec)
    ks = np.array([k for k, _ in lv], np.int32)
    ss = np.array([s for _, s in lv], np.int32)
    pushes = sorted({0, 1, hop - 1, hop, hop + 1, 2 * hop + 3})
    sim = brute(lv, 3 * hop + max(pushes))
    n_in = (ctypes.c_longlong * (nl + 1))()
    bc = (ctypes.c_longlong * (nl + 1))()
    carry = (ctypes.c_longlong * nl)()
    step = 1 if hop <= 64 else 7          # (every total at the small ratio; a comb of them + the frame edges at hop 1920)
    totals = sorted(set(range(0, 3 * hop + 1, step)) | {h * hop + d for h in range(4) for d in (-1, 0, 1) if 0 <= h * hop + d <= 3 * hop})
    for before in totals:
        T0, D0 = sim[before]
        for n_new in pushes:
            for fin in (0, 1):
                assert tl.q3t_enc_stream_plan(hiplib.iptr(ks), hiplib.iptr(ss), nl, before, n_new, fin, n_in, bc, carry) == 0
                T1, D1 = sim[before + n_new]
                after = brute_finish(lv, T1, D1) if fin else T1
                assert list(bc) == T0, (before, n_new, fin)
                assert list(n_in) == [a - b for a, b in zip(after, T0)], (before, n_new, fin)
                # what a strided op holds: inputs from its next output's left context to the last one it was given
                assert list(carry) == [T0[l] - D0[l] * s + (k - s) for l, (k, s) in enumerate(lv)], (before, n_new, fin)
                assert after[nl] == (W.enc_frames(ec, before + n_new) if fin and before + n_new else (before + n_new) // hop if not fin else 0)


def declared():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(enc_stream_[a-z0-9_]+)\s*\(", code)))


def test_header_symbols_are_exported_and_no_hook_is():
    from qwen3_tts_axera_russian_amd import LIB_PATH, build
    lib = ctypes.CDLL(build.build())
    names = declared()
    assert names == ["enc_stream_create", "enc_stream_device_bytes", "enc_stream_free", "enc_stream_last_launches",
                     "enc_stream_last_ms", "enc_stream_push", "enc_stream_push_max_frames", "enc_stream_reset",
                     "enc_stream_state_bytes"], names
    assert not [n for n in names if not hasattr(lib, n)]
    assert '#include "qwen3tts_enc_stream.h"' in open(os.path.join(ROOT, "include", "qwen3tts_enc.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH], text=True)
    prod = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [n for n in prod if n.startswith("q3t_")]
    assert {"enc_stream_conv_in_kernel", "enc_stream_unfold_kernel"} <= set(build.NO_SPILL)
    # every signature hiplib declares for the stream is one the header declares
    from qwen3_tts_axera_russian_amd import hiplib
    h = hiplib.load()
    assert all(getattr(h, n).argtypes is not None for n in names)
