"""The diagnostic timeline across translation units (csrc/q3_timeline.h / q3_timeline.hip): every kernel file has its own
__device__ copy of the timeline state, and q3t_tl2_begin must reach all of them.  A fresh child process loads the timeline
build (lib/libqwen3tts_tl.so, which build() always makes), records three frames of a two-layer engine and reports the
per-node stamps and kinds: every numbered node is stamped, and the kinds cover a kernel of each of q3_linear.hip (10..16),
q3_attn.hip (30..33), q3_rows.hip (40) and q3_sample.hip (42, 43)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TL = os.path.join(ROOT, "qwen3_tts_axera_russian_amd", "lib", "libqwen3tts_tl.so")
CAP = 400

CHILD = r"""
import ctypes, json
import numpy as np
from tests.util import synthetic_pack
from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd.engine import FrameEngine
CAP, MAXB = %d, 1024
lib = hiplib.load()
lib.q3t_tl2_begin.argtypes = [ctypes.c_int]
lib.q3t_tl2_end.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
lib.q3t_tl2_kinds.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
path = synthetic_pack(2, 2)[0]
rng = np.random.default_rng(72)
prefixes = [(0.05 * rng.standard_normal((n, 1024))).astype(np.float32) for n in (12, 17)]
eng = FrameEngine(path, max_batch=2, n_ctx=64, max_frames=8)
eng.set_pad_embed((0.05 * rng.standard_normal(1024)).astype(np.float32))
assert lib.q3t_tl2_begin(CAP) == 0
eng.start(prefixes, [30, 30], ignore_eos=True, max_frames=8)
assert eng.run(3) == 3
buf = (ctypes.c_ulonglong * (CAP * MAXB * 2))()
n = lib.q3t_tl2_end(buf, CAP)
kinds = (ctypes.c_int * CAP)()
assert lib.q3t_tl2_kinds(kinds, CAP) == 0
eng.destroy()
arr = np.frombuffer(buf, dtype=np.uint64).reshape(CAP, MAXB, 2)
m = min(n, CAP)
ok = [bool(((arr[i, :, 0] != 0) & (arr[i, :, 1] >= arr[i, :, 0])).any()) for i in range(m)]
print("TIMELINE " + json.dumps({"n": int(n), "stamped": ok, "kinds": [int(kinds[i]) for i in range(m)]}), flush=True)
""" % CAP


@pytest.mark.gpu
def test_every_kernel_file_stamps_the_timeline(gpu_lib):
    assert os.path.exists(TL), f"{TL} missing: the build makes the timeline library beside the product one"
    env = dict(os.environ, QWEN3TTS_LIB=TL)
    out = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("TIMELINE ")]
    assert len(line) == 1, out.stdout[-2000:]
    r = json.loads(line[0][len("TIMELINE "):])
    n, kinds = r["n"], set(r["kinds"])
    print(f"{n} numbered nodes, kinds {sorted(kinds)}")
    assert 0 < n <= CAP, n
    unstamped = [i for i, ok in enumerate(r["stamped"]) if not ok]
    assert not unstamped, (unstamped[:20], [r["kinds"][i] for i in unstamped[:20]])
    assert kinds & set(range(10, 17)), kinds      # q3_linear.hip
    assert kinds & set(range(30, 34)), kinds      # q3_attn.hip
    assert {40, 42, 43} <= kinds, kinds           # q3_rows.hip (final norm), q3_sample.hip (talker sample, cp arg-max)
