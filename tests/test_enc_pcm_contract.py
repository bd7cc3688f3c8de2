"""The PCM front-end's ABI without a GPU: include/qwen3tts_enc_pcm.h declares enc_pcm_frames and enc_encode_pcm, qwen3tts_enc.h
includes it, the product library exports both (and the hook enc_debug_pcm beside enc_debug_run), hiplib declares them, and the
host arithmetic (csrc/q3_enc_pcm_host.h) names no HIP header: a CPU driver compiles it alone.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_exports():
    from qwen3_tts_axera_russian_amd import build
    src = open(os.path.join(ROOT, "include", "qwen3tts_enc_pcm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(enc_[a-z0-9_]+)\s*\(", code))) == ["enc_encode_pcm", "enc_pcm_frames"]
    assert re.search(r"#define\s+ENC_PCM_S16\s+0\b", code) and re.search(r"#define\s+ENC_PCM_F32\s+1\b", code)
    assert '#include "qwen3tts_enc_pcm.h"' in open(os.path.join(ROOT, "include", "qwen3tts_enc.h")).read()
    lib = ctypes.CDLL(build.build())
    for name in ("enc_encode_pcm", "enc_pcm_frames", "enc_debug_pcm"):
        assert hasattr(lib, name), name
    lib.enc_pcm_frames.restype = ctypes.c_int
    lib.enc_pcm_frames.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert lib.enc_pcm_frames(None, 100, 16000) < 0          # no handle: refused, no device touched


def test_hiplib_declares_them():
    from qwen3_tts_axera_russian_amd import hiplib
    lib = hiplib.load()
    assert lib.enc_encode_pcm.restype is ctypes.c_int and len(lib.enc_encode_pcm.argtypes) == 10
    assert len(lib.enc_pcm_frames.argtypes) == 3 and len(lib.enc_debug_pcm.argtypes) == 10


def test_the_host_header_stands_alone():
    src = open(os.path.join(ROOT, "qwen3_tts_axera_russian_amd", "csrc", "q3_enc_pcm_host.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
    assert includes and all(i in ("cmath", "cstdint", "cstdio", "vector") for i in includes), includes
    assert "hip" not in re.sub(r"//.*", "", src).lower()
