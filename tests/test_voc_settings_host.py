"""The vocoder's settings store (csrc/q3_voc_settings.h) in a stand-alone program under ThreadSanitizer: the defaults, every
setter's normalisation, and concurrent writers against concurrent readers (tests/voc_settings_host_driver.cpp).  The header is
host-only, so the program is plain C++: nothing of it is loaded into this process."""
import os
import subprocess

from tests.test_native_formats_malformed import rocm_clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen3_tts_axera_russian_amd", "csrc")


def test_settings_store_is_race_free_and_normalises(tmp_path):
    cxx, _ = rocm_clang()
    exe = str(tmp_path / "voc_settings_host_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "voc_settings_host_driver.cpp"), "-o", exe, "-pthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-2000:]
