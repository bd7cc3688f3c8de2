"""The one frag_idx of csrc/q3_frag.h (kernels, the C-ABI files and the test hooks share it) as a host compiler builds
it: tests/frag_idx_host_driver.cpp, compiled with g++, against the fragment order restated in tests/text_ref.py from the
layout's text.  34 rows pad to 48, so for every K the 48 padded rows fill [0, 48 K) exactly once.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.text_ref import frag_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 34


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert shutil.which("g++"), "the host form of frag_idx is tested with g++"
    exe = str(tmp_path_factory.mktemp("frag_idx") / "frag_idx_host_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "frag_idx_host_driver.cpp"),
                           "-o", exe])
    return exe


def host_frag_idx(driver, K, rows):
    out = subprocess.run([driver, str(K), str(rows)], capture_output=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return np.frombuffer(out.stdout, np.uint64).astype(np.int64).reshape(rows, K)


@pytest.mark.parametrize("K", [32, 64, 1024])
def test_frag_idx_host_matches_the_layout(driver, K):
    got = host_frag_idx(driver, K, ROWS)
    want = frag_index(np.arange(ROWS)[:, None], np.arange(K)[None, :], K)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("K", [32, 64, 1024])
def test_frag_idx_host_is_a_permutation_of_the_padded_rows(driver, K):
    padded = (ROWS + 15) // 16 * 16
    assert padded == 48
    got = host_frag_idx(driver, K, padded)
    np.testing.assert_array_equal(got[:ROWS], host_frag_idx(driver, K, ROWS))
    np.testing.assert_array_equal(np.sort(got.reshape(-1)), np.arange(padded * K))
