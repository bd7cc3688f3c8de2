"""The code predictor's layer-0 q|k|v table (Model::cp_qkv_tab, DESIGN.md 4 "Fewer nodes").

Positions 2..15 of a code-predictor frame embed a code-predictor token, so layer 0's q|k|v launch of those passes is a
function of (group, token id).  The table holds that launch's output for every token, built at load by the launch itself;
the arg-max kernel copies the row and cp_frame leaves the launch out.  Nothing about the results may change:

  * a table row holds exactly the bits the live launch produces for that token, at every row count (the <= 16-row and the
    17..32-row variants of linear_kernel split K the same way, so ONE table serves every row count of the weight-streaming
    kernel; a row count that takes the tiled GEMM is not served: the engine keeps the launch there);
  * the frame engine and cp_predict give identical outputs with the table on and with Q3_CP_QKV_TABLE=0 (read at load:
    one fresh child process per setting), greedy, sampled, per-slot and teacher-forced, including a slot that has ended,
    a forced id of -1 and a forced id outside the vocabulary.

cp_predict returns ids only; the hidden state compared between the two settings is the engine's talker hidden after the
last frame, which is downstream of every code-predictor pass through the feedback sum."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = (0, 7, 13)
ROWS = (1, 3, 16, 17, 32)


def _tokens():
    rng = np.random.default_rng(20251)
    return np.concatenate([[0, 1, 2047], rng.integers(0, 2048, size=13)]).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# child process: every engine / cp_predict scenario under the Q3_CP_QKV_TABLE of its environment -> one .npz
# ---------------------------------------------------------------------------------------------------------------------
def _child(out_path):
    from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
    from qwen3_tts_axera_russian_amd.llama_cpp_bindings import CodePredictor
    from tests.util import synthetic_pack
    path, cfg, _ = synthetic_pack(2, 2)
    rng = np.random.default_rng(72)
    prefixes = [(0.05 * rng.standard_normal((9 + (b % 7), 1024))).astype(np.float32) for b in range(32)]
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    res = {}
    F = 3
    eng = FrameEngine(path, max_batch=32, n_ctx=64, max_frames=F)
    eng.set_pad_embed(pad)

    def run(tag, B, sampling=None, forced=None):
        if sampling:
            eng.set_sampling(talker_temperature=0.8, talker_top_k=50, talker_top_p=0.95, cp_temperature=0.1, cp_top_k=50, seed=4242)
        else:
            eng.set_sampling(talker_temperature=0.0, cp_temperature=0.0)
        eng.start(prefixes[:B], [5] * B, ignore_eos=True, max_frames=F)
        eng.set_forced_codes(forced)
        assert eng.run(F) == F
        codes, per = eng.codes()
        res[f"{tag}_codes"] = codes.copy()
        res[f"{tag}_hidden"] = eng.hidden().copy()

    for B in (1, 3, 32):
        run(f"greedy{B}", B)
        run(f"sampled{B}", B, sampling=True)
        # teacher forcing: every decision of some (frame, row, column) entries replaced, the others free-running (-1)
        frng = np.random.default_rng(100 + B)
        forced = np.where(frng.random((F, B, 16)) < 0.5, frng.integers(0, 2048, size=(F, B, 16)), -1).astype(np.int32)
        run(f"forced{B}", B, forced=forced)
        # a column of -1 everywhere (nothing forced) next to ids outside the vocabulary in code-predictor columns: those
        # embed as zeros and must read neither table
        edge = np.full((F, B, 16), -1, np.int32)
        edge[:, :, 3] = 2048
        edge[1:, :, 9] = 5000
        edge[:, B - 1, 15] = 1 << 30
        run(f"edge{B}", B, forced=edge)
    eng.destroy()
    # per-slot mode, sampled, with slots that end early (their rows keep running through the code predictor)
    eng = FrameEngine(path, max_batch=3, n_ctx=64, max_frames=F)
    eng.set_pad_embed(pad)
    eng.open(3, ignore_eos=True)
    eng.admit([0, 1, 2], prefixes[:3], [5, 5, 5],
              [SlotParams(max_frames=mf, temperature=0.8, top_k=50, top_p=0.95, cp_temperature=0.1, cp_top_k=50, seed=77, utt=u)
               for u, mf in enumerate((3, 1, 2))])
    eng.run(F)
    codes, per = eng.codes()
    res["slots_codes"], res["slots_per"] = codes.copy(), per.copy()
    eng.destroy()
    # cp_predict: one utterance, greedy (captured graph from the second call on) and sampled (eager)
    cp = CodePredictor(path, max_batch=1)
    hid = rng.standard_normal((3, 1024)).astype(np.float32)
    res["cp_greedy"] = np.array([cp.predict(hid[i], 100 + i) for i in range(3)], np.int32)
    res["cp_sampled"] = np.array([cp.predict(hid[i], 100 + i, temperature=0.9, top_k=50, seed=11 + i) for i in range(3)], np.int32)
    cp.destroy()
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def ab(gpu_lib, tmp_path_factory):
    """-> ({name: array} with the table, the same without, stderr with, stderr without)."""
    d = tmp_path_factory.mktemp("cp_qkv_table")
    out = []
    for on in ("1", "0"):
        env = dict(os.environ, Q3_CP_QKV_TABLE=on)
        p = str(d / f"table{on}.npz")
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_cp_qkv_table", p], cwd=ROOT, env=env, text=True,
                           capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        out.append((dict(np.load(p)), r.stderr))
    return out[0][0], out[1][0], out[0][1], out[1][1]


@pytest.fixture(scope="module")
def model(test_lib):
    from tests.util import synthetic_pack
    path, cfg, tensors = synthetic_pack(2, 2)
    test_lib.q3t_reset_linear_knobs()     # the dispatch a fresh process starts with, whatever an earlier test module set
    m = test_lib.q3t_cp_model_load(path.encode())
    assert m
    yield m, cfg
    test_lib.q3t_cp_model_free(m)


def _tab_rows(test_lib, m, g, toks):
    from qwen3_tts_axera_russian_amd import hiplib
    ld = test_lib.q3t_cp_qkv_ld(m)
    assert ld > 0, "the model carries no q|k|v table (Q3_CP_QKV_TABLE=0 in this environment?)"
    toks = np.ascontiguousarray(toks, np.int32)
    out = np.empty((len(toks), ld), np.float32)
    assert test_lib.q3t_cp_qkv_tab(m, g, hiplib.iptr(toks), len(toks), hiplib.fptr(out)) == 0
    return out


def _live_rows(test_lib, m, g, toks, row0=0):
    from qwen3_tts_axera_russian_amd import hiplib
    toks = np.ascontiguousarray(toks, np.int32)
    out = np.empty((len(toks), 4096), np.float32)
    assert test_lib.q3t_cp_qkv_live(m, g, hiplib.iptr(toks), len(toks), row0, hiplib.fptr(out)) == 0
    return out, test_lib.q3t_last_linear_variant().decode()


@pytest.mark.parametrize("g", GROUPS)
def test_table_rows_equal_live_rows_bit_for_bit(test_lib, model, g):
    m, cfg = model
    assert (cfg.n_heads + 2 * cfg.n_kv_heads) * 128 == 4096 and test_lib.q3t_cp_qkv_ld(m) == 4096
    toks = _tokens()
    tab = _tab_rows(test_lib, m, g, toks)
    assert np.isfinite(tab).all() and np.abs(tab).max() > 0
    variants = {}
    for R in ROWS:
        assert test_lib.q3t_cp_qkv_serves(m, R) == 1, R     # one table serves every row count of the weight-streaming kernel
        t = np.resize(toks, R)     # the first R ids, cycled beyond 16: {0}, {0, 1, 2047}, ...
        live, variants[R] = _live_rows(test_lib, m, g, t)
        want = _tab_rows(test_lib, m, g, t)
        assert np.array_equal(live.view(np.uint32), want.view(np.uint32)), (g, R, variants[R])
    # the two row-tile variants of linear_kernel were both exercised (same K split: 4 k-blocks per wave, 8 waves)
    assert variants[1] == variants[3] == variants[16] == "linear<1,1,4,8,NORM,STORE,t>", variants
    assert variants[17] == variants[32] == "linear<1,2,4,8,NORM,STORE,t>", variants
    # rows of a chain that starts at a later 16-row block
    live, _ = _live_rows(test_lib, m, g, toks[:3], row0=16)
    assert np.array_equal(live.view(np.uint32), tab[:3].view(np.uint32))


def test_row_counts_of_the_tiled_gemm_keep_the_live_launch(test_lib, model):
    """>= 65 rows go to the tiled GEMM, which sums K in another order: cp_frame's predicate leaves the launch in."""
    m, cfg = model
    assert test_lib.q3t_cp_qkv_serves(m, 64) == 1
    assert test_lib.q3t_cp_qkv_serves(m, 65) == 0 and test_lib.q3t_cp_qkv_serves(m, 128) == 0


def test_opt_out_allocates_no_table(ab):
    on, off, err_on, err_off = ab
    lines = [ln for ln in err_on.splitlines() if "layer-0 q|k|v table" in ln]
    assert lines and all("14 groups x 2048 tokens x 4096 columns f32 = 469762048 bytes" in ln for ln in lines), err_on[-2000:]
    assert "q|k|v table" not in err_off


@pytest.mark.parametrize("B", (1, 3, 32))
@pytest.mark.parametrize("mode", ("greedy", "sampled", "forced", "edge"))
def test_engine_codes_identical_with_and_without_the_table(ab, mode, B):
    on, off = ab[0], ab[1]
    a, b = on[f"{mode}{B}_codes"], off[f"{mode}{B}_codes"]
    assert a.shape == (3, B, 16) and (a[:, :, 1:] >= 0).all() and (a[:, :, 1:] < 2048).all()
    assert np.array_equal(a, b)
    assert np.array_equal(on[f"{mode}{B}_hidden"].view(np.uint32), off[f"{mode}{B}_hidden"].view(np.uint32))
    if mode == "sampled":   # the draws really are draws: not the greedy trajectory
        assert not np.array_equal(a, on[f"greedy{B}_codes"])


def test_per_slot_mode_with_ended_slots_identical(ab):
    on, off = ab[0], ab[1]
    assert list(on["slots_per"]) == [3, 1, 2]
    assert np.array_equal(on["slots_codes"], off["slots_codes"]) and np.array_equal(on["slots_per"], off["slots_per"])


def test_cp_predict_identical_with_and_without_the_table(ab):
    on, off = ab[0], ab[1]
    for k in ("cp_greedy", "cp_sampled"):
        assert on[k].shape == (3, 15) and np.array_equal(on[k], off[k]), k
    assert not np.array_equal(on["cp_greedy"], on["cp_sampled"])


if __name__ == "__main__":
    _child(sys.argv[1])
