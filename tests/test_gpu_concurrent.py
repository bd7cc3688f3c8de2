"""Per-slot frame loop (q3e_open / q3e_admit / q3e_release) and batch_server --concurrent on the GPU, with tiny synthetic
packs: per-slot budgets, greedy and sampled rows side by side, draws that do not depend on the slot, the old q3e_start path
untouched, and concurrent requests that each get the reply they get alone."""
import os
import socket
import threading
import time

import numpy as np
import pytest

from oracle.pipeline import CpuPipeline
from qwen3_tts_axera_russian_amd import weights as W
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from tests.test_gpu_engine import _compare, _prefixes
from tests.util import CACHE, synthetic_pack

pytestmark = pytest.mark.gpu

SAMPLED = dict(temperature=1.0, top_k=50, top_p=0.95, cp_temperature=1.0, cp_top_k=50)


@pytest.fixture(scope="module")
def world():
    path, cfg, tensors = synthetic_pack(2, 2)
    return path, cfg, tensors, CpuPipeline(cfg, tensors, n_ctx=96)


def _engine(path, pad, max_batch=4, n_ctx=96, max_frames=24):
    eng = FrameEngine(path, max_batch=max_batch, n_ctx=n_ctx, max_frames=max_frames)
    eng.set_pad_embed(pad)
    return eng


def _column(eng, b):
    codes, per = eng.codes()
    return np.ascontiguousarray(codes[:int(per[b]), b, :])


def test_per_slot_budgets_end_each_slot_at_its_own_frame(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(81)
    prefixes = _prefixes(rng, [12, 15, 9, 20])
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    budgets = [3, 6, 9, 12]
    eng = _engine(path, pad, max_frames=16)
    eng.open(4, ignore_eos=True)
    assert eng.run(8) == 0                                   # nothing admitted: no step
    eng.admit([0, 1, 2, 3], prefixes, [30] * 4, [SlotParams(max_frames=m) for m in budgets])
    for k in range(1, 13):
        assert eng.run(1) == 1
        done, per = eng.done()
        assert [int(x) for x in per] == [min(k, m) for m in budgets], k
        assert [bool(x) for x in done] == [k >= m for m in budgets], k
    assert eng.run(8) == 0                                   # every slot has used its budget
    codes, per = eng.codes()
    assert codes.shape[0] == 12
    for b, m in enumerate(budgets):
        assert ((codes[:m, b] >= 0) & (codes[:m, b] < 2048)).all()
        assert (codes[m:, b, 0] == -1).all()
    # greedy rows of a per-slot batch decode what the CPU pipeline decodes (EOS ignored, each to its budget)
    for b, m in enumerate(budgets):
        ref, margins = cpu.generate(prefixes[b], 30, pad, m, ignore_eos=True, want_margins=True)
        _compare(codes[:, b:b + 1], per[b:b + 1], [ref], [margins])
    eng.destroy()


def test_greedy_and_sampled_rows_share_one_loop(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(82)
    p0, p1 = _prefixes(rng, [12, 17])
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    F = 20
    eng = _engine(path, pad)
    eng.open(4)
    greedy = SlotParams(max_frames=F)
    top1 = SlotParams(max_frames=F, temperature=1.0, top_k=1, top_p=0.95, cp_temperature=1.0, cp_top_k=1, seed=7)
    tiny_p = SlotParams(max_frames=F, temperature=1.0, top_k=50, top_p=1e-6, cp_temperature=1.0, cp_top_k=1, seed=7)
    eng.admit([0, 1, 2, 3], [p0, p0, p1, p1], [30, 30, 30, 30], [greedy, top1, greedy, tiny_p])
    while eng.run(8) > 0:
        pass
    done, per = eng.done()
    assert done.all()
    codes, _ = eng.codes()
    refs, margins = [], []
    for p in (p0, p1):
        fr, mm = cpu.generate(p, 30, pad, F, want_margins=True)
        refs.append(fr)
        margins.append(mm)
    stats = _compare(codes[:, [0, 2]], per[[0, 2]], refs, margins)
    print("greedy rows:", stats)
    np.testing.assert_array_equal(_column(eng, 1), _column(eng, 0))   # top_k = 1 draws the arg-max
    np.testing.assert_array_equal(_column(eng, 3), _column(eng, 2))   # top_p -> 0 keeps the top entry only
    # sampled rows beside greedy ones: valid ids, a different stream than the greedy one
    eng.admit([1, 3], [p0, p0], [30, 30], [SlotParams(max_frames=F, seed=11, **SAMPLED), greedy])
    while eng.run(8) > 0:
        pass
    s, g = _column(eng, 1), _column(eng, 3)
    assert s.shape[0] >= 1 and ((s >= 0) & (s < 2048)).all()
    assert not np.array_equal(s[:min(len(s), len(g))], g[:min(len(s), len(g))])
    eng.destroy()


def test_release_ends_a_slot_mid_run_and_leaves_the_others(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(85)
    prefixes = _prefixes(rng, [12, 15])
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    eng = _engine(path, pad)
    eng.open(4, ignore_eos=True)
    eng.admit([0, 1], prefixes, [30, 30], [SlotParams(max_frames=20)] * 2)
    assert eng.run(4) == 4
    eng.release([0])
    done, per = eng.done()
    assert done[0] and not done[1] and int(per[0]) == 4
    assert eng.run(100) == 16                            # the released slot no longer holds the loop
    done, per = eng.done()
    assert done.all() and [int(x) for x in per[:2]] == [4, 20]
    codes, _ = eng.codes()
    assert (codes[4:, 0, 0] == -1).all() and (codes[:20, 1, 0] >= 0).all()
    eng.destroy()


def test_draws_do_not_depend_on_the_slot_or_earlier_admissions(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(83)
    p, q0, q1, q2 = _prefixes(rng, [14, 11, 16, 9])
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    F = 12
    S = SlotParams(max_frames=F, seed=1234, **SAMPLED)
    other = [SlotParams(max_frames=F, seed=s, **SAMPLED) for s in (1, 2, 3)]
    eng = _engine(path, pad)

    def finish():
        while eng.run(8) > 0:
            pass

    eng.open(4, ignore_eos=True)                         # alone in slot 0
    eng.admit([0], [p], [30], [S])
    finish()
    alone = _column(eng, 0)
    assert alone.shape == (F, 16)
    eng.open(4, ignore_eos=True)                         # slot 3, beside three live utterances
    eng.admit([0, 1, 2, 3], [q0, q1, q2, p], [30] * 4, other + [S])
    finish()
    np.testing.assert_array_equal(_column(eng, 3), alone)
    eng.open(4, ignore_eos=True)                         # after five earlier admissions, mid-run of the others
    for k, (b, pr) in enumerate([(0, q0), (1, q1), (2, q2), (3, q0)]):
        eng.admit([b], [pr], [30], [other[k % 3]])
        eng.run(2)
    eng.release([0])
    eng.admit([0], [q1], [30], [other[0]])
    eng.run(3)
    eng.release([2])
    eng.admit([2], [p], [30], [S])
    finish()
    np.testing.assert_array_equal(_column(eng, 2), alone)
    eng.open(4, ignore_eos=True)                         # another seed: another stream
    eng.admit([0], [p], [30], [SlotParams(max_frames=F, seed=1235, **SAMPLED)])
    finish()
    assert not np.array_equal(_column(eng, 0), alone)
    eng.destroy()


def test_q3e_start_sampling_is_unchanged_after_a_per_slot_batch(gpu_lib, world):
    path, cfg, tensors, cpu = world
    rng = np.random.default_rng(84)
    prefixes = _prefixes(rng, [12, 14, 10])
    pad = (0.05 * rng.standard_normal(1024)).astype(np.float32)
    F = 10
    eng = _engine(path, pad)

    def old_path():
        eng.set_sampling(talker_temperature=1.0, talker_top_k=50, talker_top_p=0.95, cp_temperature=1.0, cp_top_k=50, seed=99)
        eng.start(prefixes, [30] * 3, ignore_eos=True, max_frames=F)
        assert eng.run(F) == F
        return eng.codes()[0].copy()

    before = old_path()
    eng.open(4, ignore_eos=True)
    eng.admit([1, 2], prefixes[:2], [30, 30], [SlotParams(max_frames=F, seed=5, **SAMPLED)] * 2)
    while eng.run(8) > 0:
        pass
    with pytest.raises(RuntimeError):
        eng.refill([0], [prefixes[0]], [30])             # a per-slot batch takes q3e_admit only
    after = old_path()
    np.testing.assert_array_equal(after, before)
    eng.destroy()


# ---- batch_server --concurrent, end to end ----

@pytest.fixture(scope="module")
def packs():
    os.makedirs(CACHE, exist_ok=True)
    cfg = W.tiny_config(2, 2, text_vocab=512)
    cfg.text_dim = 64
    main = os.path.join(CACHE, "srv_tiny_t2c2.q3w")
    if not os.path.exists(main):
        W.write_synthetic(main, cfg, seed=1234, parts=("talker", "cp", "text"))
    voc = os.path.join(CACHE, "srv_voc_tiny.q3w")
    if not os.path.exists(voc):
        W.write_pack(voc, {"voc_chunk": 64.0}, W.make_synthetic_voc(W.tiny_voc_config(), seed=7))
    return main, voc


def _server(packs, sock):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    main, voc = packs
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=160, max_tokens=80, temperature=0.0,
                                  cp_temperature=0.0, install_signal_handlers=False, concurrent=True)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(400):
        if os.path.exists(sock) and srv.sched is not None:
            break
        time.sleep(0.05)
    return srv, th


def _stop(srv, th):
    srv._running = False
    th.join(timeout=60)
    assert not th.is_alive()
    srv.close()


def _call(sock, req):
    """-> list of (codes, pcm) per utterance; a streamed request's records joined."""
    from qwen3_tts_axera_russian_amd import batch_server as bs
    req = dict(req)
    if not req.pop("stream", False):
        return bs.synthesize_batch(sock, **req)
    n = len(req["token_ids"])
    pcm, codes = [[] for _ in range(n)], [None] * n
    for rec in bs.synthesize_batch_stream(sock, **req):
        if rec[0] == "audio":
            pcm[rec[1]].append(rec[2])
        else:
            codes[rec[1]] = rec[2]
    return [(codes[u], np.concatenate(pcm[u]) if pcm[u] else np.zeros(0, np.int16)) for u in range(n)]


LONG = [5, 17, 200, 33, 41, 7, 90, 120, 64, 3, 11, 250, 77, 8, 19, 300, 45, 60, 2, 150, 99, 21, 13, 55, 180]
SAMPLE_KEYS = dict(temperature=0.9, top_k=30, top_p=0.9, cp_temperature=0.5, cp_top_k=20)
REQUESTS = [
    dict(token_ids=[LONG], max_tokens=70),
    dict(token_ids=[[9, 8, 7], [301, 302, 303, 304, 305, 306]], max_tokens=40, stream=True),
    dict(token_ids=[LONG[:12]], max_tokens=66, seed=5, **SAMPLE_KEYS),
    dict(token_ids=[LONG[3:20], [44, 45]], max_tokens=50, seed=6, stream=True, **SAMPLE_KEYS),
    dict(token_ids=[[301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311, 312]], max_tokens=25),
    dict(token_ids=[LONG[5:]], max_tokens=80, seed=7, stream=True, **SAMPLE_KEYS),
    dict(token_ids=[[1, 2, 3, 4, 5], LONG[:9], [77]], max_tokens=33, seed=8, **SAMPLE_KEYS),
    dict(token_ids=[LONG[::-1]], max_tokens=64, stream=True),
]


def test_concurrent_server_replies_do_not_depend_on_the_traffic(gpu_lib, packs, tmp_path):
    from qwen3_tts_axera_russian_amd import batch_server as bs
    sock = str(tmp_path / "conc.sock")
    srv, th = _server(packs, sock)
    got, errs = [None] * len(REQUESTS), []
    # the engine's calls, seen from the test: which slots the quitter's utterances get (budget 79 marks them), which slots are
    # released; the first run after the quitter's admission waits until the quitter has closed its connection, so its
    # utterances are mid-run (8 frames in, budget 79) when the scheduler notices
    eng = srv.eng
    admit0, run0, release0 = eng.admit, eng.run, eng.release
    q_slots, released, closed = [], [], threading.Event()

    def admit(slots, prefixes, n_text, params):
        admit0(slots, prefixes, n_text, params)
        q_slots.extend(int(b) for b, p in zip(slots, params) if p.max_frames == 79)

    def run(n):
        if q_slots:
            closed.wait(timeout=120)
        return run0(n)

    def release(slots):
        released.extend(int(b) for b in slots)
        release0(slots)
    eng.admit, eng.run, eng.release = admit, run, release
    try:
        # a client that goes away mid-request: its slots are released and the others are not stalled
        quitter = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        quitter.connect(sock)
        quitter.sendall(bs.pack_batch_request(token_ids=[LONG, LONG], max_tokens=79))
        t = time.time()
        while len(q_slots) < 2:
            assert time.time() - t < 60, "the quitter's utterances were not admitted"
            time.sleep(0.005)
        quitter.close()
        closed.set()

        def client(i):
            try:
                got[i] = _call(sock, REQUESTS[i])
            except Exception as e:      # noqa: BLE001 -- reported below
                errs.append((i, repr(e)))
        ths = [threading.Thread(target=client, args=(i,)) for i in range(len(REQUESTS))]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=300)
        assert not errs, errs
        assert len(set(q_slots)) == 2 and set(q_slots) <= set(released), (q_slots, released)   # released mid-run
        steps = srv.sched.frame_steps
    finally:
        _stop(srv, th)
    # every reply = the reply the same request gets alone on a fresh --concurrent server (unstreamed there: a streamed reply
    # joined equals the unstreamed one)
    total = 0
    for i, req in enumerate(REQUESTS):
        alone_sock = str(tmp_path / f"alone{i}.sock")
        srv, th = _server(packs, alone_sock)
        try:
            ref = _call(alone_sock, dict(req, stream=False))
        finally:
            _stop(srv, th)
        assert len(got[i]) == len(ref) == len(req["token_ids"])
        for u, ((c, p), (rc, rp)) in enumerate(zip(got[i], ref)):
            assert rc.shape[0] >= 1 and rc.shape[0] <= req["max_tokens"], (i, u)
            np.testing.assert_array_equal(c, rc, err_msg=f"request {i} utterance {u}: codes")
            np.testing.assert_array_equal(p, rp, err_msg=f"request {i} utterance {u}: pcm")
            total += rc.shape[0]
    print("frame steps", steps, "frames", total)
    assert steps < total                                   # the requests shared the loop
