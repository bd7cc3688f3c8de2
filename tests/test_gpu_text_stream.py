"""Text streamed into running utterances (q3e_text_reserve / q3e_push_text / q3e_text_state), on the tiny synthetic pack of
tests/test_gpu_concurrent.py: a text row stands where the pad stands in the feedback, a slot never runs ahead of its
text, the EOS rules wait for the final push, and the old paths keep their bits.

Bounds: NEAR_TIE of tests/test_gpu_engine.py.  Two hidden states are "the same" when max |logit difference| over the
codec head is below NEAR_TIE / 2 (the bound that file measures for device against oracle), and a device decision is
accepted when it is the oracle's arg-max or the oracle's own gap to it is below NEAR_TIE."""
import numpy as np
import pytest

from oracle import oracle as orc
from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from tests.test_gpu_engine import NEAR_TIE, _prefixes
from tests.text_stream_ref import Follower, logit_distance
from tests.util import synthetic_pack

pytestmark = pytest.mark.gpu

SAMPLED = dict(temperature=1.0, top_k=50, top_p=0.95, cp_temperature=1.0, cp_top_k=50)
H = 1024


@pytest.fixture(scope="module")
def world():
    return synthetic_pack(2, 2)


def _rows(rng, n):
    return (0.05 * rng.standard_normal((n, H))).astype(np.float32)


def _engine(path, pad, max_batch=4, max_frames=24, reserve=16):
    eng = FrameEngine(path, max_batch=max_batch, n_ctx=96, max_frames=max_frames)
    eng.set_pad_embed(pad)
    if reserve:
        eng.reserve_text(reserve)
    return eng


def _column(eng, b):
    codes, per = eng.codes()
    return np.ascontiguousarray(codes[:int(per[b]), b, :])


def _finish(eng):
    while eng.run(8) > 0:
        pass


def test_pad_rows_give_the_ordinary_slots_bits(gpu_lib, world):
    path, cfg, tensors = world
    rng = np.random.default_rng(301)
    (p,) = _prefixes(rng, [13])
    pad = _rows(rng, 1)[0]
    F = 16
    eng = _engine(path, pad)
    for one_by_one in (False, True):
        eng.open(4, ignore_eos=True)
        eng.admit([0, 1], [p, p], [30, 30], [SlotParams(max_frames=F), SlotParams(max_frames=F, text_stream=True)])
        if one_by_one:
            for k in range(F):
                eng.push_text(1, pad[None])
                assert eng.run(1) == 1, k
        else:
            eng.push_text(1, np.repeat(pad[None], F, axis=0))
            assert eng.run(F) == F
        a, b = _column(eng, 0), _column(eng, 1)
        assert a.shape == (F, 16)
        np.testing.assert_array_equal(b, a)
    eng.destroy()


def test_every_frame_against_the_oracle_following_the_device(gpu_lib, world):
    path, cfg, tensors = world
    rng = np.random.default_rng(302)
    prefixes = _prefixes(rng, [8, 12, 9, 15])
    pad = _rows(rng, 1)[0]
    n_rows = [1, 5, 11, 16]
    rows = [_rows(rng, n) for n in n_rows]
    F = 16
    eng = _engine(path, pad)
    eng.open(4, ignore_eos=True)
    eng.admit([0, 1, 2, 3], prefixes, [0] * 4, [SlotParams(max_frames=F, text_stream=True)] * 4)
    eng.push_text(0, rows[0], final=True, n_text=1)          # everything at admit, final
    eng.push_text(1, rows[1], final=True, n_text=5)
    eng.push_text(3, rows[3][:3])                            # 3 rows, the rest before they are needed, never final
    talker, cp = orc.TalkerOracle(cfg, tensors, n_ctx=96), orc.CpOracle(cfg, tensors)
    true = [Follower(cfg, talker, cp, prefixes[b], rows[b], pad) for b in range(4)]
    # what a wrong implementation would compute from the same ids: the rows one frame late, and pad instead of the rows
    late = [Follower(cfg, talker, cp, prefixes[b], [pad] + list(rows[b]), pad) for b in range(4)]
    none = [Follower(cfg, talker, cp, prefixes[b], [], pad) for b in range(4)]
    hid = eng.hidden()
    worst = max(logit_distance(true[b].talker, hid[b], true[b].hidden) for b in range(4))
    sep_late = sep_none = 0.0
    bad = []
    for k in range(F):
        if k < 11:                                           # slot 2: one row per step, final with the last
            eng.push_text(2, rows[2][k:k + 1], final=(k == 10), n_text=11)
        if k == 2:
            eng.push_text(3, rows[3][3:])
        assert eng.run(1) == 1, k
        codes, per = eng.codes()
        assert [int(x) for x in per] == [k + 1] * 4
        hid = eng.hidden()
        for b in range(4):
            ids = codes[k, b]
            bad += [(b, k) + x for x in true[b].grade(ids, NEAR_TIE)]
            h = true[b].feed(ids)
            worst = max(worst, logit_distance(true[b].talker, hid[b], h))
            sep_late = max(sep_late, logit_distance(true[b].talker, late[b].feed(ids), h))
            sep_none = max(sep_none, logit_distance(true[b].talker, none[b].feed(ids), h))
    print(f"device vs oracle: max logit distance {worst:.3e} (bound {NEAR_TIE / 2}); rows one frame late {sep_late:.3e}, "
          f"pad for rows {sep_none:.3e} (must be >= {10 * NEAR_TIE / 2}); decisions off a near-tie: {bad}")
    # the check cannot weaken silently: a wrong row must move the logits by ten times the bound
    assert sep_late >= 10 * NEAR_TIE / 2 and sep_none >= 10 * NEAR_TIE / 2
    assert worst < NEAR_TIE / 2
    assert not bad, bad
    eng.destroy()


def _one_text_run(eng, slot, prefix, rows, params, schedule, B=4, beside=None):
    """The text utterance in `slot` with its rows pushed per `schedule` ('all', 'split', 'steps') -> its codes."""
    eng.open(B, ignore_eos=True)
    if beside is not None:
        b, p, sp = beside
        eng.admit([b], [p], [30], [sp])
    eng.admit([slot], [prefix], [0], [params])
    n = len(rows)
    if schedule == "all":
        eng.push_text(slot, rows, final=True, n_text=n)
    elif schedule == "split":
        eng.push_text(slot, rows[:3])
        assert eng.run(8) == 3
        eng.push_text(slot, rows[3:], final=True, n_text=n)
    else:
        for k in range(n):
            eng.push_text(slot, rows[k:k + 1], final=(k == n - 1), n_text=n)
            assert eng.run(1) == 1
    _finish(eng)
    return _column(eng, slot)


@pytest.mark.parametrize("sampled", [False, True])
def test_codes_depend_on_the_text_and_not_on_its_arrival(gpu_lib, world, sampled):
    path, cfg, tensors = world
    rng = np.random.default_rng(303)
    p, q = _prefixes(rng, [8, 14])
    pad = _rows(rng, 1)[0]
    rows = _rows(rng, 9)
    F = 14
    kw = dict(seed=77, **SAMPLED) if sampled else {}
    S = SlotParams(max_frames=F, text_stream=True, **kw)
    other = SlotParams(max_frames=F, seed=5, **SAMPLED)
    # a batch of 17 rows throughout: slot 16 sits in the second 16-row tile of the frame's buffers
    eng = _engine(path, pad, max_batch=17)
    run = lambda slot, sched, beside=None, r=rows: _one_text_run(eng, slot, p, r, S, sched, B=17, beside=beside)
    base = run(0, "all")
    assert base.shape == (F, 16)
    np.testing.assert_array_equal(run(0, "split"), base)
    np.testing.assert_array_equal(run(0, "steps"), base)
    np.testing.assert_array_equal(run(3, "split"), base)
    np.testing.assert_array_equal(run(16, "steps"), base)
    np.testing.assert_array_equal(run(16, "split", beside=(3, q, other)), base)
    np.testing.assert_array_equal(run(2, "all", beside=(16, q, other)), base)
    # the rows matter: pad in their place gives other codes
    assert not np.array_equal(run(0, "all", r=np.repeat(pad[None], 9, axis=0)), base)
    eng.destroy()


def test_a_starved_slot_stalls_the_batch_and_resumes(gpu_lib, world):
    path, cfg, tensors = world
    rng = np.random.default_rng(304)
    p, q = _prefixes(rng, [8, 11])
    pad = _rows(rng, 1)[0]
    rows = _rows(rng, 10)
    F = 14
    T, O = SlotParams(max_frames=F, text_stream=True), SlotParams(max_frames=F)
    eng = _engine(path, pad)
    eng.open(4, ignore_eos=True)                            # unstarved
    eng.admit([0, 2], [q, p], [30, 0], [O, T])
    eng.push_text(2, rows, final=True, n_text=10)
    _finish(eng)
    ref_o, ref_t = _column(eng, 0), _column(eng, 2)
    eng.open(4, ignore_eos=True)
    eng.admit([0, 2], [q, p], [30, 0], [O, T])
    n, starved = eng.text_state()
    assert list(n) == [0, 0, 0, 0] and list(starved) == [False, False, True, False]
    assert eng.run(8) == 0                                   # no row yet: no step
    eng.push_text(2, rows[:3])
    assert not eng.text_state()[1].any()
    assert eng.run(8) == 3
    n, starved = eng.text_state()
    assert list(n) == [0, 0, 3, 0] and list(starved) == [False, False, True, False]
    done, per = eng.done()
    assert [int(per[0]), int(per[2])] == [3, 3] and not done[0] and not done[2]   # the ordinary slot waited too
    assert eng.run(8) == 0
    eng.push_text(2, rows[3:], final=True, n_text=10)
    assert not eng.text_state()[1].any()
    _finish(eng)
    np.testing.assert_array_equal(_column(eng, 0), ref_o)
    np.testing.assert_array_equal(_column(eng, 2), ref_t)
    assert ref_t.shape == (F, 16)
    # a released starving slot no longer holds the loop
    eng.open(4, ignore_eos=True)
    eng.admit([0, 2], [q, p], [30, 0], [O, T])
    assert eng.run(8) == 0
    eng.release([2])
    assert eng.run(4) == 4
    eng.destroy()


def test_eos_rules_wait_for_the_final_push(gpu_lib, world):
    path, cfg, tensors = world
    rng = np.random.default_rng(305)
    p, q = _prefixes(rng, [8, 10])
    pad = _rows(rng, 1)[0]
    rows = _rows(rng, 16)
    F = 24
    T = SlotParams(max_frames=F, text_stream=True)
    eng = _engine(path, pad, reserve=24)
    eng.open(4, ignore_eos=False)
    eng.admit([0, 1], [p, q], [2, 2], [T, T])                # (n_text of a text slot is ignored)
    eng.push_text(0, rows[:2])
    eng.push_text(0, np.repeat(pad[None], 12, axis=0))       # rows to run on, the text still open
    eng.push_text(1, rows[:16])
    ran = 0
    for k in range(14):
        if k == 4:                                           # slot 1: final early, 1 token: forced at progress > 2, frame 7
            eng.push_text(1, rows[:0], final=True, n_text=1)
        assert eng.run(1) == 1
        done, per = eng.done()
        # slot 0: n_text = 2 would force EOS at progress 13 / 6 > 2; with the text open nothing ends it
        assert not done[0] and int(per[0]) == k + 1, k
        if k < 4:
            assert not done[1] and int(per[1]) == k + 1, k   # never before its final push
    done, per = eng.done()
    # slot 1 after its final push (4 frames emitted, n_text 1): the rule forces EOS once progress = np / 3 > 2, i.e. at the
    # frame sampled with np = 7; the boost may end it earlier, never before the push
    assert done[1] and 4 <= int(per[1]) <= 7, per
    codes, _ = eng.codes()
    assert (codes[:14, 0, 0] >= 0).all() and (codes[:14, 0, 0] < 2048).all()
    eng.push_text(0, rows[:0], final=True, n_text=2)
    assert eng.run(1) == 1                                   # the next sampled frame: progress 14 / 6 > 2, EOS forced
    done, per = eng.done()
    assert done[0] and int(per[0]) == 14
    eng.destroy()


def test_refused_calls_change_nothing(gpu_lib, world):
    path, cfg, tensors = world
    rng = np.random.default_rng(306)
    p, q = _prefixes(rng, [8, 11])
    pad = _rows(rng, 1)[0]
    rows = _rows(rng, 8)
    F = 10
    T, O = SlotParams(max_frames=F, text_stream=True), SlotParams(max_frames=F)
    eng = _engine(path, pad, reserve=0)
    eng.open(4, ignore_eos=True)
    with pytest.raises(RuntimeError):
        eng.admit([1], [p], [0], [T])                        # the text bit without a reservation
    assert eng.run(4) == 0                                   # nothing was admitted
    with pytest.raises(RuntimeError):
        eng.reserve_text(25)                                 # more rows than frames
    eng.reserve_text(8)
    eng.open(4, ignore_eos=True)
    eng.admit([0, 1], [q, p], [30, 0], [O, T])
    eng.push_text(1, rows, final=True, n_text=8)
    _finish(eng)
    ref_o, ref_t = _column(eng, 0), _column(eng, 1)

    eng.open(4, ignore_eos=True)
    eng.admit([0, 1], [q, p], [30, 0], [O, T])
    with pytest.raises(ValueError):
        eng.push_text(0, rows[:1])                           # an ordinary slot
    with pytest.raises(ValueError):
        eng.push_text(3, rows[:1])                           # an idle slot
    nan = rows[:3].copy()
    nan[2, 100] = np.nan
    with pytest.raises(ValueError):
        eng.push_text(1, nan)                                # a non-finite value: none of the three rows is written
    with pytest.raises(ValueError):
        eng.push_text(1, np.concatenate([rows, rows[:1]]))   # 9 rows into a reservation of 8
    assert list(eng.text_state()[0]) == [0, 0, 0, 0]
    eng.push_text(1, rows[:5])
    with pytest.raises(ValueError):
        eng.push_text(1, rows[:4])                           # 5 + 4 > 8
    eng.push_text(1, rows[5:], final=True, n_text=8)
    with pytest.raises(ValueError):
        eng.push_text(1, rows[:0])                           # after the final push
    assert list(eng.text_state()[0]) == [0, 8, 0, 0]
    _finish(eng)
    np.testing.assert_array_equal(_column(eng, 0), ref_o)
    np.testing.assert_array_equal(_column(eng, 1), ref_t)
    eng.destroy()


def test_old_paths_keep_their_bits_after_a_text_batch(gpu_lib, world):
    path, cfg, tensors = world
    rng = np.random.default_rng(307)
    prefixes = _prefixes(rng, [12, 14, 10])
    pad = _rows(rng, 1)[0]
    rows = _rows(rng, 6)
    F = 10
    eng = _engine(path, pad, reserve=0)
    S = SlotParams(max_frames=F, seed=5, **SAMPLED)

    def start_path():
        eng.set_sampling(talker_temperature=1.0, talker_top_k=50, talker_top_p=0.95, cp_temperature=1.0, cp_top_k=50, seed=99)
        eng.start(prefixes, [30] * 3, ignore_eos=True, max_frames=F)
        assert eng.run(F) == F
        return eng.codes()[0].copy()

    def slot_path():
        eng.open(4, ignore_eos=True)
        eng.admit([1, 2], prefixes[:2], [30, 30], [S, SlotParams(max_frames=F)])
        _finish(eng)
        return eng.codes()[0].copy()

    before = start_path(), slot_path()
    eng.reserve_text(8)
    eng.open(4, ignore_eos=True)
    eng.admit([0, 1], prefixes[:2], [0, 30], [SlotParams(max_frames=F, text_stream=True, seed=5, **SAMPLED), S])
    eng.push_text(0, rows, final=True, n_text=6)
    _finish(eng)
    with pytest.raises(RuntimeError):
        eng.refill([0], [prefixes[0]], [30])
    after = start_path(), slot_path()                        # (the reservation still stands: the ordinary slots read no row)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    eng.reserve_text(0)
    np.testing.assert_array_equal(slot_path(), before[1])
    eng.destroy()


def test_device_text_abi_matches_the_host_mirror(gpu_lib):
    import os

    from qwen3_tts_axera_russian_amd import hiplib
    from qwen3_tts_axera_russian_amd import weights as W
    from qwen3_tts_axera_russian_amd.frontend import DeviceTextFrontEnd, load_text_front_end, text_stream_rows
    from tests.test_gpu_text import TOL, _rel
    from tests.util import CACHE
    os.makedirs(CACHE, exist_ok=True)
    cfg = W.tiny_config(2, 2, text_vocab=640)            # the pack of tests/test_gpu_text.py
    path = os.path.join(CACHE, "text_t2c2_v640.q3w")
    if not os.path.exists(path):
        W.write_synthetic(path, cfg, seed=77, parts=("talker", "text"))
    _, host = load_text_front_end(path, cfg=cfg)
    dev = DeviceTextFrontEnd(cfg, path, max_tokens=64)
    ids = [5, 17, 200, 33, 41]
    d, h = dev.build_prefix_stream(ids[0]), host.build_prefix_stream(ids[0])
    assert d.shape == h.shape == (8, 1024)
    assert _rel(d, h) <= TOL
    for j in range(8):                                       # row by row: a swapped row is not hidden by the largest one
        assert _rel(d[j], h[j]) <= TOL, j
    eos = np.empty(1024, np.float32)
    assert gpu_lib.tfe_tts_eos_embed(dev.h, hiplib.fptr(eos)) == 0
    np.testing.assert_array_equal(eos, dev.tts_eos_embed)
    assert _rel(eos, host.tts_eos_embed) <= TOL
    R = text_stream_rows(dev, ids[1:], final=True)
    assert R.shape == (5, 1024) and _rel(R, text_stream_rows(host, ids[1:], final=True)) <= TOL
    np.testing.assert_array_equal(R[4], dev.tts_eos_embed)
    dev.destroy()


# ---- batch_server --concurrent, a "text_stream" request end to end ----

from tests.test_gpu_concurrent import LONG, _call, _server, _stop, packs  # noqa: E402,F401 -- (packs: the fixture)


def _text_call(sock, pieces, gap_s, **req):
    """A text-stream request whose pieces (token ids) go out gap_s apart -> (codes, pcm)."""
    import time

    from qwen3_tts_axera_russian_amd import batch_server as bs

    def slowly():
        for i, p in enumerate(pieces):
            if i:
                time.sleep(gap_s)
            yield p
    pcm, codes = [], None
    for rec in bs.synthesize_text_stream(sock, slowly(), **req):
        assert rec[1] == 0
        if rec[0] == "audio":
            pcm.append(rec[2])
        else:
            codes = rec[2]
    return codes, np.concatenate(pcm) if pcm else np.zeros(0, np.int16)


def test_server_text_stream_reply_does_not_depend_on_the_cut_or_the_traffic(gpu_lib, packs, tmp_path):
    import threading
    text = LONG[:18]
    ordinary = dict(token_ids=[[9, 8, 7], [301, 302, 303, 304, 305, 306]], max_tokens=40, stream=True)
    sock = str(tmp_path / "ts_a.sock")
    srv, th = _server(packs, sock)
    got = {}
    try:
        def client():
            got["ordinary"] = _call(sock, ordinary)
        t = threading.Thread(target=client)
        t.start()
        got["a"] = _text_call(sock, [text[:2], text[2:3], text[3:9], [], text[9:]], 0.004, max_tokens=40)
        t.join(timeout=120)
        assert "ordinary" in got
        starved = srv.sched.starved_checks
    finally:
        _stop(srv, th)
    sock = str(tmp_path / "ts_b.sock")
    srv, th = _server(packs, sock)
    try:
        b = _text_call(sock, [text[:1]] + [[x] for x in text[1:]], 0.001, max_tokens=40)
        whole = _text_call(sock, [text], 0.0, max_tokens=40, vocoder="incremental")
        alone = _call(sock, ordinary)
        from qwen3_tts_axera_russian_amd import batch_server as bs
        with pytest.raises(RuntimeError, match="server error"):
            list(bs.synthesize_text_stream(sock, [text[:1], text[1:]], max_tokens=40, vocoder="fast"))
    finally:
        _stop(srv, th)
    print("frames", got["a"][0].shape[0], "starved checks with the slower client:", starved)
    assert 1 <= got["a"][0].shape[0] <= 40
    np.testing.assert_array_equal(got["a"][0], b[0])
    np.testing.assert_array_equal(got["a"][1], b[1])
    np.testing.assert_array_equal(whole[0], b[0])            # the whole text in the request: the same codes
    assert len(alone) == len(got["ordinary"]) == 2
    for (c, p), (rc, rp) in zip(got["ordinary"], alone):
        np.testing.assert_array_equal(c, rc)
        np.testing.assert_array_equal(p, rp)
