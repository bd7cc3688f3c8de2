"""Held text slots (q3e_text_hold / q3e_text_held), on the tiny synthetic pack and with the helpers of
tests/test_gpu_text_stream.py: a live text slot without a row for its next frame is held inside the captured frame while
the other slots step on, and a held step leaves the held row exactly where it was.

Every reference is an engine with hold OFF and all rows pushed at admission (what tests/test_gpu_text_stream.py grades
against the CPU oracle); every comparison is exact."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd.engine import FrameEngine, SlotParams
from tests.test_gpu_engine import _prefixes
from tests.test_gpu_text_stream import SAMPLED, _column, _engine, _finish, _rows, world  # noqa: F401 -- (world: the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(world):
    """(hold on, hold off): 17 slots, 24 frames, 24 text rows; one pad row for both."""
    path, cfg, tensors = world
    pad = _rows(np.random.default_rng(400), 1)[0]
    on = _engine(path, pad, max_batch=17, reserve=24)
    on.hold_text()
    off = _engine(path, pad, max_batch=17, reserve=24)
    yield on, off, pad
    on.destroy()
    off.destroy()


def _admit(eng, B, utts, ignore_eos=True):
    """utts: {slot: (prefix, SlotParams, text rows or None)} -> an open batch with them admitted, nothing pushed."""
    eng.open(B, ignore_eos=ignore_eos)
    for b, (p, sp, rows) in utts.items():
        eng.admit([b], [p], [0 if rows is not None else 30], [sp])


def _reference(off, B, utts):
    """Hold off, every row at admission -> {slot: codes}."""
    _admit(off, B, utts)
    for b, (p, sp, rows) in utts.items():
        if rows is not None:
            off.push_text(b, rows, final=True, n_text=len(rows))
    _finish(off)
    return {b: _column(off, b) for b in utts}


def _frames(eng, slots):
    done, per = eng.done()
    return [int(per[b]) for b in slots], [bool(done[b]) for b in slots]


def test_a_held_slot_does_not_stall_the_others(gpu_lib, engines):
    on, off, pad = engines
    rng = np.random.default_rng(401)
    p, q = _prefixes(rng, [8, 11])
    rows = _rows(rng, 10)
    F = 14
    utts = {0: (q, SlotParams(max_frames=F), None), 2: (p, SlotParams(max_frames=F, text_stream=True), rows)}
    ref = _reference(off, 4, utts)
    _admit(on, 4, utts)
    on.push_text(2, rows[:3])
    assert on.run(8) == 8                                    # (without the hold: 3, the batch stalls)
    assert _frames(on, [0, 2]) == ([8, 3], [False, False])
    assert list(on.text_state()[1]) == [False, False, True, False]
    assert on.run(8) == 6                                    # slot 0 ends at its budget; slot 2 is where it was
    per, done = _frames(on, [0, 2])
    assert per == [14, 3] and done == [True, False]
    assert list(on.held_steps()) == [0, 0, 11, 0]
    assert on.run(8) == 0                                    # every live slot is held
    on.push_text(2, rows[3:], final=True, n_text=10)
    _finish(on)
    np.testing.assert_array_equal(_column(on, 0), ref[0])
    np.testing.assert_array_equal(_column(on, 2), ref[2])
    assert ref[2].shape == (F, 16) and ref[0].shape == (F, 16)


@pytest.mark.parametrize("sampled", [False, True])
def test_codes_depend_on_the_text_and_on_nothing_about_arrival_for_every_slot(gpu_lib, engines, sampled):
    on, off, pad = engines
    rng = np.random.default_rng(402)
    p, q, r = _prefixes(rng, [8, 14, 10])
    rows, rows2 = _rows(rng, 9), _rows(rng, 12)
    F = 14
    kw = dict(seed=77, **SAMPLED) if sampled else {}
    S = SlotParams(max_frames=F, text_stream=True, **kw)
    S2 = SlotParams(max_frames=F, text_stream=True, **(dict(seed=78, **SAMPLED) if sampled else {}))
    other = SlotParams(max_frames=24, seed=5, **SAMPLED)    # a sampled ordinary slot that outlives every hold below

    def check(utts):
        ref = _reference(off, 17, utts)
        for b in utts:
            np.testing.assert_array_equal(_column(on, b), ref[b], err_msg=f"slot {b}")
        return ref

    for slot, beside in ((0, 16), (16, 3)):                  # the first tile, then the second 16-row tile
        # single steps: held at frame 1 for 1 step, in the middle for 2, just before the final row for 9
        utts = {slot: (p, S, rows), beside: (q, other, None)}
        _admit(on, 17, utts)
        on.push_text(slot, rows[:1])
        for k, (n_steps, push) in enumerate([(1, None), (1, rows[1:4]), (3, None), (2, rows[4:8]), (4, None), (9, None)]):
            for _ in range(n_steps):
                assert on.run(1) == 1, k
            if push is not None:
                on.push_text(slot, push)
        assert _frames(on, [slot, beside])[0] == [8, 20]
        assert int(on.held_steps()[slot]) == 12
        on.push_text(slot, rows[8:], final=True, n_text=9)
        _finish(on)
        ref = check(utts)
        assert ref[slot].shape == (F, 16)
        # one run over unheld and held steps
        _admit(on, 17, utts)
        on.push_text(slot, rows[:3])
        assert on.run(8) == 8
        assert _frames(on, [slot, beside])[0] == [3, 8]
        on.push_text(slot, rows[3:], final=True, n_text=9)
        _finish(on)
        check(utts)
    # two text slots held at different frames of one run, a sampled ordinary slot beside them
    utts = {0: (p, S, rows), 16: (r, S2, rows2), 3: (q, other, None)}
    _admit(on, 17, utts)
    on.push_text(0, rows[:2])
    on.push_text(16, rows2[:5])
    assert on.run(8) == 8
    assert _frames(on, [0, 16, 3])[0] == [2, 5, 8]
    assert [int(x) for x in on.held_steps()[[0, 16, 3]]] == [6, 3, 0]
    on.push_text(16, rows2[5:], final=True, n_text=12)
    assert on.run(2) == 2                                    # slot 16 goes on, slot 0 is still held
    on.push_text(0, rows[2:], final=True, n_text=9)
    _finish(on)
    check(utts)


@pytest.mark.parametrize("k", [1, 5])
def test_a_held_step_is_a_no_op_for_the_held_row(gpu_lib, engines, k):
    on, off, pad = engines
    rng = np.random.default_rng(403)
    p, q = _prefixes(rng, [9, 12])
    rows = _rows(rng, 8)
    T = SlotParams(max_frames=14, text_stream=True, seed=9, **SAMPLED)
    utts = {0: (q, SlotParams(max_frames=24), None), 1: (p, T, rows)}
    _admit(on, 4, utts)
    on.push_text(1, rows[:4])
    assert on.run(4) == 4
    hid, col, other = on.hidden()[1].copy(), _column(on, 1), on.hidden()[0].copy()
    assert col.shape == (4, 16) and int(on.held_steps()[1]) == 0
    assert on.run(k) == k
    np.testing.assert_array_equal(on.hidden()[1], hid)       # bit for bit
    assert not np.array_equal(on.hidden()[0], other)         # (the ordinary row did step)
    np.testing.assert_array_equal(_column(on, 1), col)
    codes, per = on.codes()
    assert int(per[1]) == 4 and int(per[0]) == 4 + k
    assert (codes[4:, 1, :] == -1).all()                     # nothing recorded past the row's last frame
    assert int(on.held_steps()[1]) == k
    on.push_text(1, rows[4:], final=True, n_text=8)
    _finish(on)
    ref = _reference(off, 4, utts)
    np.testing.assert_array_equal(_column(on, 1), ref[1])
    np.testing.assert_array_equal(_column(on, 0), ref[0])


def test_hold_on_and_never_held_equals_hold_off(gpu_lib, engines):
    on, off, pad = engines
    rng = np.random.default_rng(404)
    p, q, r = _prefixes(rng, [8, 13, 10])
    utts = {0: (p, SlotParams(max_frames=14, text_stream=True, seed=3, **SAMPLED), _rows(rng, 9)),
            1: (q, SlotParams(max_frames=12, seed=4, **SAMPLED), None),
            16: (r, SlotParams(max_frames=10, text_stream=True), _rows(rng, 10))}
    ref = _reference(off, 17, utts)
    got = _reference(on, 17, utts)
    assert not on.held_steps().any()
    for b in utts:
        np.testing.assert_array_equal(got[b], ref[b])


def test_edges(gpu_lib, engines):
    on, off, pad = engines
    rng = np.random.default_rng(405)
    p, q = _prefixes(rng, [8, 11])
    rows = _rows(rng, 16)
    F = 12
    T, O = SlotParams(max_frames=F, text_stream=True), SlotParams(max_frames=F)
    # every live slot held: no step
    _admit(on, 4, {1: (p, T, rows)})
    on.push_text(1, rows[:2])
    assert on.run(8) == 2 and on.run(8) == 0
    assert int(on.held_steps()[1]) == 0                      # (a step that was not run holds nobody)
    # a text slot without a frame and without a row stalls the batch, also beside a live ordinary slot
    utts = {0: (q, O, None), 1: (p, T, rows[:6])}
    ref = _reference(off, 4, utts)
    _admit(on, 4, utts)
    assert on.run(8) == 0
    assert list(on.text_state()[1]) == [False, True, False, False]
    on.push_text(1, rows[:1])                                # one row releases it: a step of its own, then it is held
    assert on.run(8) == 8
    assert _frames(on, [0, 1])[0] == [8, 1]
    # a held slot released: the loop goes on, the slot is reusable
    on.release([1])
    assert on.run(2) == 2
    on.admit([1], [p], [0], [T])
    on.push_text(1, rows[:6], final=True, n_text=6)
    _finish(on)
    np.testing.assert_array_equal(_column(on, 0), ref[0])
    np.testing.assert_array_equal(_column(on, 1), ref[1])
    # a text slot whose budget equals its rows ends at its budget, never held
    T5 = SlotParams(max_frames=5, text_stream=True)
    utts = {0: (q, O, None), 2: (p, T5, rows[:5])}
    ref = _reference(off, 4, utts)
    _admit(on, 4, utts)
    on.push_text(2, rows[:5])
    assert on.run(8) == 8
    per, done = _frames(on, [0, 2])
    assert per == [8, 5] and done == [False, True]
    assert not on.held_steps().any()
    _finish(on)
    np.testing.assert_array_equal(_column(on, 2), ref[2])
    np.testing.assert_array_equal(_column(on, 0), ref[0])


def test_a_final_push_without_rows_lifts_the_hold_and_the_eos_mask(gpu_lib, engines):
    on, off, pad = engines
    rng = np.random.default_rng(406)
    p, q = _prefixes(rng, [8, 10])
    rows = _rows(rng, 16)
    T = SlotParams(max_frames=24, text_stream=True)
    # slot 1 keeps the loop stepping: its text stays open (EOS masked), 16 rows
    # hold off, the rows at admission and the same final push after the same three frames: 3 rows, then pad rows under the
    # EOS rules of a 1-token text
    off.open(4, ignore_eos=False)
    off.admit([0], [p], [2], [T])
    off.push_text(0, rows[:3])
    assert off.run(8) == 3
    off.push_text(0, rows[:0], final=True, n_text=1)
    _finish(off)
    ref = {0: _column(off, 0)}
    on.open(4, ignore_eos=False)
    on.admit([0, 1], [p, q], [2, 2], [T, T])
    on.push_text(0, rows[:3])
    on.push_text(1, rows[:16])
    assert on.run(5) == 5
    per, done = _frames(on, [0, 1])
    assert per == [3, 5] and done == [False, False]          # held, and never ended while its text was open
    on.push_text(0, rows[:0], final=True, n_text=1)
    assert not on.text_state()[1][0]
    assert on.run(8) == 8
    per, done = _frames(on, [0, 1])
    # after the push: pad rows, and the rule forces EOS once progress = np / 3 > 2 (test_eos_rules_wait_for_the_final_push)
    assert done[0] and 3 <= per[0] <= 7, per
    assert not done[1] and per[1] == 13
    assert int(on.held_steps()[0]) == 2
    np.testing.assert_array_equal(_column(on, 0), ref[0])


def test_refusals_change_nothing(gpu_lib, world):
    path, cfg, tensors = world
    rng = np.random.default_rng(407)
    p, q = _prefixes(rng, [8, 11])
    pad = _rows(rng, 1)[0]
    rows = _rows(rng, 8)
    F = 10
    utts = {0: (q, SlotParams(max_frames=F), None), 1: (p, SlotParams(max_frames=F, text_stream=True), rows)}
    eng = _engine(path, pad, reserve=0)
    with pytest.raises(ValueError):
        eng.hold_text()                                      # no reservation
    eng.reserve_text(8)
    ref = _reference(eng, 4, utts)

    def stalls():                                            # the default mode's behaviour, and the reference's codes
        _admit(eng, 4, utts)
        eng.push_text(1, rows[:3])
        assert eng.run(8) == 3
        assert _frames(eng, [0, 1])[0] == [3, 3]
        eng.push_text(1, rows[3:], final=True, n_text=8)
        _finish(eng)
        for b in utts:
            np.testing.assert_array_equal(_column(eng, b), ref[b])

    stalls()
    with pytest.raises(ValueError):
        eng.hold_text()                                      # a per-slot batch is open
    stalls()
    assert not eng.held_steps().any()
    eng.destroy()


# ---- batch_server --concurrent --text_hold, end to end ----

from tests.test_gpu_concurrent import LONG, _call, _stop, packs  # noqa: E402,F401 -- (packs: the fixture)
from tests.test_gpu_text_stream import _text_call  # noqa: E402


def _hold_server(packs, sock):
    import os
    import threading
    import time

    from qwen3_tts_axera_russian_amd import batch_server as bs
    main, voc = packs
    srv = bs.BatchSynthesisServer(main, voc, sock, max_batch=4, n_ctx=160, max_tokens=80, temperature=0.0,
                                  cp_temperature=0.0, install_signal_handlers=False, concurrent=True, text_hold=True,
                                  text_wait_ms=5000.0)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    for _ in range(400):
        if os.path.exists(sock) and srv.sched is not None:
            break
        time.sleep(0.05)
    return srv, th


def test_server_text_hold_costs_the_other_request_nothing_and_changes_no_reply(gpu_lib, packs, tmp_path):
    import threading
    text = LONG[:18]
    ordinary = dict(token_ids=[LONG, [301, 302, 303, 304, 305, 306]], max_tokens=80, stream=True)
    sock = str(tmp_path / "th_a.sock")
    srv, th = _hold_server(packs, sock)
    got, beside = {}, []
    try:
        sched = srv.sched
        inner = sched._check_held

        def spy(ran):                                        # a starved check while an ordinary request holds a slot?
            before = sched.starved_checks
            out = inner(ran)
            if sched.starved_checks > before and any(o is not None and o[0].feed is None for o in sched._owner):
                beside.append(ran)
            return out
        sched._check_held = spy

        def client():
            got["ordinary"] = _call(sock, ordinary)
        t = threading.Thread(target=client)
        t.start()
        got["text"] = _text_call(sock, [text[:2], text[2:3], text[3:9], [], text[9:]], 0.01, max_tokens=40)
        t.join(timeout=120)
        assert "ordinary" in got
        held, starved = sched.held_steps, sched.starved_checks
    finally:
        _stop(srv, th)
    sock = str(tmp_path / "th_b.sock")
    srv, th = _hold_server(packs, sock)
    try:
        whole = _text_call(sock, [text], 0.0, max_tokens=40)
        alone = _call(sock, ordinary)
    finally:
        _stop(srv, th)
    print("held steps", held, "starved checks", starved, "of them beside the ordinary request", len(beside))
    assert held > 0
    assert not beside
    assert 1 <= got["text"][0].shape[0] <= 40
    np.testing.assert_array_equal(got["text"][0], whole[0])
    np.testing.assert_array_equal(got["text"][1], whole[1])
    assert len(alone) == len(got["ordinary"]) == 2
    for (c, pc), (rc, rp) in zip(got["ordinary"], alone):
        np.testing.assert_array_equal(c, rc)
        np.testing.assert_array_equal(pc, rp)
