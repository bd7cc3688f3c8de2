"""Split-fp16 arithmetic of the carry-state incremental decode (voc_incr_set_arithmetic): opt-in per object, the same invariance
contract as the exact mode while no entry is redone, fp32-grade against the oracle (the exact mode's TOL), and a push that is a
transaction per entry -- an entry whose planes leave the fp16 range is decoded again on the exact kernels from its uncommitted
history, without touching its neighbours' bits.  An object that never switches is what it was."""
import numpy as np
import pytest
import torch

from oracle.voc_ref import voc_reference
from qwen3_tts_axera_russian_amd import weights as W
from tests.test_gpu_voc_incremental import TOL, Incr, Voc, full_table, run_pattern, samples_of, to_int16, write_tiny

pytestmark = pytest.mark.gpu

LENS = [1, 2, 7, 8, 9, 23, 24, 25, 63, 64, 65, 200]     # across the push size, the 24-frame attention window and the chunk
IRREGULAR = (3, 1, 17, 8, 64, 5, 2, 30)                 # frames per push, cycled


def set_arith(st, split):
    return st.lib.voc_incr_set_arithmetic(st.s, split)


def run_steps(st, prog, utts, steps, slots=None, i16=False, log=None):
    """run_pattern with a cycle of push sizes; log (a list) takes (pushed so far per utterance, last_redone, last_split) per push"""
    slots = list(range(len(utts))) if slots is None else slots
    got, fed = [[] for _ in utts], [0] * len(utts)
    for k in slots:
        st.reset(k)
    j = 0
    while any(fed[u] < len(c) for u, c in enumerate(utts)):
        step = steps[j % len(steps)]
        j += 1
        who = [u for u, c in enumerate(utts) if fed[u] < len(c)]
        entries = [(slots[u], utts[u][fed[u]:fed[u] + step], fed[u] + step >= len(utts[u])) for u in who]
        outs = st.push(entries, i16)
        for u, e, o in zip(who, entries, outs):
            fed[u] += len(e[1])
            got[u].append(o)
            assert sum(len(x) for x in got[u]) == samples_of(prog, fed[u])
        if log is not None:
            log.append((list(fed), st.lib.voc_incr_last_redone(st.s), st.lib.voc_incr_last_split_launches(st.s)))
    return [np.concatenate(g) for g in got]


def table_device_bytes(prog, chunk, max_batch, max_streams, state_bytes):
    """What voc_incr_create allocates, from the table alone: the carried state of every stream, three work buffers and the k | v
    buffer sized for the largest activation [history | new] of a push of `chunk` frames (first push or later) x max_batch entries
    (rows at a pitch of 32 floats, + 1024 floats of slack each), the codes, the per-op meta rows, the output offsets and the f32
    and int16 packed outputs of max_streams entries."""
    prog = [[int(x) for x in row] for row in np.asarray(prog)]
    pitch = lambda L: (L + 31) & ~31

    def chain(n):
        cols, L = [], n
        for r in prog:
            cols.append(L)
            if r[0] == W.VOP_CONVT:
                L = max(0, L * r[4] - r[6])
        return cols + [L]
    need = need_kv = 0
    for prev in (0, chunk):
        nc = [y - x for x, y in zip(chain(prev), chain(prev + chunk))]
        n, skip, C = nc[0], 0, 0
        for i, r in enumerate(prog):
            if n == 0:
                break
            op = r[0]
            if op in (W.VOP_RVQ, W.VOP_EMBMEAN):
                cout, skip = (r[4] if op == W.VOP_RVQ else r[3]), 0
                need = max(need, cout * pitch(n))
            elif op == W.VOP_ATTN:
                cout = r[3] * r[4]
                need_kv = max(need_kv, 2 * cout * pitch(r[6] - 1 + n))
                need = max(need, cout * pitch(skip + n))
            else:
                cout = r[2]
                H = {W.VOP_CONV: (r[3] - 1) * r[4], W.VOP_CONVT: r[3] // max(r[4], 1) - 1, W.VOP_DWCONV: r[3] - 1}.get(op, 0)
                if H:
                    need, skip = max(need, C * pitch(H + n)), H
                if op == W.VOP_CONVT:
                    n, skip = nc[i + 1], 0
                    if n == 0:
                        break
                need = max(need, cout * pitch(skip + n))
            C = cout
    up = int(np.prod([r[4] for r in prog if r[0] == W.VOP_CONVT]))
    out_cap = max_streams * chunk * up
    return (max(4, state_bytes * max_streams) + 3 * 4 * (need * max_batch + 1024) + 4 * (need_kv * max_batch + 1024)
            + 8 * 16 * chunk * max_batch + 4 * (1 + len(prog)) * max_batch + 8 * max_batch + 4 * out_cap + 2 * out_cap)


def test_default_is_untouched(gpu_lib, tmp_path):
    """An object on which the arithmetic was never set and one set to 0: the same bits, no launch on the fp16 MFMA path, the
    same device allocation."""
    path, tens = write_tiny(tmp_path, "both")
    prog = tens["voc.program"]
    utts = [np.random.default_rng(3).integers(0, 2048, size=(n, 16)).astype(np.int64) for n in (30, 9, 70)]
    v = Voc(gpu_lib, path, 64, max_batch=5)
    a, b = Incr(v, 4), Incr(v, 4)
    try:
        assert gpu_lib.voc_incr_arithmetic(a.s) == 0
        assert set_arith(b, 0) == 0 and gpu_lib.voc_incr_arithmetic(b.s) == 0
        state = gpu_lib.voc_incr_state_bytes(a.s)
        # the default allocation is what the table asks for, for both: nothing of the split mode is in it
        assert gpu_lib.voc_incr_device_bytes(a.s) == gpu_lib.voc_incr_device_bytes(b.s) == table_device_bytes(prog, 64, 5, 4, state)
        ga = run_pattern(a, prog, utts, 8)
        assert gpu_lib.voc_incr_last_split_launches(a.s) == 0 and gpu_lib.voc_incr_last_redone(a.s) == 0
        gb = run_pattern(b, prog, utts, 8)
        assert gpu_lib.voc_incr_last_split_launches(b.s) == 0 and gpu_lib.voc_incr_last_redone(b.s) == 0
        for x, y in zip(ga, gb):
            np.testing.assert_array_equal(x, y)
        assert gpu_lib.voc_incr_device_bytes(a.s) == gpu_lib.voc_incr_device_bytes(b.s)
        # the switch grows the allocation once; the per-stream state keeps its size; back at 0 the bits are the default's
        before = gpu_lib.voc_incr_device_bytes(b.s)
        assert set_arith(b, 1) == 1 and gpu_lib.voc_incr_device_bytes(b.s) > before
        grown = gpu_lib.voc_incr_device_bytes(b.s)
        assert gpu_lib.voc_incr_state_bytes(b.s) == state
        assert set_arith(b, 0) == 0 and set_arith(b, 1) == 1 and gpu_lib.voc_incr_device_bytes(b.s) == grown
        assert set_arith(b, 0) == 0
        for x, y in zip(ga, run_pattern(b, prog, utts, 7)):
            np.testing.assert_array_equal(x, y)
        assert set_arith(b, 2) < 0 and gpu_lib.voc_incr_arithmetic(b.s) == 0
    finally:
        a.close()
        b.close()
        v.close()


def test_the_split_path_really_runs(gpu_lib, tmp_path):
    path, tens = write_tiny(tmp_path, "both")
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 2)
    try:
        assert set_arith(st, 1) == 1
        assert gpu_lib.voc_incr_arithmetic(st.s) == 1
        c = np.random.default_rng(4).integers(0, 2048, size=(8, 16)).astype(np.int64)
        out = st.push([(0, c, False)])[0]
        assert len(out) == samples_of(tens["voc.program"], 8) and np.isfinite(out).all()
        assert gpu_lib.voc_incr_last_split_launches(st.s) > 0
        assert gpu_lib.voc_incr_last_redone(st.s) == 0
    finally:
        st.close()
        v.close()


@pytest.mark.parametrize("trim", ["both", "right"])
def test_invariance_and_accuracy(gpu_lib, tmp_path, trim):
    """Split mode, 12 streams over a handle of max_batch 5: every push pattern, stream placement and neighbourhood gives the same
    bits, the int16 push is the int16 rule on the f32 push, and the joined samples are the oracle's whole decode within the exact
    mode's TOL.  Against a float64 evaluation of the same table the split and the exact incremental errors are printed side by
    side."""
    path, tens = write_tiny(tmp_path, trim)
    prog = tens["voc.program"]
    rng = np.random.default_rng(5)
    utts = [rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in LENS]
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, len(utts) + 3)
    ex = Incr(v, len(utts))
    try:
        assert set_arith(st, 1) == 1
        log = []
        base = run_steps(st, prog, utts, (64,), log=log)
        assert all(r == 0 for _, r, _ in log) and all(s > 0 for _, _, s in log)
        exact = run_pattern(ex, prog, utts, None)
        e_split = e_exact = 0.0
        for u, c in enumerate(utts):
            ref = voc_reference(tens, c[None])[0]
            assert base[u].shape == ref.shape
            err = float(np.abs(base[u] - ref).max())
            print(f"tiny {trim} N={LENS[u]}: split incremental max abs err vs the oracle's whole decode {err:.2e}")
            assert err < TOL, (LENS[u], err)
            ref64 = voc_reference(tens, c[None], dtype=np.float64)[0]
            e_split = max(e_split, float(np.abs(base[u] - ref64).max()))
            e_exact = max(e_exact, float(np.abs(exact[u] - ref64).max()))
        print(f"tiny {trim}: max err vs float64: incremental split {e_split:.2e}, incremental exact {e_exact:.2e}")
        for steps in ((1,), (8,), IRREGULAR, (48,)):
            log = []
            got = run_steps(st, prog, utts, steps, log=log)
            assert all(r == 0 for _, r, _ in log)
            for u in range(len(utts)):
                np.testing.assert_array_equal(got[u], base[u], err_msg=f"len {LENS[u]} steps {steps}")
        slots = [(7 * u + 2) % (len(utts) + 3) for u in range(len(utts))]       # permuted stream indices (7 is coprime to 15), reversed neighbours
        assert len(set(slots)) == len(slots)
        got = run_steps(st, prog, utts[::-1], (7,), slots=slots)
        for u in range(len(utts)):
            np.testing.assert_array_equal(got[len(utts) - 1 - u], base[u])
        np.testing.assert_array_equal(run_steps(st, prog, [utts[-1]], (8,), slots=[4])[0], base[-1])   # alone in its calls
        got16 = run_steps(st, prog, utts, (48,), i16=True)
        for u in range(len(utts)):
            np.testing.assert_array_equal(got16[u], to_int16(base[u]))
        # independent of the process-wide arithmetic
        for flag in (1, 0):
            gpu_lib.voc_set_exact_fp32(flag)
            np.testing.assert_array_equal(run_steps(st, prog, utts[-3:], (8,))[2], base[-1])
            assert gpu_lib.voc_incr_last_split_launches(st.s) > 0
    finally:
        gpu_lib.voc_set_exact_fp32(0)
        st.close()
        ex.close()
        v.close()


def test_mode_switch_rules(gpu_lib, tmp_path):
    """The arithmetic changes between utterances only: refused (<0, nothing changes) while a stream runs, accepted once every
    stream is finished or reset."""
    path, tens = write_tiny(tmp_path, "both")
    prog = tens["voc.program"]
    a = np.random.default_rng(6).integers(0, 2048, size=(40, 16)).astype(np.int64)
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 3)
    try:
        want_exact = run_pattern(st, prog, [a], 8)[0]              # (finished)
        assert set_arith(st, 1) == 1
        want_split = run_pattern(st, prog, [a], 8)[0]
        assert gpu_lib.voc_incr_last_split_launches(st.s) > 0
        assert set_arith(st, 0) == 0                               # every stream finished: accepted
        st.reset(1)
        head = st.push([(1, a[:16], False)])
        assert set_arith(st, 1) < 0 and gpu_lib.voc_incr_arithmetic(st.s) == 0     # stream 1 runs
        rest = st.push([(1, a[16:], True)])
        np.testing.assert_array_equal(np.concatenate(head + rest), want_exact)
        assert set_arith(st, 1) == 1                               # finished
        st.reset(2)
        head = st.push([(2, a[:16], False)])
        assert set_arith(st, 0) < 0 and gpu_lib.voc_incr_arithmetic(st.s) == 1
        rest = st.push([(2, a[16:], True)])
        np.testing.assert_array_equal(np.concatenate(head + rest), want_split)
        st.reset(0)
        st.push([(0, a[:5], False)])
        assert set_arith(st, 0) < 0
        st.reset(0)                                                # a reset makes it idle too
        assert set_arith(st, 0) == 0
        np.testing.assert_array_equal(run_pattern(st, prog, [a], 8, slots=[2])[0], want_exact)
    finally:
        st.close()
        v.close()


def plane_peaks(tens, codes):
    """the oracle's largest |value| a conv op reads (its Snake / GELU applied) -- what the split path writes as planes"""
    prog = np.asarray(tens["voc.program"])
    peak = 0.0
    for i, row in enumerate(prog):
        if int(row[0]) not in (W.VOP_CONV, W.VOP_CONVT) or int(row[1]) % 16:
            continue
        x = torch.from_numpy(voc_reference(tens, codes[None], n_ops=i))
        flags = int(row[5])
        if flags & W.VF_SNAKE:
            al, be = torch.from_numpy(np.array(tens[f"voc.op{i}.alpha"])), torch.from_numpy(np.array(tens[f"voc.op{i}.beta"]))
            x = x + torch.sin(torch.exp(al)[None, :, None] * x) ** 2 / (torch.exp(be)[None, :, None] + 1e-9)
        if flags & W.VF_GELU:
            x = torch.nn.functional.gelu(x)
        peak = max(peak, float(x.abs().max()))
    return peak


def test_per_entry_redo(gpu_lib, tmp_path):
    """One codebook row (entry 7 of the first quantiser) is scaled beyond the fp16 range and the first conv scales it back.
    Stream A uses that id in frame 12 only, stream B never: pushed together in steps of 8, exactly A's push of frames 8..15 is
    redone exactly, B's bits are those of B alone, A's earlier pushes are those of an A without the id, and A stays on the oracle.
    A weight beyond the fp16 range keeps its op exact: nothing is redone."""
    vc = W.tiny_full_voc_config()
    tens = {k: np.array(x) for k, x in W.make_synthetic_voc(vc, seed=7).items()}
    prog = tens["voc.program"]
    assert int(prog[0][0]) == W.VOP_RVQ and int(prog[1][0]) == W.VOP_CONV
    cb = tens["voc.op0.codebook"].copy()
    cb[0, 7] *= np.float32(3.0e5)
    tens["voc.op0.codebook"] = cb
    tens["voc.op1.weight"] = (tens["voc.op1.weight"] * 1.0e-6).astype(np.float32)
    path = str(tmp_path / "voc_row7.q3w")
    W.write_pack(path, {"voc_chunk": 64.0}, tens)
    rng = np.random.default_rng(9)
    N = 24
    b = rng.integers(0, 2048, size=(N, 16)).astype(np.int64)
    a_plain = rng.integers(0, 2048, size=(N, 16)).astype(np.int64)
    for c in (b, a_plain):
        c[c[:, 0] == 7, 0] = 8
    a = a_plain.copy()
    a[12, 0] = 7
    # the fixture tests what it claims: B (and A without the id) stay inside the fp16 range, A leaves it
    assert plane_peaks(tens, b) < 65504.0 and plane_peaks(tens, a_plain) < 65504.0 and plane_peaks(tens, a) > 65504.0
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 3)
    try:
        assert set_arith(st, 1) == 1
        log = []
        b_alone = run_steps(st, prog, [b], (8,), slots=[2], log=log)[0]
        assert [r for _, r, _ in log] == [0, 0, 0]
        log = []
        a_plain_got = run_steps(st, prog, [a_plain], (8,), log=log)[0]
        assert [r for _, r, _ in log] == [0, 0, 0]
        log = []
        a_got, b_got = run_steps(st, prog, [a, b], (8,), log=log)
        assert [r for _, r, _ in log] == [0, 1, 0], log        # exactly the push holding frame 12
        assert all(s > 0 for _, _, s in log)
        np.testing.assert_array_equal(b_got, b_alone)            # B never depended on its neighbour's overflow
        s8 = samples_of(prog, 8)
        np.testing.assert_array_equal(a_got[:s8], a_plain_got[:s8])   # A's push before the redo: the split bits
        ref = voc_reference(tens, a[None])[0]
        scale = float(np.abs(ref).max())
        err = float(np.abs(a_got - ref).max())
        print(f"redo: A max abs err vs the oracle {err:.2e} (signal {scale:.3f}); B vs its oracle "
              f"{float(np.abs(b_got - voc_reference(tens, b[None])[0]).max()):.2e}")
        assert np.isfinite(a_got).all() and scale > 0 and err < TOL * scale
        # other placements of the same two streams: the same bits (the redo is the same push)
        a2, b2 = run_steps(st, prog, [b, a], (8,), slots=[1, 2])[::-1]
        np.testing.assert_array_equal(a2, a_got)
        np.testing.assert_array_equal(b2, b_alone)
    finally:
        st.close()
        v.close()
    # a weight beyond the fp16 range: that op stays on the exact kernels, nothing is redone
    bigw = {k: np.array(x) for k, x in W.make_synthetic_voc(vc, seed=7).items()}
    w2 = bigw["voc.op2.weight"].copy()
    w2.flat[0] = 1.0e5
    bigw["voc.op2.weight"] = w2
    path = str(tmp_path / "voc_big_w.q3w")
    W.write_pack(path, {"voc_chunk": 64.0}, bigw)
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 2)
    try:
        assert set_arith(st, 1) == 1
        log = []
        got = run_steps(st, prog, [b], (8,), log=log)[0]
        assert [r for _, r, _ in log] == [0, 0, 0] and all(s > 0 for _, _, s in log)
        ref = voc_reference(bigw, b[None])[0]
        err = float(np.abs(got - ref).max())
        print(f"weight beyond fp16: max abs err vs the oracle {err:.2e} (signal {np.abs(ref).max():.3f})")
        assert err < TOL
    finally:
        st.close()
        v.close()


def test_full_size_table(gpu_lib):
    """The benchmark's vocoder (trim both): the 96- and 192-channel units run as two split convs, the long one-tap convs -- three
    streams in steps of 8, 64 and 1 give the same bits."""
    path, tens = full_table("both")
    prog = tens["voc.program"]
    rng = np.random.default_rng(22)
    lens = [9, 64, 70]
    utts = [rng.integers(0, 2048, size=(n, 16)).astype(np.int64) for n in lens]
    v = Voc(gpu_lib, path, 64, max_batch=5)
    st = Incr(v, 3)
    try:
        assert set_arith(st, 1) == 1
        log = []
        base = run_steps(st, prog, utts, (8,), log=log)
        assert all(r == 0 for _, r, _ in log) and all(s > 0 for _, _, s in log)
        for steps in ((64,), (1,)):
            got = run_steps(st, prog, utts, steps)
            for u in range(len(utts)):
                np.testing.assert_array_equal(got[u], base[u], err_msg=f"len {lens[u]} steps {steps}")
    finally:
        st.close()
        v.close()
