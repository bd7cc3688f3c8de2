"""The small kernels that move a residual row between the tested pieces, one launch each against tests/row_ref.py:
final_norm_kernel, gather_embed_kernel, feedback_kernel, prompt_rows_kernel and prefix_move_kernel, through the hooks
q3t_final_norm_case / q3t_gather_embed_case / q3t_feedback_case / q3t_prompt_rows_case / q3t_prefix_move_case.

Buffers have 40 rows (two and a half 16-row fragment blocks); H = 1024 is the width the product runs, H = 96 has three
32-k blocks, 6 partials and 24 float4 per row (most lanes idle, the quad reduction of the stored partials on partly
filled waves).  Rows are bit-equal to the reference wherever the operation is a copy or a sequential f32 sum; the final
norm is inside a bound counted from its roundings (row_ref.final_norm_bound; the test prints the worst error / bound).
Every hook fills its outputs with NaN guards over the 16-row-padded extent and answers -3 when a word outside the rows
the launch owns changed."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import row_ref as RR
from tests import sample_cases as SC
from tests import sample_ref as SR

pytestmark = pytest.mark.gpu

ROWS = 40
SENT = np.float32(777.0)
SENT16 = 0x1234


def _f(a):
    return None if a is None else hiplib.fptr(a)


def _i(a):
    return None if a is None else hiplib.iptr(a)


def _u16(a):
    return None if a is None else a.ctypes.data_as(hiplib.u16p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gamma(rng, H):
    return (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)


def _row_outputs(rows, H, with_xh):
    return (np.full((rows, H), SENT, np.float32), np.full((rows, H // 16), SENT, np.float32),
            np.full((rows, H), SENT16, np.uint16) if with_xh else None)


def _check_rows(h, ssq, xh, gamma, want, what):
    """Rows `want` (dict row -> expected f32 row) bit-equal, their ssq / xh as stored rows; every other row untouched."""
    for r in range(h.shape[0]):
        if r not in want:
            assert (h[r] == SENT).all() and (ssq[r] == SENT).all() and (xh is None or (xh[r] == SENT16).all()), f"{what}: row {r} written"
            continue
        np.testing.assert_array_equal(_bits(h[r]), _bits(want[r]), err_msg=f"{what}: h row {r}")
        RR.check_stored_row(h[r], ssq[r], None if xh is None else xh[r], gamma, f"{what}: row {r}")


# ---- final norm ----------------------------------------------------------------------------------------------------------
def run_final_norm(lib, h, ssq, gamma, eps, R, row0, row_map=None, src_off=0, f16=False, copy=False, off=0, copy_gamma=None):
    rows, H = h.shape
    out = dict(f32=np.full((rows, H), SENT, np.float32))
    if f16:
        out["f16"] = np.full((rows, H), SENT16, np.uint16)
    if copy:
        out["copy"], out["copy_ssq"], out["copy_xh"] = _row_outputs(rows, H, copy_gamma is not None)
    rc = lib.q3t_final_norm_case(_f(h), _f(ssq), rows, H, H // 16, _f(gamma), eps, R, row0, _i(row_map), src_off, 1, int(f16),
                                 int(copy), off, _f(copy_gamma), _f(out["f32"]), _u16(out.get("f16")), _f(out.get("copy")),
                                 _f(out.get("copy_ssq")), _u16(out.get("copy_xh")))
    return rc, out


@pytest.mark.parametrize("H", [96, 1024])
def test_final_norm(test_lib, H):
    """Output rows (row0, R), source rows by src_off or by a row_map that permutes, repeats and reaches the last row, every
    subset of outputs a caller uses.  The ssq partials are NOT the sums of squares of h: a kernel that read another row's
    partials, or recomputed them, would miss the bound.  Rows 7 and 39 are scaled beyond the fp16 range."""
    rng = SC.rng_for("final_norm", H)
    eps = 1e-6
    h = (rng.standard_normal((ROWS, H)) * 10.0 ** rng.uniform(-3, 3, (ROWS, 1))).astype(np.float32)
    ssq = (16.0 * rng.uniform(0.2, 3.0, (ROWS, H // 16)) * 10.0 ** rng.uniform(-2, 2, (ROWS, 1))).astype(np.float32)
    gamma, copy_gamma = _gamma(rng, H), _gamma(rng, H)
    for r in (7, 39):
        h[r] = (1.0 + rng.random(H)) * 1e7 * rng.choice([-1.0, 1.0], H)
        ssq[r] = rng.uniform(0.5, 2.0, H // 16)
    row_map = rng.permutation(ROWS).astype(np.int32)
    row_map[[0, 5, 16]] = ROWS - 1                       # repeats, and every launch reaches the last row
    row_map[6] = 7
    worst, ran, saturated = 0.0, set(), 0
    for row0, R in ((0, 1), (5, 13), (16, 24), (0, 40)):
        for source in ("off0", "off3", "map"):
            for outputs in ("f32", "f16", "copy0", "copy16", "copy-5"):
                src_off = 3 if source == "off3" else 0
                rmap = row_map if source == "map" else None
                copy, off = outputs.startswith("copy"), int(outputs[4:] or 0) if outputs.startswith("copy") else 0
                src = [int(rmap[r]) if rmap is not None else r + src_off for r in range(row0, row0 + R)]
                valid = max(src) < ROWS and (not copy or (row0 + off >= 0 and row0 + R + off <= ROWS))
                rc, out = run_final_norm(test_lib, h, ssq, gamma, eps, R, row0, rmap, src_off, f16=outputs != "f32", copy=copy,
                                         off=off, copy_gamma=copy_gamma if copy and source != "off0" else None)
                what = f"rows ({row0}, {R}) {source} {outputs}"
                if not valid:                           # a row outside the buffers: the hook launches nothing
                    assert rc == -2, what
                    continue
                assert rc == 0, f"{what}: {rc}"
                ran.add((row0, source, outputs))
                for i, r in enumerate(range(row0, row0 + R)):
                    o = RR.final_norm_ref(h[src[i]], ssq[src[i]], gamma, eps, H)
                    err = np.abs(out["f32"][r].astype(np.float64) - o)
                    ratio = float((err / RR.final_norm_bound(o, H // 16)).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, f"{what}: out_f32 row {r} (source {src[i]}) error / bound {ratio}"
                    if "f16" in out:
                        got = out["f16"][r].view(np.float16).astype(np.float64)
                        want = RR.f16_of(o)
                        assert (np.abs(got - want) <= SR.fp16_ulp(want)).all(), f"{what}: out_f16 row {r}"
                        if src[i] in (7, 39):
                            np.testing.assert_array_equal(got, np.sign(o) * 65504.0, err_msg=f"{what}: saturation, row {r}")
                            saturated += 1
                    if copy:
                        np.testing.assert_array_equal(_bits(out["copy"][r + off]), _bits(out["f32"][r]), err_msg=f"{what}: copy of row {r}")
                        RR.check_stored_row(out["copy"][r + off], out["copy_ssq"][r + off],
                                            None if out["copy_xh"] is None else out["copy_xh"][r + off], copy_gamma, f"{what}: copy of row {r}")
                own = set(range(row0, row0 + R))
                for r in set(range(ROWS)) - own:
                    assert (out["f32"][r] == SENT).all() and ("f16" not in out or (out["f16"][r] == SENT16).all()), f"{what}: row {r} written"
                if copy:
                    for r in set(range(ROWS)) - {x + off for x in own}:
                        assert (out["copy"][r] == SENT).all() and (out["copy_ssq"][r] == SENT).all(), f"{what}: copy row {r} written"
                        assert out["copy_xh"] is None or (out["copy_xh"][r] == SENT16).all()
    print(f"final_norm H={H}: worst error / bound {worst:.3f} over {len(ran)} launches")
    assert {s for _, s, _ in ran} == {"off0", "off3", "map"} and {o for _, _, o in ran} == {"f32", "f16", "copy0", "copy16", "copy-5"}
    assert {r for r, _, _ in ran} == {0, 5, 16} and saturated > 0 and worst > 0.0


def test_final_norm_hook_refuses_what_no_caller_passes(test_lib):
    H = 96
    h, ssq, g = np.ones((ROWS, H), np.float32), np.ones((ROWS, H // 16), np.float32), np.ones(H, np.float32)
    assert run_final_norm(test_lib, h, ssq, g, 1e-6, 24, 17)[0] == -2                    # rows beyond the buffer
    assert run_final_norm(test_lib, h, ssq, g, 1e-6, 8, 0, src_off=-1)[0] == -2
    assert run_final_norm(test_lib, h, ssq, g, 1e-6, 8, 0, row_map=np.full(ROWS, ROWS, np.int32))[0] == -2
    out = np.zeros((ROWS, H), np.float32)
    assert test_lib.q3t_final_norm_case(_f(h), _f(ssq), ROWS, H, H // 32, _f(g), 1e-6, 8, 0, None, 0, 1, 0, 0, 0, None, _f(out),
                                        None, None, None, None) == -2                     # parts != H / 16


# ---- gather --------------------------------------------------------------------------------------------------------------
def run_gather(lib, table, tok, tok_stride, n_frames, frame_cap, col, forced, R, row0, gamma):
    V, H = table.shape
    h, ssq, xh = _row_outputs(ROWS, H, gamma is not None)
    rc = lib.q3t_gather_embed_case(_f(table), V, H, _i(tok), tok_stride, _i(n_frames), frame_cap, col, _i(forced), R, row0, ROWS,
                                   _f(gamma), _f(h), _f(ssq), _u16(xh))
    return rc, h, ssq, xh


@pytest.mark.parametrize("H", [96, 1024])
def test_gather_embed(test_lib, H):
    V, cap = 50, 4
    rng = SC.rng_for("gather_embed", H)
    table = (rng.standard_normal((V, H)) * 10.0 ** rng.uniform(-3, 3, (V, 1))).astype(np.float32)
    gamma = _gamma(rng, H)
    kinds = set()
    # the `tok` form: row r reads tok[r * tok_stride]
    for stride in (1, 16):
        for row0, R in ((0, ROWS), (5, 13)):
            tok = rng.integers(0, V, ROWS * stride).astype(np.int32)
            ids = np.array([(int(rng.integers(0, V)), -1, V, V + 7)[r % 4] for r in range(ROWS)], np.int32)
            tok[::stride] = ids
            g = gamma if row0 else None
            rc, h, ssq, xh = run_gather(test_lib, table, tok, stride, None, 0, 0, None, R, row0, g)
            assert rc == 0
            _check_rows(h, ssq, xh, g, {r: SR.gather_row(table, int(ids[r])) for r in range(row0, row0 + R)}, f"tok stride {stride}")
    # the `codes` form: column col of the row's current frame
    n_frames = np.array([(0, 1, cap, cap + 3)[r % 4] for r in range(ROWS)], np.int32)
    for col in (0, 5, 15):
        for with_forced in (0, 1):
            for row0, R in ((0, ROWS), (5, 13)):
                codes = rng.integers(0, V, (cap, ROWS, 16)).astype(np.int32)
                codes[:, rng.random(ROWS) < 0.3, col] = -1
                codes[:, rng.random(ROWS) < 0.2, col] = V + 2
                forced = None
                if with_forced:
                    forced = np.full_like(codes, -1)
                    pick = rng.random((cap, ROWS)) < 0.6
                    forced[:, :, col][pick] = rng.integers(0, V + 3, int(pick.sum()))
                g = gamma if col else None
                rc, h, ssq, xh = run_gather(test_lib, table, codes, 0, n_frames, cap, col, forced, R, row0, g)
                assert rc == 0
                want = {}
                for r in range(row0, row0 + R):
                    t = RR.gather_token(codes, n_frames, cap, col, forced, r)
                    want[r] = SR.gather_row(table, t)
                    f = min(max(int(n_frames[r]) - 1, 0), cap - 1)
                    if forced is not None and forced[f, r, col] >= 0:
                        kinds.add("not revived" if codes[f, r, col] < 0 else "forced beyond" if t >= V else "forced")
                    else:
                        kinds.add("own -1" if t < 0 else "own beyond" if t >= V else "own")
                _check_rows(h, ssq, xh, g, want, f"codes col {col} forced {with_forced}")
    assert kinds == {"not revived", "forced beyond", "forced", "own -1", "own beyond", "own"}


# ---- feedback ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [96, 1024])
def test_feedback(test_lib, H):
    TV, CV = 30, 20
    rng = SC.rng_for("feedback kernel", H)
    temb = rng.standard_normal((TV, H), dtype=np.float32)
    tabs = rng.standard_normal((15, CV, H), dtype=np.float32)
    pad, gamma = rng.standard_normal(H, dtype=np.float32), _gamma(rng, H)
    for R in (1, 17):
        for n_groups in (1, 15):
            for p in (None, pad):
                codes = rng.integers(-1, TV + 5, (R, 16)).astype(np.int32)      # in range, -1, beyond each vocabulary
                if R > 1:
                    codes[:4, 0], codes[:4, 1] = (-1, TV, TV + 4, 0), (CV, -1, 0, CV + 9)
                g = gamma if p is not None else None
                h, ssq, xh = _row_outputs(R, H, g is not None)
                rc = test_lib.q3t_feedback_case(_i(codes), R, _f(temb), TV, _f(np.ascontiguousarray(tabs[:n_groups])), CV, n_groups,
                                                _f(p), H, _f(g), _f(h), _f(ssq), _u16(xh))
                assert rc == 0
                want = {r: SR.feedback_row(codes[r], temb, list(tabs[:n_groups]), p) for r in range(R)}
                _check_rows(h, ssq, xh, g, want, f"R {R} groups {n_groups} pad {p is not None}")


# ---- codec prompt --------------------------------------------------------------------------------------------------------
def run_prompt_rows(lib, codes, T, temb, tabs, pad, H, row0, gamma, with_h=True, max_rows=None, n_groups=15, null_table=0):
    buf_rows = (row0 + T + 15) // 16 * 16
    past, n_past = np.full(32, -7, np.int32), np.full(1, -7, np.int32)
    h, ssq, xh = _row_outputs(buf_rows, H, gamma is not None)
    rc = lib.q3t_prompt_rows_case(_i(codes), T, _i(past), _i(n_past), _f(temb), temb.shape[0], _f(tabs), tabs.shape[0], tabs.shape[1],
                                  n_groups, _f(pad), H, row0, buf_rows if max_rows is None else max_rows, buf_rows, int(with_h),
                                  _f(gamma) if with_h else None, _f(h) if with_h else None, _f(ssq) if with_h else None,
                                  _u16(xh) if with_h else None, null_table)
    return rc, past, n_past, h, ssq, xh


@pytest.mark.parametrize("H", [96, 1024])
def test_prompt_rows(test_lib, H):
    TV, CV = 30, 20
    rng = SC.rng_for("prompt rows", H)
    temb = rng.standard_normal((TV, H), dtype=np.float32)
    tabs = rng.standard_normal((15, CV, H), dtype=np.float32)
    pad, gamma = rng.standard_normal(H, dtype=np.float32), _gamma(rng, H)
    for T in (1, 31, 32, 33, 70):
        codes = rng.integers(0, CV, (T, 16)).astype(np.int32)
        codes[:, 0] = rng.integers(0, TV, T)
        ring, n = RR.prompt_ring(np.full(32, -7, np.int32), codes, T)
        assert (ring == -7).sum() == 32 - min(T, 32)
        for row0 in (0, 9):
            g = gamma if row0 else None
            rc, past, n_past, h, ssq, xh = run_prompt_rows(test_lib, codes, T, temb, tabs, pad, H, row0, g)
            assert rc == 0, f"T {T} row0 {row0}: {rc}"
            np.testing.assert_array_equal(past, ring, err_msg=f"ring, T {T}")
            assert n_past[0] == n == T
            want = {row0 + i: SR.feedback_row(codes[i], temb, list(tabs), pad) for i in range(T)}
            _check_rows(h, ssq, xh, g, want, f"T {T} row0 {row0}")
        # h = null (a prefix-cache hit): only the ring and the counter change (the hook's guards cover h / ssq / xh)
        rc, past, n_past, h, ssq, xh = run_prompt_rows(test_lib, codes, T, temb, tabs, pad, H, 0, None, with_h=False)
        assert rc == 0
        np.testing.assert_array_equal(past, ring)
        assert n_past[0] == T and (h == SENT).all() and (ssq == SENT).all()
    # refusals: -1, and nothing changes (ring, counter, and every guard of the row buffers)
    T, row0 = 33, 9
    codes = rng.integers(0, CV, (T, 16)).astype(np.int32)
    for kw in (dict(max_rows=row0 + T - 1), dict(n_groups=16), dict(n_groups=0), dict(null_table=1), dict(null_table=2)):
        rc, past, n_past, h, ssq, xh = run_prompt_rows(test_lib, codes, T, temb, tabs, pad, H, row0, gamma, **kw)
        assert rc == -1, kw
        assert (past == -7).all() and n_past[0] == -7 and (h == SENT).all() and (ssq == SENT).all() and (xh == SENT16).all()
    rc = run_prompt_rows(test_lib, codes, T, temb, tabs, pad, H, row0, gamma, max_rows=row0 + T)[0]
    assert rc == 0                                        # the exact fit is served


# ---- prefix cache --------------------------------------------------------------------------------------------------------
L, KV, SLOTS, ENTRIES = 2, 2, 3, 2


def _prefix_buffers(rng, n_ctx, max_rows, H):
    u16 = lambda *shape: rng.integers(0, 65536, shape, dtype=np.uint16)
    return dict(kc=u16(L, SLOTS, KV, n_ctx, 128), vc=u16(L, SLOTS, KV, n_ctx, 128), pool=u16(ENTRIES, L, 2, KV, max_rows, 128),
                states=rng.standard_normal((ENTRIES, H + H // 16), dtype=np.float32), h=rng.standard_normal((max_rows, H), dtype=np.float32),
                ssq=rng.standard_normal((max_rows, H // 16), dtype=np.float32))


def run_prefix_move(lib, b, entry, launch):
    """-> (rc, buffers after the call); b stays as it is."""
    o = {k: np.array(v, copy=True) for k, v in b.items()}
    n_ctx, max_rows, H = b["kc"].shape[3], b["pool"].shape[4], b["h"].shape[1]
    rc = lib.q3t_prefix_move_case(_u16(o["kc"]), _u16(o["vc"]), L, SLOTS, KV, n_ctx, _u16(o["pool"]), ENTRIES, max_rows, _f(o["states"]),
                                  _f(o["h"]), _f(o["ssq"]), max_rows, H, entry, _i(np.array(launch, np.int32)))
    return rc, o


def _launch(b, slot, n_rows, h_row, restore, over=()):
    d = dict(n_layers=L, n_kv=KV, n_ctx=b["kc"].shape[3], max_rows=b["pool"].shape[4], H=b["h"].shape[1], slot=slot, n_rows=n_rows,
             h_row=h_row, restore=restore, null=0)
    d.update(dict(over))
    return [d[k] for k in ("n_layers", "n_kv", "n_ctx", "max_rows", "H", "slot", "n_rows", "h_row", "restore", "null")]


def _same(got, want, what):
    for k, w in zip(("kc", "vc", "pool", "states", "h", "ssq"), want):
        a, b = got[k], np.asarray(w)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {k}")


@pytest.mark.parametrize("H", [96, 1024])
@pytest.mark.parametrize("n_ctx,max_rows,n_rows", [(48, 40, 1), (48, 40, 15), (48, 40, 16), (48, 40, 17), (48, 40, 40), (160, 130, 130)])
def test_prefix_move(test_lib, n_ctx, max_rows, n_rows, H):
    """Save slot 2 into entry 1, restore entry 1 into slot 0: rows [0, n_rows) of every (layer, K|V, head) run and the
    residual row with its partials move, bit for bit; everything else -- the rows behind n_rows, the other slots and
    entry, every other row of h -- stays (row_ref.prefix_move_ref over the whole of every buffer).  130 rows reach the
    grid cap of 8 workgroups per run."""
    b = _prefix_buffers(SC.rng_for("prefix", n_ctx, n_rows, H), n_ctx, max_rows, H)
    for h_row in (0, 21):
        rc, got = run_prefix_move(test_lib, b, 1, _launch(b, 2, n_rows, h_row, 0))
        assert rc == 0, f"save: {rc}"
        want = RR.prefix_move_ref(b["kc"], b["vc"], b["pool"], b["states"], b["h"], b["ssq"], 2, 1, n_rows, h_row, 0)
        _same(got, want, f"save h_row {h_row}")
        assert not (want[2][1] == b["pool"][1]).all() and (want[2][0] == b["pool"][0]).all()
        rc, got = run_prefix_move(test_lib, b, 1, _launch(b, 0, n_rows, h_row, 1))
        assert rc == 0, f"restore: {rc}"
        want = RR.prefix_move_ref(b["kc"], b["vc"], b["pool"], b["states"], b["h"], b["ssq"], 0, 1, n_rows, h_row, 1)
        _same(got, want, f"restore h_row {h_row}")
        assert (want[0][:, 1:] == b["kc"][:, 1:]).all() and not (want[4][h_row] == b["h"][h_row]).all()


def test_prefix_move_refusals(test_lib):
    """Every refusal of launch_prefix_move: -1 and nothing changes."""
    H = 96
    b = _prefix_buffers(SC.rng_for("prefix refusals"), 48, 40, H)
    wide = _prefix_buffers(SC.rng_for("prefix refusals wide"), 48, 64, H)       # an entry longer than the context
    bad = [(b, dict(null=1 << i)) for i in range(6)]
    bad += [(b, dict(n_layers=0)), (b, dict(n_kv=0)), (b, dict(slot=-1)), (b, dict(n_rows=0)), (b, dict(n_rows=-3)),
            (b, dict(n_rows=41)), (wide, dict(n_rows=49)), (b, dict(h_row=-1)), (b, dict(H=0)), (b, dict(H=48))]
    for bufs, over in bad:
        for restore in (0, 1):
            rc, got = run_prefix_move(test_lib, bufs, 1, _launch(bufs, 2, 8, 3, restore, over))
            assert rc == -1, over
            _same(got, [bufs[k] for k in ("kc", "vc", "pool", "states", "h", "ssq")], f"refused {over}")
    rc, _ = run_prefix_move(test_lib, wide, 1, _launch(wide, 2, 48, 3, 0))       # n_rows = n_ctx is served
    assert rc == 0
    assert run_prefix_move(test_lib, b, 1, _launch(b, 3, 8, 3, 0))[0] == -2      # a slot the buffers do not have
