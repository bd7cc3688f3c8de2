"""Every attention kernel variant against the float64 restatement of its contract (tests/attn_ref.py), one launch at a time
through the test hooks q3t_attn / q3t_voc_attn (csrc/q3_test_api.hip).

Talker / code-predictor attention (launch_attn), per case:
  * cache: the appended K / V rows are within 1 fp16 ulp of the reference (or, for entries far below their row's scale,
    within the f32 arithmetic's own absolute error, 2^-21 of the row's largest value) and >= 99 % bit-equal; every other entry
    (other slots, positions at or past a row's limit, padding rows' targets) is unchanged bit for bit;
  * output: against the reference computed from the cache the device wrote, |err| <= ulp16(ref) + 2^-20 max|V| (the
    fp16 rounding of the output is half an ulp; the rest is f32 arithmetic); rows the call does not compute keep
    their sentinel;
  * poison: V rows beyond each row's causal limit and the whole cache of slots no row reads hold +-3e4, so one
    unmasked key moves an output by far more than the tolerance, even at the longest context.
The hook validates every row and tile on the host: a mistake here is refused before anything launches."""
import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from tests import attn_ref as A

pytestmark = pytest.mark.gpu

EPS = 1e-6
MAX_POS = 4096
COS, SIN = A.rope_tables(MAX_POS)
SENTINEL = np.uint16(0x7E01)       # a NaN pattern no kernel writes
POISON = 3e4
ULPS = {}                          # variant -> largest output error in fp16 ulps of the reference (printed at the end)


def u16p(a):
    return a.ctypes.data_as(hiplib.u16p)


def i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def ordered(h):
    """fp16 bit patterns -> integers in value order (adjacent values differ by 1)."""
    b = h.view(np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def make_world(rng, n_slots, n_ctx, R):
    qkv = rng.standard_normal((R, A.LD)).astype(np.float32)
    qkv[:, :A.NH * A.D] *= 3.0                                     # the norm must undo the projection's scale
    q_norm = (1.0 + 0.25 * rng.standard_normal(A.D)).astype(np.float32)
    k_norm = (1.0 + 0.25 * rng.standard_normal(A.D)).astype(np.float32)
    kc = rng.standard_normal((n_slots, A.NKV, n_ctx, A.D)).astype(np.float16)
    vc = np.where(rng.random((n_slots, A.NKV, n_ctx, A.D)) < 0.5, -POISON, POISON).astype(np.float16)
    return qkv, q_norm, k_norm, kc, vc


def history(rng, vc, reads):
    """Real V values (|v| ~ 1) on the rows every output reads but its own append: (slot, last key) pairs."""
    for s, p in reads:
        if p > 0:
            vc[s, :, :p] = rng.standard_normal((A.NKV, p, A.D)).astype(np.float16)


def run(lib, variant, mode, R, row0=0, slot=None, pos=None, slot_base=0, slot_stride=0, pos_base=0, pos_stride=0,
        tiles=None, n_tiles=0, valid_mod=0, valid_n=0, threads=256, n_slots=4, n_ctx=320, seed=0):
    rng = np.random.default_rng(seed)
    qkv, q_norm, k_norm, kc0, vc0 = make_world(rng, n_slots, n_ctx, R)
    sl, ps, active = A.row_layout(R, row0, slot, pos, slot_base, slot_stride, pos_base, pos_stride, valid_mod, valid_n)
    reads = A.output_rows(R, row0, sl, ps, active, tiles, n_tiles, slot_base, pos_base)
    # the history of a prefill run is what the run itself appends: only keys before the run's first position are real
    first = {}
    for i, s, p in reads:
        first[s] = min(first.get(s, p), p)
    for i in range(R):
        if active[i]:
            first[int(sl[i])] = min(first.get(int(sl[i]), int(ps[i])), int(ps[i]))
    history(rng, vc0, first.items())
    kc, vc = kc0.copy(), vc0.copy()
    out = np.full((R, A.OW), SENTINEL, np.uint16)
    tl = i32(tiles)
    rc = lib.q3t_attn(mode, R, row0, hiplib.fptr(qkv), hiplib.fptr(q_norm), hiplib.fptr(k_norm), EPS, hiplib.fptr(COS),
                      hiplib.fptr(SIN), MAX_POS, None if slot is None else hiplib.iptr(i32(slot)),
                      None if pos is None else hiplib.iptr(i32(pos)), slot_base, slot_stride, pos_base, pos_stride,
                      u16p(kc.view(np.uint16)), u16p(vc.view(np.uint16)), n_slots, n_ctx,
                      None if tl is None else hiplib.iptr(tl), n_tiles, valid_mod, valid_n, threads, u16p(out))
    assert rc == 0, rc
    # ---- cache ----
    act = np.flatnonzero(active)
    q, k, v = A.prep(qkv[act], q_norm, k_norm, EPS, COS, SIN, ps[act])
    kw, vw = A.write_cache(kc0, vc0, k, v, sl[act], ps[act])
    written = np.zeros(kc0.shape[:3], bool)
    written[sl[act], :, ps[act]] = True
    for got, want, before, name in ((kc, kw, kc0, "K"), (vc, vw, vc0, "V")):
        np.testing.assert_array_equal(got[~written].view(np.uint16), before[~written].view(np.uint16),
                                      err_msg=f"{name} cache entries outside the appended rows changed")
        g16, w16 = got[written], want[written]                     # [n][128] appended head rows
        d = np.abs(ordered(g16) - ordered(w16))
        # 1 fp16 ulp -- or, for entries far below their row's scale, the f32 arithmetic's own absolute error: the rotation
        # subtracts terms as large as the row (|x0|, |x1| <= sqrt(2) max|row|) after a few f32 roundings (norm scale, weight,
        # two products, the difference: ~5 * 2^-24 max|row|), which is more than an fp16 ulp of a result under ~2^-11 max|row|
        # (measured: 2 ulps on such entries).  Held to 2^-21 max|row| there.
        w64 = w16.astype(np.float64)
        near = np.abs(g16.astype(np.float64) - w64) <= 2.0 ** -21 * np.abs(w64).max(-1, keepdims=True)
        assert ((d <= 1) | near).all(), f"{name} cache: appended rows differ by {d[~near].max()} fp16 ulps"
        assert (d == 0).mean() >= 0.99, f"{name} cache: only {(d == 0).mean():.4f} of appended values bit-equal"
    # ---- output, from the cache the device wrote ----
    qfull = np.zeros((R, A.NH, A.D))
    qfull[act] = q
    rows = [i for i, _, _ in reads]
    ref, vmax = A.attend(qfull[rows], kc, vc, [s for _, s, _ in reads], [p for _, _, p in reads])
    got = out[rows].view(np.float16).astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64)
    err = np.abs(got - ref)
    tol = ulp + 2.0 ** -20 * vmax[:, None]
    worst = float((err / ulp).max())
    ULPS[variant] = max(ULPS.get(variant, 0.0), worst)
    bad = np.argwhere(~(err <= tol))
    assert not len(bad), (f"{variant}: {len(bad)} outputs off, first (row, col) {tuple(bad[0])}: got {got[tuple(bad[0])]}, "
                          f"want {ref[tuple(bad[0])]}, {worst:.2f} ulp at worst")
    untouched = np.setdiff1d(np.arange(R), rows)
    assert (out[untouched] == SENTINEL).all(), f"{variant}: rows the call skips were written"
    return worst


def effective_threads(R, threads):
    fit = 65536 // (R * A.NKV)
    t = fit // 64 * 64 if threads > fit else threads
    return min(max(t, 256), 1024)


def prefetch_edge(threads):
    """APRE * ngrp: the cached keys the kernel requests before its loop (8 x 16 groups at 256 threads, 4 x threads/16)."""
    return 128 if threads <= 256 else 4 * (threads // 16)


N_CTX = 320
BASE_POS = [0, 1, 15, 16, 79, 80, 81, 127, 128, 129, 255, 256, 257, N_CTX - 1]


@pytest.mark.parametrize("threads", [256, 320, 448, 640, 896, 1024])
@pytest.mark.parametrize("R", [1, 9, 32])
def test_fused_decode(test_lib, threads, R):
    """ATTN_FUSED (attn_kernel<FUSED, 8> at 256 threads, <FUSED, 4> at 5..16 waves) with per-row pos / slot arrays:
    mixed positions around every prefetch edge, slots permuted (continuous batching)."""
    t = effective_threads(R, threads)
    edge = prefetch_edge(t)
    positions = sorted(set(BASE_POS + [edge - 1, edge, edge + 1]))
    variant = f"fused<{8 if t <= 256 else 4}> {t} threads"
    rng = np.random.default_rng(threads * 100 + R)
    if R == 1:
        for p in positions:
            run(test_lib, variant, 0, 1, slot=[1], pos=[p], threads=threads, n_slots=3, n_ctx=N_CTX, seed=p)
        return
    n_slots = R + 3
    pos = [positions[i % len(positions)] for i in range(R)]
    rng.shuffle(pos)
    slot = rng.permutation(n_slots)[:R]
    run(test_lib, variant, 0, R, row0=R % 5, slot=slot, pos=pos, threads=threads, n_slots=n_slots, n_ctx=N_CTX,
        seed=threads + R)


@pytest.mark.parametrize("threads", [256, 1024])
def test_fused_long_context(test_lib, threads):
    """The longest context: one row at position 4095 (every key of a 4096-row cache, poison next door in slot 0)."""
    run(test_lib, f"fused<{8 if threads <= 256 else 4}> {threads} threads", 0, 1, slot=[1], pos=[4095], threads=threads,
        n_slots=2, n_ctx=4096, seed=4095)


@pytest.mark.parametrize("p", [0, 1, 63, 64, 300])
def test_wrapper_single_token_form(test_lib, p):
    """The talker wrapper's decode: R = 1, slot_stride = 0, pos_stride = 1 (pos = pos_base + row)."""
    run(test_lib, "fused wrapper form", 0, 1, slot_base=2, slot_stride=0, pos_base=p, pos_stride=1, threads=1024,
        n_slots=3, n_ctx=N_CTX, seed=p)


@pytest.mark.parametrize("short", [1, 0])
def test_short_kernel_positions(test_lib, short):
    """attn_short_kernel: every row at pos_base 0..15 (pos == null, pos_stride == 0); 16 is the first value that falls back
    to attn_kernel, and q3t_set_attn_short(0) sends every position there."""
    try:
        test_lib.q3t_set_attn_short(short)
        for p in range(17):
            variant = "short" if short and p <= 15 else "fused<8> 256 threads (short off)"
            rng = np.random.default_rng(p)
            run(test_lib, variant, 0, 5, slot=rng.permutation(7)[:5], pos_base=p, threads=256, n_slots=7, n_ctx=32,
                seed=100 + p)
    finally:
        test_lib.q3t_set_attn_short(1)


@pytest.mark.parametrize("threads", [256, 1024])
def test_prep_attend_code_predictor_form(test_lib, threads):
    """ATTN_PREP + attn_kernel<ATTEND>: rows of several utterances, each at consecutive positions of its own slot, with
    valid_mod / valid_n padding rows.  Padding rows carry an in-range (slot, pos) of a slot no real row uses, so a kernel
    that forgot to skip them would change that slot's cache and their output rows."""
    U, mod, n = 3, 6, 4          # 3 utterances x 6 rows, the last 2 of each are padding
    R = U * mod
    slots = [3, 0, 2]
    base = [0, 11, 140]
    slot = np.empty(R, np.int32)
    pos = np.empty(R, np.int32)
    for u in range(U):
        for i in range(mod):
            r = u * mod + i
            slot[r], pos[r] = (slots[u], base[u] + i) if i < n else (1, 200 + r)
    run(test_lib, f"prep+attend<{8 if threads <= 256 else 4}> {threads} threads", 1, R, slot=slot, pos=pos,
        valid_mod=mod, valid_n=n, threads=threads, n_slots=4, n_ctx=N_CTX, seed=threads)


@pytest.mark.parametrize("pos_base", [0, 5, 37, 60, 63, 64, 1000])
@pytest.mark.parametrize("length", [1, 15, 16, 17, 50, 971])
def test_tile_kernel_implicit_run(test_lib, pos_base, length):
    """ATTN_PREP + attn_tile_mfma_kernel over one implicit run (the talker wrapper's prefill from any pos_base)."""
    run(test_lib, "prep+tile (implicit run)", 1, length, slot_base=1, slot_stride=0, pos_base=pos_base, pos_stride=1,
        n_tiles=(length + 15) // 16, n_slots=2, n_ctx=2048, seed=pos_base * 7 + length)


def test_tile_kernel_explicit_ragged_tiles(test_lib):
    """Explicit tile lists (the engine's batched prefill): several utterances in several slots, ragged tiles of 1..16 rows
    packed back to back against the next utterance's rows, tiles that straddle key 64 and key 128, listed out of order."""
    rng = np.random.default_rng(5)
    # (slot, first position, tile sizes): 50..65 and 63..64 straddle key 64, 125..140 straddles key 128
    utts = [(2, 50, [16, 16, 8]), (0, 120, [5, 16]), (4, 0, [1, 6]), (1, 61, [2, 2, 4, 1]), (3, 126, [7, 1, 16, 11])]
    row0 = 3
    slot, pos, tiles = [], [], []
    r = row0
    for s, p0, sizes in utts:
        i = 0
        for k in sizes:
            tiles.append([r + i, k, s, p0 + i])
            i += k
        slot += [s] * i
        pos += list(range(p0, p0 + i))
        r += i
    assert any(t[3] < 64 < t[3] + t[1] for t in tiles) and any(t[3] < 128 < t[3] + t[1] for t in tiles)
    tiles = [tiles[i] for i in rng.permutation(len(tiles))]
    run(test_lib, "prep+tile (explicit tiles)", 1, len(slot), row0=row0, slot=slot, pos=pos, tiles=tiles,
        n_tiles=len(tiles), n_slots=6, n_ctx=N_CTX, seed=6)


def test_hook_refuses_out_of_range_calls(test_lib):
    """Bounds are checked on the host: nothing launches for a row past the cache, the rope table or the slots, a tile
    past the rows, or a FUSED call in which two rows append to one slot."""
    R, n_slots, n_ctx = 2, 2, 16
    qkv = np.zeros((R, A.LD), np.float32)
    nrm = np.ones(A.D, np.float32)
    kc = np.zeros((n_slots, A.NKV, n_ctx, A.D), np.uint16)
    vc = kc.copy()
    out = np.full((R, A.OW), SENTINEL, np.uint16)

    def call(mode, slot, pos, tiles=None, n_tiles=0, max_pos=MAX_POS):
        return test_lib.q3t_attn(mode, R, 0, hiplib.fptr(qkv), hiplib.fptr(nrm), hiplib.fptr(nrm), EPS, hiplib.fptr(COS),
                                 hiplib.fptr(SIN), max_pos, hiplib.iptr(i32(slot)), hiplib.iptr(i32(pos)), 0, 0, 0, 0,
                                 u16p(kc), u16p(vc), n_slots, n_ctx, None if tiles is None else hiplib.iptr(i32(tiles)),
                                 n_tiles, 0, 0, 256, u16p(out))

    assert call(0, [0, 1], [3, n_ctx]) == -2               # position past the cache
    assert call(0, [0, 1], [3, 5], max_pos=4) == -2        # position past the rope table
    assert call(0, [0, 2], [3, 5]) == -2                   # slot past the cache
    assert call(0, [1, 1], [3, 5]) == -2                   # two FUSED rows in one slot
    assert call(1, [1, 1], [3, 4], tiles=[0, 3, 1, 3], n_tiles=1) == -2    # tile past the rows
    assert call(1, [1, 1], [14, 15], tiles=[0, 2, 1, 15], n_tiles=1) == -2  # tile past the cache
    assert (out == SENTINEL).all() and not kc.any()




# ---- vocoder attention (voc_attn_kernel, voc_attn_tile_kernel) ----

VOC_ERR = {}


@pytest.fixture(scope="module", autouse=True)
def measured_errors():
    """Prints the largest errors measured per variant once the module's cases have run (visible with -s)."""
    yield
    for k in sorted(ULPS):
        print(f"\nattention max error {ULPS[k]:.3f} ulp  {k}", end="")
    for k in sorted(VOC_ERR, key=lambda s: (s.split()[0], int(s.split("D=")[1].split()[0]), int(s.split("L=")[1]))):
        print(f"\nvoc attention max err {VOC_ERR[k]:.2e} of scale  {k}", end="")
    print()


@pytest.mark.parametrize("kernel,Dh", [(0, 64), (0, 128), (1, 64)])
@pytest.mark.parametrize("L", [1, 7, 64, 72, 73, 84, 85, 256, 750, 1500])
@pytest.mark.parametrize("window", [24, 72, 100000])
def test_voc_attention_kernels(test_lib, kernel, Dh, L, window):
    """Both vocoder attention kernels against the float64 op (B = 2, 2 heads): window edges at 24 and 72, the tile
    kernel up to its 84-column LDS limit (it must refuse 85 and longer), and the global kernel to encoder lengths where
    the RoPE angles reach ~1500 rad.  Tolerance: the exact-fp32 grade of the vocoder tests, 2e-4 of the output's scale."""
    B, H = 2, 2
    rng = np.random.default_rng(L * 7 + window + Dh + kernel)
    x = rng.standard_normal((B, 3 * H * Dh, L)).astype(np.float32)
    y = np.zeros((B, H * Dh, L), np.float32)
    theta = 10000.0
    rc = test_lib.q3t_voc_attn(kernel, hiplib.fptr(x), hiplib.fptr(y), B, H, Dh, L, window, theta)
    if kernel == 1 and 3 * L * (Dh + 1) * 4 > 64 * 1024:
        assert rc == -2
        return
    assert rc == 0, rc
    ref = A.voc_attention(x, H, Dh, window, theta)
    scale = float(np.abs(ref).max())
    err = float(np.abs(y - ref).max()) / scale
    key = f"{'tile' if kernel else 'global'} D={Dh} L={L}"
    VOC_ERR[key] = max(VOC_ERR.get(key, 0.0), err)
    assert err <= 2e-4, f"{key} window={window}: max err {err:.2e} of scale {scale:.3f}"

