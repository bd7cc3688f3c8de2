"""The text front-end (tfe_*, csrc/q3_text_api.hip) stage by stage against tests/text_ref.py: gather bit for bit, fc1 / fc2
element by element against float64 within the accumulation bound, SiLU within half an fp16 ulp plus the measured f32 error, the
prefix rows bit for bit, the whole chain against the composed bound and, on the exact-integer family, bit for bit against int64.
tfe_debug_stages copies the device's x16 / h1 / a16 / h2 back in fragment order; every stage is graded from the device's own
previous stage.

Geometries (text dim -> mid -> hidden), each the smallest the loader takes that reaches another kernel:
  G1 2048 -> 2048 -> 1024   the product's widths; fc2 on linear_narrow_kernel<16,4>, the 64 x 64 GEMM tile from 65 rows
  G2 3072 -> 2048 -> 128    fc1 at K = 3072; fc2 on plain linear_kernel
  G3 2048 -> 3072 -> 1024   fc1 at N = 3072 (128 x 128 GEMM tile); fc2 on linear_narrow_kernel<12,8>
  G4 2048 -> 2048 -> 4224   hidden > 2 mid with max_tokens 100: the sum-of-squares scratch is sized by the wider of mid and
                            hidden (129 rows need a handle of max_tokens 128: 116 rows is all the first one takes)
Row counts stand on both sides of 8/9 (row groups of the narrow kernel), 16/17, 32/33 (row tiles of linear_kernel), 64/65
(tiled GEMM), 128/129 (its 128-row tile), plus max_rows."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import hiplib
from qwen3_tts_axera_russian_amd import weights as W
from tests import text_ref as T

pytestmark = pytest.mark.gpu

V, CV = 48, 32
GEOM = {"G1": (2048, 2048, 1024), "G2": (3072, 2048, 128), "G3": (2048, 3072, 1024), "G4": (2048, 2048, 4224)}
MAX_TOKENS = {"G1": 128, "G2": 128, "G3": 128, "G4": 100}
ROWS_ALL = (1, 7, 8, 9, 15, 16, 17, 32, 33, 64, 65, 127, 128, 129, 144)          # 144 = max_rows at max_tokens 128
ROWS_FEW = (1, 9, 17, 33, 64, 65, 129)
FC2_KERNEL = {"G1": ("narrow<16,4", "<64,64"), "G2": ("linear<1,", "<64,64"), "G3": ("narrow<12,8", "<64,64"),
              "G4": ("linear<1,", "<128,128")}                                  # below 65 rows, from 65 rows (a GEMM tile)
CFG = W.ModelConfig(text_vocab=V, im_start=40, assistant=41, newline=42, tts_pad=43, tts_bos=44, tts_eos=45, codec_pad=20,
                    codec_bos=21, codec_nothink=27, codec_think_bos=28, codec_think_eos=29)
SPECIAL = [getattr(CFG, k) for k in T.SPECIAL_KEYS] + [0]
OTHER_SPECIAL = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 0]                            # a caller's own: other rows of both tables
u16p = hiplib.u16p


def _u16(a):
    return a.ctypes.data_as(u16p)


class Dev:
    def __init__(self, lib, path, max_tokens):
        self.lib, self.h = lib, lib.tfe_load(path.encode(), None, max_tokens)
        assert self.h, path
        d = (ctypes.c_int32 * 4)()
        assert lib.tfe_debug_stages(self.h, None, 0, None, None, None, None, d) == 0
        self.TD, self.mid, self.H, self.max_rows = (int(x) for x in d)

    def stages(self, ids):
        """-> x16 [n][TD] fp16, h1 [n][mid] f32, a16 [n][mid] fp16, h2 [n][H] f32 (None when the call is refused)"""
        ids = np.ascontiguousarray(ids, np.int32)
        n, Rp = len(ids), (len(ids) + 15) // 16 * 16
        x, a = np.empty(Rp * self.TD, np.uint16), np.empty(Rp * self.mid, np.uint16)
        h1, h2 = np.empty(Rp * self.mid, np.float32), np.empty(Rp * self.H, np.float32)
        rc = self.lib.tfe_debug_stages(self.h, hiplib.iptr(ids), n, _u16(x), hiplib.fptr(h1), _u16(a), hiplib.fptr(h2), None)
        if rc < 0:
            return None
        assert rc == Rp
        return dict(x16=T.defrag(x.view(np.float16), n, self.TD), h1=T.defrag(h1, n, self.mid),
                    a16=T.defrag(a.view(np.float16), n, self.mid), h2=T.defrag(h2, n, self.H))

    def embed(self, ids):
        ids = np.ascontiguousarray(ids, np.int32)
        out = np.full((max(len(ids), 1), self.H), np.nan, np.float32)
        rc = self.lib.tfe_embed_text(self.h, hiplib.iptr(ids), len(ids), hiplib.fptr(out))
        return out[:len(ids)] if rc == 0 else None

    def prefix(self, ids, special=None):
        ids = np.ascontiguousarray(ids, np.int32)
        sp = None if special is None else np.ascontiguousarray(special, np.int32)
        out = np.full((len(ids) + 9, self.H), np.nan, np.float32)
        rc = self.lib.tfe_build_prefix(self.h, hiplib.iptr(ids) if len(ids) else None, len(ids),
                                       None if sp is None else hiplib.iptr(sp), hiplib.fptr(out))
        return out if rc == len(ids) + 9 else None

    def stream(self, first, special=None):
        sp = None if special is None else np.ascontiguousarray(special, np.int32)
        out = np.full((8, self.H), np.nan, np.float32)
        rc = self.lib.tfe_build_prefix_stream(self.h, int(first), None if sp is None else hiplib.iptr(sp), hiplib.fptr(out))
        return out if rc == 8 else None

    def one(self, which):
        out = np.full((1, self.H), np.nan, np.float32)
        fn = self.lib.tfe_tts_pad_embed if which == "pad" else self.lib.tfe_tts_eos_embed
        return out if fn(self.h, hiplib.fptr(out)) == 0 else None

    def free(self):
        if self.h:
            self.lib.tfe_free(self.h)
            self.h = None


class World:
    """packs, handles and the float64 / int64 tables of every pack, made once and left unchanged"""

    def __init__(self, lib, root):
        self.lib, self.root, self.packs, self.devs, self.refs = lib, root, {}, {}, {}

    def tensors(self, geom, kind):
        if (geom, kind) not in self.packs:
            td, mid, h = GEOM[geom]
            t = (T.real_tensors if kind == "real" else T.int_tensors)(len(self.packs) + 7, V, td, mid, h, CV)
            path = os.path.join(self.root, f"text_{geom}_{kind}.q3w")
            W.write_pack(path, CFG.meta(), t)
            self.packs[geom, kind] = (path, t)
        return self.packs[geom, kind]

    def dev(self, geom, kind, max_tokens=None):
        mt = max_tokens or MAX_TOKENS[geom]
        if (geom, kind, mt) not in self.devs:
            self.devs[geom, kind, mt] = Dev(self.lib, self.tensors(geom, kind)[0], mt)
        return self.devs[geom, kind, mt]

    def chain(self, geom, kind):
        """(h2, bound) of every table row from the fp16-rounded inputs alone; int: h2 as int64, bound None"""
        if (geom, kind) not in self.refs:
            _, t = self.tensors(geom, kind)
            if kind == "int":
                self.refs[geom, kind] = (T.int_chain(t, np.arange(V))[3], None)
            else:
                self.refs[geom, kind] = T.chain(T.table_f16(t["text.embedding"]), t["text.fc1.weight"], t["text.fc1.bias"],
                                                t["text.fc2.weight"], t["text.fc2.bias"])
        return self.refs[geom, kind]

    def close(self):
        for d in self.devs.values():
            d.free()


@pytest.fixture(scope="module")
def world(gpu_lib, test_lib, tmp_path_factory):
    test_lib.q3t_reset_linear_knobs()      # the dispatch a fresh process starts with, whatever an earlier module set
    w = World(gpu_lib, str(tmp_path_factory.mktemp("text_stages")))
    yield w
    w.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def worst(err, bound):
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    return float((err / np.maximum(bound, 1e-300)).max())


def ids_for(geom, kind, n):
    return np.random.default_rng(1000 * n + sum(map(ord, geom + kind))).integers(0, V, size=n)


def sweep_cases():
    for geom in GEOM:
        rows = ROWS_ALL if geom == "G1" else ROWS_FEW
        for kind in ("real", "int"):
            for n in rows:
                yield pytest.param(geom, kind, n, id=f"{geom}-{kind}-{n}")
            if geom == "G4":
                yield pytest.param(geom, kind, 116, id=f"{geom}-{kind}-116")     # max_rows at max_tokens 100


@pytest.mark.parametrize("geom,kind,n", list(sweep_cases()))
def test_stages(world, test_lib, geom, kind, n):
    big = geom == "G4" and n > MAX_TOKENS["G4"] + 16
    dev = world.dev(geom, kind, 128 if big else None)
    assert n <= dev.max_rows
    _, t = world.tensors(geom, kind)
    ids = ids_for(geom, kind, n)
    st = dev.stages(ids)
    assert st is not None
    variant = test_lib.q3t_last_linear_variant().decode()                       # fc2's launch
    want = FC2_KERNEL[geom][n >= 65]
    assert (variant.startswith(want) if n < 65 else variant.startswith("gemm") and want in variant), variant
    out = dev.embed(ids)
    np.testing.assert_array_equal(bits(out), bits(st["h2"]))                    # rows without a codec id: h2 as it is
    t16 = T.table_f16(t["text.embedding"])
    np.testing.assert_array_equal(bits(st["x16"]), bits(T.gather(t16, ids)))
    if kind == "int":
        x, h1, a, h2 = T.int_chain(t, ids)
        for name, ref in (("x16", x), ("h1", h1), ("a16", a), ("h2", h2)):
            got = st[name].astype(np.float64)
            assert np.array_equal(got, ref), (name, int((got != ref).sum()))    # values: -0 is 0
        np.testing.assert_array_equal(world.chain(geom, kind)[0][ids], h2)
        print(f"{geom} int n={n} fc2={variant}: gather, fc1, silu, fc2 exact")
        return
    ref, bound = T.fc(st["x16"], t["text.fc1.weight"], t["text.fc1.bias"])
    r1 = worst(np.abs(st["h1"] - ref), bound)
    ref, bound = T.silu_f16(st["h1"])
    rs = worst(np.abs(st["a16"].astype(np.float64) - ref), bound)
    ref, bound = T.fc(st["a16"], t["text.fc2.weight"], t["text.fc2.bias"])
    r2 = worst(np.abs(st["h2"] - ref), bound)
    ref, bound = world.chain(geom, kind)
    re = worst(np.abs(out - ref[ids]), bound[ids])
    print(f"{geom} real n={n} fc2={variant}: worst error / bound  fc1 {r1:.1e}  silu {rs:.3f}  fc2 {r2:.1e}  chain {re:.1e}")


# ---------------------------------------------------------------------------------------------------------------------------
# gather: table dtypes and rounding edges
# ---------------------------------------------------------------------------------------------------------------------------
def edge_table(td):
    """48 rows of N(0, 0.05) with the values a conversion gets wrong planted in rows 0..3: halfway cases (ties to even), fp16
    subnormals and values beyond +-65504 (saturate, never inf)"""
    r = np.random.default_rng(21)
    t = (0.05 * r.standard_normal((V, td))).astype(np.float32)
    m = np.arange(td)
    t[0] = (1.0 + (2 * m + 1) * 2.0 ** -11).astype(np.float32)                  # exactly between two fp16 values, both parities
    t[1] = ((m + 1) * 2.0 ** -25).astype(np.float32) * np.where(m % 2, -1, 1)   # subnormal range, ties included
    t[2, :8] = [65504.0, 65519.0, 65520.0, 70000.0, 1e9, -65520.0, -70000.0, -3e38]
    t[3] = (2.0 ** -14 * (1.0 + (2 * m + 1) * 2.0 ** -11)).astype(np.float32)   # ties at the smallest normal binade
    return t


def write_safetensors(path, tensors):
    """{HF key: (dtype name, ndarray of raw elements)} -> a .safetensors file (8-byte header length, JSON table, raw data)"""
    head, off = {}, 0
    for k, (dt, a) in tensors.items():
        head[k] = {"dtype": dt, "shape": list(a.shape), "data_offsets": [off, off + a.nbytes]}
        off += a.nbytes
    js = json.dumps(head).encode()
    js += b" " * (-len(js) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(js)) + js)
        for _, a in tensors.values():
            f.write(np.ascontiguousarray(a).tobytes())


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_gather_is_the_rounded_table_bit_for_bit(world, tmp_path, dtype):
    td, mid, h = 2048, 2048, 128
    t = T.real_tensors(3, V, td, mid, h, CV)
    table = edge_table(td)
    if dtype == "bf16":
        raw = T.bf16_bits(table)
        raw[2, :8] = T.bf16_bits(np.array([65504.0, 65280.0, 65536.0, 70144.0, 1e9, -65536.0, -70144.0, -3e38], np.float32))
        want = T.table_f16(raw, bf16=True)
        path = str(tmp_path / "text_bf16.safetensors")
        write_safetensors(path, {"talker.model.text_embedding.weight": ("BF16", raw),
                                 "talker.text_projection.linear_fc1.weight": ("F16", t["text.fc1.weight"]),
                                 "talker.text_projection.linear_fc1.bias": ("F32", t["text.fc1.bias"]),
                                 "talker.text_projection.linear_fc2.weight": ("F16", t["text.fc2.weight"]),
                                 "talker.text_projection.linear_fc2.bias": ("F32", t["text.fc2.bias"]),
                                 "talker.model.codec_embedding.weight": ("F32", t["talker.codec_embedding"])})
    else:
        t["text.embedding"] = table if dtype == "f32" else T.table_f16(table)
        want = T.table_f16(t["text.embedding"])
        path = str(tmp_path / f"text_{dtype}.q3w")
        W.write_pack(path, CFG.meta(), t)
    assert np.isfinite(want.astype(np.float32)).all() and float(np.abs(want.astype(np.float32)).max()) == 65504.0
    dev = Dev(world.lib, path, 64)
    try:
        ids = np.array([2, 0, 1, 3, 47, 0, 2, 30, 3, 1] + list(range(V)), np.int32)
        st = dev.stages(ids)
        np.testing.assert_array_equal(bits(st["x16"]), bits(want[ids]))
        assert np.isfinite(st["h2"]).all()
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------
# SiLU: the measured constant
# ---------------------------------------------------------------------------------------------------------------------------
def test_silu_probe(world, tmp_path):
    """fc1 = identity, table row r = -16 + r / 32 in every column, b1[c] = c / 65536: h1[r][c] = -16 + r / 32 + c / 65536, a grid
    of 1024 x 2048 points of step 2^-16 over [-16, 16).  Measures text_ref.SILU32_MEASURED and holds SILU32_ERR to it."""
    td = mid = 2048
    rows = 1024
    t = {"text.embedding": np.repeat((-16.0 + np.arange(rows) / 32.0).astype(np.float16)[:, None], td, axis=1),
         "text.fc1.weight": np.eye(mid, td, dtype=np.float16),
         "text.fc1.bias": (np.arange(mid) / 65536.0).astype(np.float32),
         "text.fc2.weight": np.zeros((128, mid), np.float16), "text.fc2.bias": np.zeros(128, np.float32),
         "talker.codec_embedding": np.zeros((CV, 128), np.float32)}
    path = str(tmp_path / "text_silu_probe.q3w")
    W.write_pack(path, CFG.meta(), t)
    dev = Dev(world.lib, path, 128)
    try:
        measured, points = 0.0, 0
        for r0 in range(0, rows, 128):
            st = dev.stages(np.arange(r0, r0 + 128))
            want = (-16.0 + np.arange(r0, r0 + 128)[:, None] / 32.0 + np.arange(mid)[None, :] / 65536.0).astype(np.float32)
            np.testing.assert_array_equal(st["h1"], want)                       # the grid is what it was meant to be
            measured = max(measured, float(T.silu_probe_excess(st["h1"], st["a16"]).max()))
            ref, bound = T.silu_f16(st["h1"])
            worst(np.abs(st["a16"].astype(np.float64) - ref), bound)
            points += want.size
    finally:
        dev.free()
    print(f"silu probe: {points} points over |v| <= 16, max |device - float64| beyond the fp16 half ulp {measured:.4e} "
          f"(text_ref.SILU32_MEASURED {T.SILU32_MEASURED:.4e}, SILU32_ERR {T.SILU32_ERR:.4e})")
    assert points >= 100000 and measured <= T.SILU32_ERR


def test_silu_saturates_instead_of_overflowing(world, tmp_path):
    """h1 beyond the fp16 range (fc1 = identity, b1 as large as f32 goes): a16 is +-65504 or -0, never inf or NaN"""
    td = mid = 2048
    big = np.array([65503.0, 65504.0, 65519.0, 65520.0, 65536.0, 7e4, 1e6, 3e38, -7e4, -1e6, -3e38, 88.0, -88.0, -104.0], np.float32)
    b1 = np.resize(big, mid)
    t = {"text.embedding": np.repeat(np.array([0.0, 1.0, -1.0, 1000.0], np.float16)[:, None], td, axis=1),
         "text.fc1.weight": np.eye(mid, td, dtype=np.float16), "text.fc1.bias": b1,
         "text.fc2.weight": np.zeros((128, mid), np.float16), "text.fc2.bias": np.zeros(128, np.float32),
         "talker.codec_embedding": np.zeros((CV, 128), np.float32)}
    path = str(tmp_path / "text_silu_sat.q3w")
    W.write_pack(path, CFG.meta(), t)
    dev = Dev(world.lib, path, 64)
    try:
        st = dev.stages([0, 1, 2, 3])
    finally:
        dev.free()
    assert st["h1"].max() > 1e38 and st["h1"].min() < -1e38
    a = st["a16"].astype(np.float64)
    assert np.isfinite(a).all() and a.max() == 65504.0 and a.min() > -1.0
    ref, bound = T.silu_f16(st["h1"])
    worst(np.abs(a - ref), bound)
    assert (a[st["h1"] >= 65520.0] == 65504.0).all() and (a[st["h1"] <= -88.0] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# prefix rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["real", "int"])
@pytest.mark.parametrize("special", ["default", "caller"])
def test_prefix_rows_bit_for_bit(world, kind, special):
    """every entry point's rows = f32(h2_dev[src[j]]) + codec[cod[j]], from the h2 the same projection leaves (equal row count:
    equal kernels, equal bits)"""
    dev = world.dev("G1", kind)
    _, t = world.tensors("G1", kind)
    codec = t["talker.codec_embedding"]
    sp_arg, sp = (None, SPECIAL) if special == "default" else (OTHER_SPECIAL, OTHER_SPECIAL)
    rng = np.random.default_rng(8)
    for n in (0, 1, 11, 60):                                                    # 6 + 60 projected rows: the tiled GEMM
        ids = rng.integers(0, V, size=n)
        proj, src, cod = T.prefix_plan("prefix", ids, sp)
        got = dev.prefix(ids, sp_arg)
        assert got is not None and got.shape == (n + 9, dev.H)
        np.testing.assert_array_equal(bits(got), bits(T.prefix_rows(dev.stages(proj)["h2"], src, cod, codec)))
        for a, b in ((3, 4), (4, 5), (3, n + 8)):                               # the tts_pad rows differ by their codec rows only
            if kind == "int":
                np.testing.assert_array_equal(got[b] - got[a], codec[cod[b]] - codec[cod[a]])
        if kind == "int":
            h2 = world.chain("G1", "int")[0]
            want = h2[proj][src] + np.where(np.array(cod)[:, None] >= 0, codec[np.maximum(cod, 0)], 0).astype(np.int64)
            assert np.array_equal(got.astype(np.float64), want)
    proj, src, cod = T.prefix_plan("stream", [13], sp)
    got = dev.stream(13, sp_arg)
    assert got is not None
    np.testing.assert_array_equal(bits(got), bits(T.prefix_rows(dev.stages(proj)["h2"], src, cod, codec)))
    # the two one-row calls read the pack's own ids, whatever a caller passes elsewhere
    np.testing.assert_array_equal(bits(dev.one("pad")), bits(dev.stages([CFG.tts_pad])["h2"]))
    np.testing.assert_array_equal(bits(dev.one("eos")), bits(dev.stages([CFG.tts_eos])["h2"]))
    assert (dev.one("pad") != dev.one("eos")).any()


# ---------------------------------------------------------------------------------------------------------------------------
# invariances
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 70])
def test_same_call_same_bits(world, n):
    """At a fixed row count: permuting the ids permutes the rows, and a call gives the same bits on a fresh handle, after a
    longer call on the same handle (stale rows n.. of x16 / h1 / a16 beside the live ones) and after a refused call"""
    dev = world.dev("G1", "real")
    ids = ids_for("G1", "perm", n)
    first = dev.stages(ids)
    out = dev.embed(ids)
    perm = np.random.default_rng(n).permutation(n)
    np.testing.assert_array_equal(bits(dev.embed(ids[perm])), bits(out[perm]))
    fresh = Dev(world.lib, world.tensors("G1", "real")[0], MAX_TOKENS["G1"])
    try:
        np.testing.assert_array_equal(bits(fresh.embed(ids)), bits(out))
    finally:
        fresh.free()
    assert dev.stages((ids_for("G1", "long", 140) + 1) % V) is not None
    again = dev.stages(ids)
    for k in first:
        np.testing.assert_array_equal(bits(again[k]), bits(first[k]), err_msg=k)
    assert dev.embed([V]) is None and dev.stages([0, -1]) is None
    np.testing.assert_array_equal(bits(dev.embed(ids)), bits(out))


def test_rows_across_row_counts_agree_within_the_bounds(world):
    """Another row count is another kernel or another split of K: the same token's row is not promised bit for bit, only within
    the sum of both calls' bounds (text front-end)"""
    dev = world.dev("G1", "real")
    _, bound = world.chain("G1", "real")
    ids = ids_for("G1", "across", 9)
    alone = dev.embed(ids)
    for n in (16, 33, 64, 70, 130):
        more = np.concatenate([ids, ids_for("G1", "fill", n - 9)])
        got = dev.embed(more)[:9]
        worst(np.abs(got.astype(np.float64) - alone), 2 * bound[ids])
        print(f"9 rows alone against the same 9 among {n}: {int((bits(got) != bits(alone)).sum())} of {got.size} elements differ, "
              f"max |difference| {float(np.abs(got - alone).max()):.2e}")


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(world):
    dev = world.dev("G1", "real")
    mt = MAX_TOKENS["G1"]
    ids = ids_for("G1", "refuse", 12)
    before = dev.prefix(ids)
    assert before is not None

    def still_good():
        np.testing.assert_array_equal(bits(dev.prefix(ids)), bits(before))

    bad_text, bad_codec, neg_codec = list(SPECIAL), list(SPECIAL), list(SPECIAL)
    bad_text[3], bad_codec[8], neg_codec[6] = V, CV, -2
    no_codec = list(SPECIAL)
    no_codec[9] = -1                                                            # -1 is "no codec row", not a bad id
    refused = [lambda: dev.embed([3, V, 4]), lambda: dev.embed([3, -1, 4]), lambda: dev.embed([]),
               lambda: dev.prefix(np.zeros(mt + 8, np.int32)),                  # mt + 17 rows > max_rows = mt + 16
               lambda: dev.prefix(ids, bad_text), lambda: dev.prefix(ids, bad_codec), lambda: dev.prefix(ids, neg_codec),
               lambda: dev.stream(5, bad_codec), lambda: dev.stream(V), lambda: dev.stages(np.zeros(mt + 17, np.int32))]
    for i, call in enumerate(refused):
        assert call() is None, i
        still_good()
    full = dev.prefix(ids_for("G1", "full", mt))                                # max_tokens itself: mt + 9 rows
    assert full is not None and np.isfinite(full).all()
    got = dev.prefix(ids, no_codec)
    np.testing.assert_array_equal(bits(got[4]), bits(dev.stages(T.prefix_plan("prefix", ids, SPECIAL)[0])["h2"][3]))
    np.testing.assert_array_equal(bits(np.delete(got, 4, 0)), bits(np.delete(before, 4, 0)))
    still_good()


@pytest.mark.parametrize("dims", [(1024, 2048, 128), (2048, 1024, 128)])
def test_load_refuses_a_1024_wide_projection(world, tmp_path, dims):
    """launch_linear has no fp16-input, residual-epilogue kernel for K = 1024 below 65 rows: such a pack must not load"""
    t = T.real_tensors(4, V, *dims, CV)
    path = str(tmp_path / "text_k1024.q3w")
    W.write_pack(path, CFG.meta(), t)
    assert not world.lib.tfe_load(path.encode(), None, 64)
