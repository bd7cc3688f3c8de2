"""Float64 / exact-integer restatement of the text front-end (csrc/q3_text_api.hip), one function per stage of its chain

    text_gather_kernel -> bias_rows_kernel -> fc1 -> silu_f16_kernel -> bias_rows_kernel -> fc2 -> prefix_rows_kernel

tests/test_gpu_text_stages.py grades every stage from the DEVICE's previous stage (tfe_debug_stages copies x16, h1, a16, h2
back as they lie in memory), so one stage's error never excuses the next.  numpy only.  tests/test_text_reference.py pins this
file against frontend.TextFrontEnd, the fragment index against a brute-force statement of the layout and the integer family
against int64.

Contract per stage
  gather   x16[r] = round_f16_sat(table)[ids[r]], bit for bit: the loader rounds an f32 / bf16 table to fp16 once (nearest even,
           saturating at +-65504), an fp16 table is taken as it is.
  fc1/fc2  h = bias + x16 . W16^T with exact fp16 products summed in f32 in an order that changes with the kernel, on top of an
           accumulator seeded with the f32 bias: |h_dev - h64| <= (K + 1) 2^-24 (|bias| + sum |x| |w|), element by element
           (linear_ref.acc_bound with the bias as one more term).
  silu     a16 = fp16_sat(v * (1 / (1 + __expf(-v)))) evaluated in f32.  Against the UNROUNDED float64 s = silu(v), clipped to
           +-65504: |a16_dev - s| <= 0.5 ulp16(|s| + E) + E, E = SILU32_ERR max(1, |v| / 16).  (Against the rounded value the
           same bound would be wrong: an error far below E turns a rounding at a tie by a whole ulp.)  E cannot be derived
           (hardware exp and reciprocal), it is measured: test_gpu_text_stages.py::test_silu_probe runs a pack whose fc1 is the
           identity, so that h1 = b1 + x is a dense grid over |v| <= 16, and takes the largest |a16_dev - s| - 0.5 ulp16 -- what
           is left of the error once the fp16 rounding is taken off; the constant is twice that, rounded up to a power of two,
           and the probe asserts measured <= constant on every run.  Beyond 16 the factor 1 / (1 + e^-v) is 1 to the last bit
           for v > 16 and the result is below 2e-6 for v < -16, so E |v| / 16 (f32 rounding of a value of size |v|) covers it.
           voc_ops_ref.SILU_ERR is the constant of another expression, g / (1 + __expf(-g)) with __fdividef.
  prefix   out[j] = f32(h2[src[j]]) + codec[cod[j]] (no add when cod[j] = -1), one f32 add: bit for bit.
  chain    from the fp16 inputs alone: d_h1 = fc bound; d_a = SILU_LIP d_h1 + E + 0.5 ulp16; d_h2 = |W2| d_a + fc bound at
           |a| + d_a.  SILU_LIP = 1.1 (max |silu'| = 1.0998).
"""
import numpy as np

from tests import linear_ref as L

U24 = L.U24
F16_MAX = L.F16_MAX
# measured on an MI355X by test_gpu_text_stages.py::test_silu_probe (2 097 152 grid points over |v| <= 16);
# constant = 2 x measured, rounded up to a power of two
SILU32_MEASURED, SILU32_ERR = 1.2534e-6, 2.0 ** -18   # |v * (1 / (1 + __expf(-v))) (device, f32) - float64|, |v| <= 16
SILU_LIP = 1.1
SPECIAL_KEYS = ("im_start", "assistant", "newline", "tts_pad", "tts_bos", "tts_eos", "codec_pad", "codec_bos", "codec_nothink",
                "codec_think_bos", "codec_think_eos")


# ------------------------------------------------------------------------------------------------------------------------
# fragment order (csrc/q3_kernels.h "A operands are stored in MFMA fragment order"; the layout is spelled out above frag_idx in
# q3_frag.h): 16-row x 32-k blocks, row blocks outermost; inside a block lane (m % 16) + 16 * ((k % 32) / 8) owns 8
# consecutive k.  Written from that text, not from the C expression.
# ------------------------------------------------------------------------------------------------------------------------
def frag_index(m, k, K):
    m, k = np.asarray(m, np.int64), np.asarray(k, np.int64)
    block = (m // 16) * (K // 32) + k // 32
    lane = m % 16 + 16 * ((k % 32) // 8)
    return (block * 64 + lane) * 8 + k % 8


def defrag(buf, rows, K):
    """flat fragment-ordered buffer of ceil(rows / 16) * 16 rows -> [rows][K] row-major"""
    buf = np.asarray(buf).reshape(-1)
    assert buf.size == (rows + 15) // 16 * 16 * K, (buf.size, rows, K)
    return buf[frag_index(np.arange(rows)[:, None], np.arange(K)[None, :], K)]


# ------------------------------------------------------------------------------------------------------------------------
# stages
# ------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """f32 -> bf16 bit patterns (round to nearest even), for writing a bf16 table"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def table_f16(table, bf16=False):
    """What the loader keeps of the text table: fp16, saturated.  bf16: `table` holds bf16 bit patterns (uint16)."""
    if bf16:
        table = bf16_to_f32(table)
    table = np.asarray(table)
    return table if table.dtype == np.float16 else L.round_f16_sat(table)


def gather(t16, ids):
    return t16[np.asarray(ids, np.int64)]


def fc(x16, W16, bias):
    """-> (bias + x . W^T in float64, its error bound (K + 1) 2^-24 (|bias| + |x| . |W|^T))"""
    y, mag = L.linear(np.ascontiguousarray(x16), np.ascontiguousarray(W16))
    b = np.asarray(bias, np.float32).astype(np.float64)
    return y + b, L.acc_bound(mag + np.abs(b), x16.shape[1] + 1)


def silu64(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-v))


def silu_err(v):
    return SILU32_ERR * np.maximum(1.0, np.abs(np.asarray(v, np.float64)) / 16.0)


def ulp16_floor(s):
    """fp16 spacing of the binade |s| lies in (2^-24 below the normals): the spacing a rounding of a value next to s has"""
    _, e = np.frexp(np.abs(np.asarray(s, np.float64)))
    return np.ldexp(1.0, np.maximum(e - 11, -24))


def silu_probe_excess(h1, a16):
    """What the SiLU probe measures: |a16_dev - silu64(h1_dev)| with the fp16 rounding's half ulp taken off (>= 0)"""
    s = silu64(np.asarray(h1, np.float32))
    return np.maximum(np.abs(np.asarray(a16, np.float64) - s) - 0.5 * ulp16_floor(s), 0.0)


def silu_f16(h1):
    """h1 (the device's, f32) -> (silu in float64 clipped to the fp16 range, bound on |a16_dev - that|)"""
    s = np.clip(silu64(np.asarray(h1, np.float32)), -F16_MAX, F16_MAX)
    e = silu_err(h1)
    return s, 0.5 * L.ulp16(np.abs(s) + e) + e


def prefix_plan(kind, ids, special):
    """(projected ids, src, cod) of tfe_embed_text / tfe_build_prefix / tfe_build_prefix_stream (ids: the one first token),
    from include/qwen3tts_text.h's row lists"""
    sp = [int(x) for x in special]
    ids = [int(x) for x in ids]
    n = len(ids)
    if kind == "embed":
        return ids, list(range(n)), [-1] * n
    pad3 = [(3, sp[8]), (3, sp[9]), (3, sp[10])]             # tts_pad + codec nothink / think_bos / think_eos
    if kind == "prefix":
        rows = [(0, -1), (1, -1), (2, -1)] + pad3 + [(4, sp[6])] + [(6 + i, sp[6]) for i in range(n)] + [(5, sp[6]), (3, sp[7])]
        proj = sp[0:6] + ids
    elif kind == "stream":
        rows = [(0, -1), (1, -1), (2, -1)] + pad3 + [(4, sp[6]), (5, sp[7])]
        proj = sp[0:5] + ids[:1]
    else:
        raise ValueError(kind)
    return proj, [r[0] for r in rows], [r[1] for r in rows]


def prefix_rows(h2, src, cod, codec):
    """f32(h2[src[j]]) + codec[cod[j]] in f32 (cod[j] = -1: no add)"""
    h2, codec = np.asarray(h2, np.float32), np.asarray(codec, np.float32)
    out = h2[np.asarray(src, np.int64)].copy()
    for j, c in enumerate(cod):
        if c >= 0:
            out[j] = out[j] + codec[c]
    return out


def chain(x16, W1_16, b1, W2_16, b2):
    """fp16 inputs alone -> (h2 in float64, the composed bound on |h2_dev - h2|)"""
    h1, d1 = fc(x16, W1_16, b1)
    s = np.clip(silu64(h1), -F16_MAX, F16_MAX)
    e = silu_err(np.abs(h1) + d1)
    da = SILU_LIP * d1 + e
    da = da + 0.5 * L.ulp16(np.abs(s) + da)
    w2 = np.abs(np.asarray(W2_16, np.float64))
    b2 = np.asarray(b2, np.float32).astype(np.float64)
    h2 = s @ np.asarray(W2_16, np.float64).T + b2
    mag = (np.abs(s) + da) @ w2.T + np.abs(b2)
    return h2, da @ w2.T + L.acc_bound(mag, W2_16.shape[1] + 1)


# ------------------------------------------------------------------------------------------------------------------------
# tensors
# ------------------------------------------------------------------------------------------------------------------------
def real_tensors(seed, V, TD, mid, H, CV):
    """the magnitudes of tests/test_gpu_text.py's tables, weights as fp16 (their own rounding is the loader's, tested by the
    gather cases; fp16 here keeps the packs small)"""
    r = np.random.default_rng(seed)
    return {"text.embedding": (0.05 * r.standard_normal((V, TD))).astype(np.float32),
            "text.fc1.weight": (0.02 * r.standard_normal((mid, TD))).astype(np.float16),
            "text.fc1.bias": (0.02 * r.standard_normal(mid)).astype(np.float32),
            "text.fc2.weight": (0.02 * r.standard_normal((H, mid))).astype(np.float16),
            "text.fc2.bias": (0.02 * r.standard_normal(H)).astype(np.float32),
            "talker.codec_embedding": (0.05 * r.standard_normal((CV, H))).astype(np.float32)}


def int_tensors(seed, V, TD, mid, H, CV):
    """The exact-integer family: table rows with four non-zeros from {+-32, +-64}, W1, W2 in {-2..2}, b1 in 32 {-2..2}, b2 and
    the codec rows integers of magnitude <= 8.  h1 is then a multiple of 32 with |h1| <= 4 * 64 * 2 + 64 = 576: 0, or |v| >= 32
    where the device's SiLU is ReLU to the last bit (v >= 32: e^-v < 2^-25, 1 + e^-v is 1 in f32; v <= -32: |v| e^v < 2^-25,
    below half of fp16's smallest subnormal, so +-0; v = 0: 0).  a16 <= 576 is exact in fp16, and
    sum |a| |w| + |b2| <= 3072 * 1152 + 8 < 2^24 makes every f32 summation order exact."""
    r = np.random.default_rng(seed)
    table = np.zeros((V, TD), np.float32)
    for v in range(V):
        table[v, r.choice(TD, size=4, replace=False)] = r.choice([-64.0, -32.0, 32.0, 64.0], size=4)
    return {"text.embedding": table,
            "text.fc1.weight": r.integers(-2, 3, size=(mid, TD)).astype(np.float16),
            "text.fc1.bias": (32 * r.integers(-2, 3, size=mid)).astype(np.float32),
            "text.fc2.weight": r.integers(-2, 3, size=(H, mid)).astype(np.float16),
            "text.fc2.bias": r.integers(-8, 9, size=H).astype(np.float32),
            "talker.codec_embedding": r.integers(-8, 9, size=(CV, H)).astype(np.float32)}


def int_chain(t, ids):
    """The integer chain of int_tensors -> (x, h1, a, h2) as int64, with the family's preconditions asserted.  The products run
    as float64 matrix products (numpy's integer ones are a hundred times slower): every partial sum is an integer below 2^24,
    so float64 is exact in any order and the conversion to int64 loses nothing."""
    f = lambda a: np.asarray(a, np.float64)
    for k, a in t.items():
        assert np.array_equal(f(a), np.rint(f(a))), k
    x = f(t["text.embedding"])[np.asarray(ids, np.int64)]
    w1, w2, b1, b2 = f(t["text.fc1.weight"]), f(t["text.fc2.weight"]), f(t["text.fc1.bias"]), f(t["text.fc2.bias"])
    assert (np.abs(x) @ np.abs(w1).T + np.abs(b1)).max() < 2 ** 24
    h1 = (x @ w1.T + b1).astype(np.int64)
    assert not (h1 % 32).any() and np.abs(h1).max() <= 576, "h1 must be a multiple of 32, so that SiLU is ReLU exactly"
    a = np.maximum(h1, 0)
    assert a.max() < 2048                                            # exact in fp16
    assert (f(a) @ np.abs(w2).T + np.abs(b2)).max() < 2 ** 24, "f32 must hold every partial sum exactly"
    return x.astype(np.int64), h1, a, (f(a) @ w2.T + b2).astype(np.int64)
