"""GGUF for the tests: a writer, ggml's dequantisation formulas in float64, and random / edge blocks.

Written independently of qwen3_tts_axera_russian_amd/gguf.py (which is under test): dequant64 walks the elements of a
block with the index arithmetic of the formulas as DESIGN.md 1 ("GGUF") states them -- c, h, j, l per element -- where
gguf.py reshapes whole blocks.  Every product of the formulas is exact in float64 and so is the K-quants' subtraction
(the two terms span at most 52 bits), so dequant64(...).astype(float32) is the contract's fp32 value and
f16_sat(that) its fp16 weight.
"""
import struct

import numpy as np

# name -> (ggml type number, DType of csrc/q3_common.h, block elements, block bytes)
TYPES = {"F32": (0, 0, 1, 4), "F16": (1, 1, 1, 2), "BF16": (30, 4, 1, 2), "Q4_0": (2, 5, 32, 18), "Q8_0": (8, 6, 32, 34),
         "Q4_K": (12, 7, 256, 144), "Q5_K": (13, 8, 256, 176), "Q6_K": (14, 9, 256, 210)}
BLOCK_TYPES = ("Q4_0", "Q8_0", "Q4_K", "Q5_K", "Q6_K")
# GGUF metadata value types
U8, I8, U16, I16, U32, I32, F32, BOOL, STR, ARR, U64, I64, F64 = range(13)
_FMT = {U8: "<B", I8: "<b", U16: "<H", I16: "<h", U32: "<I", I32: "<i", F32: "<f", BOOL: "<?", U64: "<Q", I64: "<q", F64: "<d"}


# ---------------------------------------------------------------------------------------------------------------------
# writer

def gstr(s):
    b = s.encode() if isinstance(s, str) else s
    return struct.pack("<Q", len(b)) + b


def kv_bytes(key, vtype, value):
    """One key/value pair.  An array's value is (element type, [elements])."""
    out = gstr(key) + struct.pack("<I", vtype)
    if vtype == STR:
        return out + gstr(value)
    if vtype == ARR:
        et, elems = value
        out += struct.pack("<IQ", et, len(elems))
        for e in elems:
            out += gstr(e) if et == STR else struct.pack(_FMT[et], e)
        return out
    return out + struct.pack(_FMT[vtype], value)


def info_bytes(name, ne, ggml_type, offset):
    return gstr(name) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", x) for x in ne) + struct.pack("<IQ", ggml_type, offset)


def nbytes_of(tname, shape):
    _, _, bs, bb = TYPES[tname]
    n = 1
    for x in shape:
        n *= x
    return n // bs * bb


def gguf_bytes(kvs, tensors, version=3, alignment=32, magic=b"GGUF", n_tensors=None, n_kv=None):
    """kvs: [(key, value type, value)]; tensors: [(name, type name, shape in row-major order, raw bytes)].
    -> (file bytes, {name: (offset in the file, nbytes)}).  general.alignment is written when alignment != 32."""
    kvs = list(kvs)
    if alignment != 32:
        kvs.append(("general.alignment", U32, alignment))
    head = magic + struct.pack("<IQQ", version, len(tensors) if n_tensors is None else n_tensors, len(kvs) if n_kv is None else n_kv)
    head += b"".join(kv_bytes(*kv) for kv in kvs)
    off, infos, place = 0, b"", {}
    for name, tname, shape, raw in tensors:
        assert len(raw) == nbytes_of(tname, shape), (name, len(raw), nbytes_of(tname, shape))
        infos += info_bytes(name, list(reversed(shape)), TYPES[tname][0], off)
        place[name] = (off, len(raw))
        off = (off + len(raw) + alignment - 1) // alignment * alignment
    head += infos
    data0 = (len(head) + alignment - 1) // alignment * alignment
    body = bytearray(head + b"\0" * (data0 - len(head)))
    for name, tname, shape, raw in tensors:
        o = data0 + place[name][0]
        body += b"\0" * (o - len(body))
        body += raw
        place[name] = (o, len(raw))
    return bytes(body), place


def qwen3_kvs(layers=2, hidden=1024, ffn=3072, heads=16, kv_heads=8, head_dim=128, eps=1e-6, theta=1e6, arch="qwen3"):
    return [("general.architecture", STR, arch), ("general.name", STR, "talker"),
            ("qwen3.block_count", U32, layers), ("qwen3.context_length", U32, 32768),
            ("qwen3.embedding_length", U32, hidden), ("qwen3.feed_forward_length", U32, ffn),
            ("qwen3.attention.head_count", U32, heads), ("qwen3.attention.head_count_kv", U32, kv_heads),
            ("qwen3.attention.layer_norm_rms_epsilon", F32, eps), ("qwen3.rope.freq_base", F32, theta),
            ("qwen3.attention.key_length", U32, head_dim), ("qwen3.attention.value_length", U32, head_dim),
            ("tokenizer.ggml.model", STR, "gpt2"), ("tokenizer.ggml.tokens", ARR, (STR, ["a", "bc", "", "d" * 9])),
            ("tokenizer.ggml.token_type", ARR, (I32, [1, 1, 3, 1])), ("general.file_type", U32, 15)]


# ---------------------------------------------------------------------------------------------------------------------
# the formulas, float64

def f16_sat(a):
    """float -> float16, round to nearest even, saturating at +-65504 (f2h_sat's rule)"""
    return np.clip(np.asarray(a, np.float32), -65504.0, 65504.0).astype(np.float16)


def _half(b, o):
    """fp16 at byte o of every block -> float64 [nb]"""
    return (b[:, o].astype(np.uint16) | (b[:, o + 1].astype(np.uint16) << 8)).view(np.float16).astype(np.float64)


def _scale_min(s, j):
    """(sc_j, m_j) of the 12 scale bytes s [nb, 12]"""
    s = s.astype(np.int64)
    if j < 4:
        return s[:, j] & 63, s[:, j + 4] & 63
    return (s[:, j + 4] & 15) | ((s[:, j - 4] >> 6) << 4), (s[:, j + 4] >> 4) | ((s[:, j] >> 6) << 4)


def dequant64(tname, data, K=None):
    """float64 values of the elements of `data` (bytes / uint8 array of whole blocks); K given: reshaped to [-1, K]"""
    raw = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1).view(np.uint8)
    _, _, bs, bb = TYPES[tname]
    if tname == "F32":
        v = raw.view("<f4").astype(np.float64)
    elif tname == "F16":
        v = raw.view("<f2").astype(np.float64)
    elif tname == "BF16":
        v = (raw.view("<u2").astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    else:
        b = raw.reshape(-1, bb)
        v = np.empty((b.shape[0], bs), np.float64)
        bi = b.astype(np.int64)
        for e in range(bs):
            l = e % 32
            if tname == "Q8_0":
                v[:, e] = _half(b, 0) * b[:, 2 + e].view(np.int8).astype(np.float64)
            elif tname == "Q4_0":
                q = (bi[:, 2 + e] & 15) if e < 16 else (bi[:, 2 + e - 16] >> 4)
                v[:, e] = _half(b, 0) * (q - 8)
            elif tname in ("Q4_K", "Q5_K"):
                c, h = e // 64, (e % 64) // 32
                j = 2 * c + h
                qs0 = 48 if tname == "Q5_K" else 16
                byte = bi[:, qs0 + 32 * c + l]
                q = (byte >> 4) if h else (byte & 15)
                if tname == "Q5_K":
                    q = q + 16 * ((bi[:, 16 + l] >> j) & 1)
                sc, m = _scale_min(b[:, 4:16], j)
                v[:, e] = (_half(b, 0) * sc) * q - _half(b, 2) * m
            else:   # Q6_K
                c, t = e // 128, (e % 128) // 32
                nib = bi[:, 64 * c + l + 32 * (t & 1)]
                nib = (nib & 15) if t < 2 else (nib >> 4)
                q = (nib | (((bi[:, 128 + 32 * c + l] >> (2 * t)) & 3) << 4)) - 32
                sc = b[:, 192 + 8 * c + l // 16 + 2 * t].view(np.int8).astype(np.float64)
                v[:, e] = _half(b, 208) * sc * q
        v = v.reshape(-1)
    return v if K is None else v.reshape(-1, K)


# ---------------------------------------------------------------------------------------------------------------------
# blocks

_D_OFFSETS = {"Q4_0": (0,), "Q8_0": (0,), "Q4_K": (0, 2), "Q5_K": (0, 2), "Q6_K": (208,)}
_EDGE_HALVES = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x3c00, 0xbc00, 0x7bff, 0xfbff], np.uint16)


def finite_halves(rng, n):
    """n finite fp16 bit patterns: uniform over all finite patterns (both signs, subnormals), every 8th one an edge value
    (+-0, smallest and largest subnormal, smallest normal, +-1, +-65504)"""
    u = rng.integers(0, 0x7c00, n, dtype=np.uint16) | (rng.integers(0, 2, n, dtype=np.uint16) << 15)
    k = np.arange(n) % 8 == 0
    u[k] = _EDGE_HALVES[rng.integers(0, len(_EDGE_HALVES), int(k.sum()))]
    return u


def put_halves(blocks, tname, which, bits):
    o = _D_OFFSETS[tname][which]
    blocks[:, o] = bits & 0xff
    blocks[:, o + 1] = bits >> 8


def random_blocks(tname, n, rng, scale=None):
    """uint8 [n, block bytes]: every byte random, then d (and dmin) finite.  scale=None: d / dmin from all finite fp16;
    scale=s: weights of a model -- |d| ~ s * U(0.5, 1.5) chosen so the dequantised values have a standard deviation near
    0.02 and (K-quants) a mean near 0."""
    bb = TYPES[tname][3]
    b = rng.integers(0, 256, (n, bb), dtype=np.uint8)
    for w in range(len(_D_OFFSETS[tname])):
        if scale is None:
            bits = finite_halves(rng, n)
        else:
            base = {"Q8_0": 0.02 / 73, "Q4_0": 0.02 / 4.6, "Q4_K": 1e-4, "Q5_K": 5e-5, "Q6_K": 0.02 / 1369}[tname]
            if w == 1:
                base *= 7.5 if tname == "Q4_K" else 15.5    # dmin * E[m] = d * E[sc] * E[q]
            mag = (scale / 0.02) * base * rng.uniform(0.5, 1.5, n)
            sign = 1.0 if tname in ("Q4_K", "Q5_K") else rng.choice([-1.0, 1.0], n)
            bits = (mag * sign).astype(np.float16).view(np.uint16)
        put_halves(b, tname, w, bits)
    return b


def edge_blocks(tname):
    """uint8 [n, block bytes]: all zero bytes; all 0xFF bytes with a finite d (and dmin); for the K-quants with packed
    scales, every 6-bit value in every scale and every minimum position (j < 4 and j >= 4) with the other bits set"""
    bb = TYPES[tname][3]
    out = [np.zeros(bb, np.uint8)]
    ff = np.full(bb, 0xFF, np.uint8)
    for o in _D_OFFSETS[tname]:
        ff[o], ff[o + 1] = 0x00, 0x3c     # 1.0
    out.append(ff)
    if tname in ("Q4_K", "Q5_K"):
        for j in range(8):
            for val in range(64):
                for other in (0x00, 0xFF):
                    for is_min in (0, 1):
                        blk = ff.copy()
                        blk[0], blk[1], blk[2], blk[3] = 0x00, 0x38, 0x00, 0x34    # d = 0.5, dmin = 0.25
                        s = np.full(12, other, np.uint8)
                        if j < 4:
                            k = j + 4 * is_min
                            s[k] = (s[k] & 0xC0) | val
                        else:
                            lo, hi = val & 15, val >> 4
                            if is_min:
                                s[j + 4] = (s[j + 4] & 0x0F) | (lo << 4)
                                s[j] = (s[j] & 0x3F) | (hi << 6)
                            else:
                                s[j + 4] = (s[j + 4] & 0xF0) | lo
                                s[j - 4] = (s[j - 4] & 0x3F) | (hi << 6)
                        blk[4:16] = s
                        out.append(blk)
    return np.stack(out)


def case_blocks(tname, n, seed):
    """n blocks for a kernel case: the edge blocks first (as many as fit, cycling through all of them over the seeds), then
    random ones"""
    rng = np.random.default_rng(seed)
    b = random_blocks(tname, n, rng)
    e = edge_blocks(tname)
    k = min(len(e), max(1, n // 2))
    start = (seed * 131) % len(e)
    b[:k] = e[(start + np.arange(k)) % len(e)]
    b[:min(2, n)] = e[:min(2, n)]          # the all-zero and the all-0xFF block are in every case
    return b
