"""A small GGUF reader (v2 / v3, little-endian) for the talker file the reference's server is started with.

    meta, tensors = read_gguf(path)      # {key: value}, {name: float32 array, row-major (ne reversed)}

Tensor types F32, F16, BF16, Q4_0, Q8_0, Q4_K, Q5_K, Q6_K are read; the block types are dequantised with ggml's
dequantize_row_* formulas in float32 (the same ones csrc/q3_dequant.hip evaluates on the GPU: DESIGN.md 1, "GGUF").
Every product of those formulas is exact in float32 and the K-quants' subtraction is their one rounding, so the values
here are the ones the device loader produces.  Host-side tool (converters, tests): the libraries parse the file natively
(csrc/q3_formats.cpp) and never call this.
"""
from __future__ import annotations

import struct

import numpy as np

# ggml type -> (name, elements per block, bytes per block)
GGML_TYPES = {0: ("F32", 1, 4), 1: ("F16", 1, 2), 30: ("BF16", 1, 2), 2: ("Q4_0", 32, 18), 8: ("Q8_0", 32, 34),
              12: ("Q4_K", 256, 144), 13: ("Q5_K", 256, 176), 14: ("Q6_K", 256, 210)}
_SCALAR = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}

# llama.cpp's qwen3 tensor names -> the container's layer parts (weights.LAYER_PARTS)
GGUF_LAYER_PARTS = {"attn_norm": "input_ln", "attn_q": "q_proj", "attn_k": "k_proj", "attn_v": "v_proj",
                    "attn_output": "o_proj", "attn_q_norm": "q_norm", "attn_k_norm": "k_norm", "ffn_norm": "post_ln",
                    "ffn_gate": "gate_proj", "ffn_up": "up_proj", "ffn_down": "down_proj"}
# metadata keys the native parser reads (general.alignment and general.architecture besides)
GGUF_META_KEYS = ("qwen3.block_count", "qwen3.embedding_length", "qwen3.feed_forward_length", "qwen3.attention.head_count",
                  "qwen3.attention.head_count_kv", "qwen3.attention.layer_norm_rms_epsilon", "qwen3.rope.freq_base",
                  "qwen3.attention.key_length")


def _f16(b):
    """bytes [..., 2] (uint8) -> float32 of the little-endian fp16 they hold"""
    return np.ascontiguousarray(b).view("<f2")[..., 0].astype(np.float32)


def _scale_min_k4(s):
    """s uint8 [nb, 12] -> (sc, m) uint8 [nb, 8]: the 6-bit scales and minima of a Q4_K / Q5_K block"""
    s = s.astype(np.uint8)
    sc = np.empty(s.shape[:-1] + (8,), np.uint8)
    m = np.empty_like(sc)
    sc[..., :4] = s[..., 0:4] & 63
    m[..., :4] = s[..., 4:8] & 63
    sc[..., 4:] = (s[..., 8:12] & 15) | ((s[..., 0:4] >> 6) << 4)
    m[..., 4:] = (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)
    return sc, m


def dequantize(ggml_type: int, data, n: int) -> np.ndarray:
    """The n float32 values of `data` (bytes or a uint8 array) holding n elements of ggml type `ggml_type`."""
    if ggml_type not in GGML_TYPES:
        raise ValueError(f"ggml type {ggml_type} is not read (F32, F16, BF16, Q4_0, Q8_0, Q4_K, Q5_K, Q6_K are)")
    name, bs, bb = GGML_TYPES[ggml_type]
    if n % bs:
        raise ValueError(f"{n} elements are no multiple of the {bs}-element {name} block")
    raw = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1)
    if raw.size != n // bs * bb:
        raise ValueError(f"{name}: {raw.size} bytes for {n} elements (want {n // bs * bb})")
    if name == "F32":
        return raw.view("<f4").astype(np.float32)
    if name == "F16":
        return raw.view("<f2").astype(np.float32)
    if name == "BF16":
        return (raw.view("<u2").astype(np.uint32) << 16).view(np.float32)
    b = raw.reshape(-1, bb)
    f32 = np.float32
    if name == "Q8_0":
        return (_f16(b[:, 0:2])[:, None] * b[:, 2:].view(np.int8).astype(f32)).reshape(-1)
    if name == "Q4_0":
        qs = b[:, 2:]
        q = np.concatenate([qs & 15, qs >> 4], axis=1).astype(np.int32) - 8
        return (_f16(b[:, 0:2])[:, None] * q.astype(f32)).reshape(-1)
    if name in ("Q4_K", "Q5_K"):
        d, dmin = _f16(b[:, 0:2]), _f16(b[:, 2:4])
        sc, m = _scale_min_k4(b[:, 4:16])
        qs = b[:, (48 if name == "Q5_K" else 16):].reshape(-1, 4, 32)
        q = np.stack([qs & 15, qs >> 4], axis=2).reshape(-1, 8, 32).astype(np.int32)     # [nb, j = 2c + h, l]
        if name == "Q5_K":
            qh = b[:, 16:48]
            q += 16 * ((qh[:, None, :] >> np.arange(8, dtype=np.uint8)[None, :, None]) & 1).astype(np.int32)
        d1 = d[:, None] * sc.astype(f32)
        m1 = dmin[:, None] * m.astype(f32)
        return (d1[:, :, None] * q.astype(f32) - m1[:, :, None]).astype(f32).reshape(-1)
    # Q6_K: ql[128] qh[64] sc[16] d
    ql, qh = b[:, 0:128].reshape(-1, 2, 2, 32), b[:, 128:192].reshape(-1, 2, 32)
    sc = b[:, 192:208].view(np.int8).astype(f32).reshape(-1, 2, 4, 2)                   # [nb, c, t, l / 16]
    d = _f16(b[:, 208:210])
    q = np.empty((b.shape[0], 2, 4, 32), np.int32)                                      # [nb, c, t, l]
    for t in range(4):
        nib = ql[:, :, t & 1, :]
        nib = (nib & 15) if t < 2 else (nib >> 4)
        q[:, :, t, :] = (nib | (((qh >> (2 * t)) & 3) << 4)).astype(np.int32) - 32
    ds = d[:, None, None, None] * sc
    return (np.repeat(ds, 16, axis=3) * q.astype(f32)).astype(f32).reshape(-1)


class _Cursor:
    def __init__(self, buf):
        self.b, self.o = buf, 0

    def take(self, fmt):
        n = struct.calcsize(fmt)
        if self.o + n > len(self.b):
            raise ValueError("truncated GGUF")
        v = struct.unpack_from(fmt, self.b, self.o)[0]
        self.o += n
        return v

    def string(self):
        n = self.take("<Q")
        if n > len(self.b) - self.o:
            raise ValueError("truncated GGUF (string)")
        s = bytes(self.b[self.o:self.o + n])
        self.o += n
        return s.decode("utf-8", errors="replace")

    def value(self, t, depth=0):
        if t in _SCALAR:
            return self.take(_SCALAR[t])
        if t == 8:
            return self.string()
        if t == 9 and depth == 0:
            et, cnt = self.take("<I"), self.take("<Q")
            if cnt > len(self.b) - self.o:
                raise ValueError("truncated GGUF (array)")
            return [self.value(et, 1) for _ in range(cnt)]
        raise ValueError(f"GGUF value type {t} is not supported")


def read_gguf_raw(path):
    """-> (meta, {name: (ggml type, shape row-major, uint8 array of the raw bytes)}); the arrays view a memory map"""
    buf = np.memmap(path, np.uint8, "r")
    c = _Cursor(buf)
    if bytes(buf[:4]) != b"GGUF":
        raise ValueError(f"{path}: not a GGUF file")
    c.o = 4
    version = c.take("<I")
    if version not in (2, 3):
        raise ValueError(f"{path}: GGUF version {version} is not supported (2 and 3 are)")
    n_tensors, n_kv = c.take("<Q"), c.take("<Q")
    meta = {}
    for _ in range(n_kv):
        k = c.string()
        meta[k] = c.value(c.take("<I"))
    infos = []
    for _ in range(n_tensors):
        name = c.string()
        nd = c.take("<I")
        if not 1 <= nd <= 4:
            raise ValueError(f"{path}: tensor {name} has {nd} dimensions")
        ne = [c.take("<Q") for _ in range(nd)]
        infos.append((name, ne, c.take("<I"), c.take("<Q")))
    align = int(meta.get("general.alignment", 32))
    if align < 8 or align & (align - 1):
        raise ValueError(f"{path}: general.alignment {align} is not a power of two >= 8")
    data0 = (c.o + align - 1) // align * align
    out = {}
    for name, ne, t, off in infos:
        if t not in GGML_TYPES:
            raise ValueError(f"{path}: tensor {name} has ggml type {t}, which is not read")
        _, bs, bb = GGML_TYPES[t]
        numel = 1
        for x in ne:
            numel *= x
        if ne[0] % bs or off % align:
            raise ValueError(f"{path}: tensor {name}: row length {ne[0]} / offset {off} do not fit block {bs} / alignment {align}")
        nb = numel // bs * bb
        if data0 + off + nb > len(buf):
            raise ValueError(f"{path}: tensor {name} runs past the end of the file")
        if name in out:
            raise ValueError(f"{path}: tensor {name} appears twice")
        out[name] = (t, tuple(reversed(ne)), buf[data0 + off:data0 + off + nb])
    return meta, out


def read_gguf(path, rows=None):
    """-> (meta, {name: float32 array}).  rows: {name: n} converts only the first n rows of those (2-D) tensors -- the
    talker's token_embd / output are padded to the text vocabulary and only the codec rows are used."""
    meta, raw = read_gguf_raw(path)
    out = {}
    for name, (t, shape, data) in raw.items():
        if rows and name in rows and len(shape) == 2 and shape[0] > rows[name]:
            _, bs, bb = GGML_TYPES[t]
            shape = (rows[name], shape[1])
            data = data[:shape[0] * (shape[1] // bs) * bb]
        out[name] = dequantize(t, np.asarray(data), int(np.prod(shape, dtype=np.int64))).reshape(shape)
    return meta, out


def talker_tensors(path, talker_vocab=3072):
    """The talker of a qwen3 GGUF under the container's names: norm vectors float32, matrices float16 (round to nearest
    even, saturating at +-65504: the fp16 weights the native loader makes), talker.codec_embedding float32."""
    meta, t = read_gguf(path, rows={"token_embd.weight": talker_vocab, "output.weight": talker_vocab})
    if meta.get("general.architecture") != "qwen3":
        raise ValueError(f"{path}: general.architecture is {meta.get('general.architecture')!r}, not 'qwen3'")
    f16 = lambda a: np.clip(a, -65504.0, 65504.0).astype(np.float16)
    out = {}
    for name, a in t.items():
        parts = name.split(".")
        if len(parts) == 4 and parts[0] == "blk" and parts[1].isdigit() and parts[2] in GGUF_LAYER_PARTS and parts[3] == "weight":
            out[f"talker.layers.{int(parts[1])}.{GGUF_LAYER_PARTS[parts[2]]}"] = a if a.ndim == 1 else f16(a)
    out["talker.norm"] = t["output_norm.weight"]
    out["talker.codec_embedding"] = t["token_embd.weight"]
    out["talker.codec_head"] = f16(t["output.weight"] if "output.weight" in t else t["token_embd.weight"])
    return meta, out
