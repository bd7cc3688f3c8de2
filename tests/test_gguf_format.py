"""The talker's GGUF on the host: qwen3_tts_axera_russian_amd/gguf.py (numpy) and the native parser (Pack::add_gguf_bytes,
Pack::open_auto in csrc/q3_formats.cpp).  CPU only.

  1. gguf.py's float32 values against tests/gguf_ref.py's float64 formulas, bit for bit, per type
  2. the metadata keys the parser reads are the ones transformers' qwen3 GGUF table knows
  3. tests/gguf_host_driver.cpp -- a program of its own, built like tests/test_native_formats_malformed.py builds its driver
     (ROCm's clang++, -fsanitize=address,undefined -fno-sanitize-recover=undefined, nothing loaded into Python) -- prints what
     the parser made of a file: it must be what the writer put in, for v2 / v3, alignments 32 / 64, 1- to 4-D tensors
  4. a catalogue of damaged files, one per refusal of the parser; every proper prefix of a small valid file; seeded
     single-byte mutants of its header region
  5. open_auto: a .gguf file, a directory with one, a directory with two (refused), .npy tables in aux_dir (they win)
"""
import os
import struct
import subprocess

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import gguf as G
from tests import gguf_ref as R
from tests.test_native_formats_malformed import driver_env, fnv1a, rocm_clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen3_tts_axera_russian_amd", "csrc")
N_MUTANTS = 400


# ---------------------------------------------------------------------------------------------------------------------
# 1. gguf.py against the float64 formulas

def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("tname", R.BLOCK_TYPES)
def test_numpy_reader_values_are_the_float64_formulas_rounded_once(tname):
    rng = np.random.default_rng(7)
    blocks = np.concatenate([R.edge_blocks(tname), R.random_blocks(tname, 3000, rng), R.random_blocks(tname, 500, rng, scale=0.02)])
    n = blocks.shape[0] * R.TYPES[tname][2]
    got = G.dequantize(R.TYPES[tname][0], blocks.reshape(-1), n)
    want = R.dequant64(tname, blocks).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(bits(got), bits(want))
    assert np.isfinite(want).all() and np.abs(want).max() > 65504     # (the range the fp16 rounding has to saturate)


def test_numpy_reader_plain_types_and_file_layout(tmp_path):
    rng = np.random.default_rng(8)
    f32 = rng.standard_normal((3, 5)).astype(np.float32)
    f16 = rng.standard_normal((2, 7)).astype(np.float16)
    bf = rng.integers(0, 0x7f80, (4, 3), dtype=np.uint16)
    q = R.random_blocks("Q4_K", 6, rng)
    data, _ = R.gguf_bytes(R.qwen3_kvs(), [("a", "F32", (3, 5), f32.tobytes()), ("b", "F16", (2, 7), f16.tobytes()),
                                           ("c", "BF16", (4, 3), bf.tobytes()), ("d", "Q4_K", (3, 512), q.tobytes())], alignment=64)
    p = tmp_path / "x.gguf"
    p.write_bytes(data)
    meta, t = G.read_gguf(str(p))
    assert meta["general.architecture"] == "qwen3" and meta["qwen3.block_count"] == 2 and meta["general.alignment"] == 64
    assert meta["tokenizer.ggml.tokens"] == ["a", "bc", "", "d" * 9]
    np.testing.assert_array_equal(t["a"], f32)
    np.testing.assert_array_equal(t["b"], f16.astype(np.float32))
    np.testing.assert_array_equal(bits(t["c"]), bf.astype(np.uint32) << 16)
    np.testing.assert_array_equal(bits(t["d"]), bits(R.dequant64("Q4_K", q, 512).astype(np.float32)))
    _, part = G.read_gguf(str(p), rows={"d": 2})
    np.testing.assert_array_equal(part["d"], t["d"][:2])


# ---------------------------------------------------------------------------------------------------------------------
# 2. metadata keys

def test_metadata_keys_are_the_ones_transformers_knows():
    ggml = pytest.importorskip("transformers.integrations.ggml")
    known = set(ggml.GGUF_CONFIG_MAPPING["qwen3"])
    src = open(os.path.join(CSRC, "q3_formats.cpp")).read()
    for key in G.GGUF_META_KEYS:
        assert '"%s"' % key in src, key                      # the parser reads exactly gguf.py's list
        arch, suffix = key.split(".", 1)
        assert arch == "qwen3"
        if suffix == "attention.key_length":                 # llama.cpp's key for head_dim; transformers derives it instead
            continue
        assert suffix in known, key
    assert '"general.alignment"' in src and '"general.architecture"' in src


# ---------------------------------------------------------------------------------------------------------------------
# 3. - 5. the native parser through the driver

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx, root = rocm_clang()
    exe = str(tmp_path_factory.mktemp("gguf_host") / "gguf_host_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include"), "-Wno-unused-value",
                           os.path.join(ROOT, "tests", "gguf_host_driver.cpp"), os.path.join(CSRC, "q3_formats.cpp"),
                           os.path.join(CSRC, "q3_common.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "lib"), "-Wl,-rpath," + os.path.join(root, "lib"), "-lamdhip64", "-lz"])
    return exe


def run_jobs(driver, workdir, jobs, timeout=300):
    """-> per job None (refused) or ({name: (dtype, shape, offset, nbytes, hash)}, meta).  Fails, naming the job, on
    anything else: a signal, a sanitizer report, a non-zero exit."""
    lst = os.path.join(str(workdir), "jobs_%d.txt" % len(os.listdir(str(workdir))))
    with open(lst, "w") as f:
        f.write("\n".join(jobs) + "\n")
    p = subprocess.run([driver, "jobs", lst], capture_output=True, text=True, errors="replace", env=driver_env(), timeout=timeout)
    res, lines, i = [], p.stdout.splitlines(), 0
    while i < len(lines) and len(res) < len(jobs):
        assert lines[i] == "job " + jobs[len(res)], (lines[i], jobs[len(res)])
        i += 1
        if i < len(lines) and lines[i] == "refused":
            res.append(None)
            i += 1
        elif i < len(lines) and lines[i].startswith("accepted "):
            tens, meta = {}, {}
            i += 1
            while i < len(lines) and lines[i] != "end":
                f = lines[i].split()
                if f[0] == "meta":
                    meta[f[1]] = float(f[2])
                else:
                    tens[f[0]] = (int(f[1]), tuple(int(x) for x in f[3:3 + int(f[2])]), int(f[7]), int(f[8]), int(f[9], 16))
                i += 1
            if i == len(lines):
                break
            i += 1
            res.append((tens, meta))
        else:
            break
    if p.returncode != 0 or len(res) != len(jobs):
        pytest.fail("input `%s`: the driver ended with %s, neither refusing nor accepting it\n%s"
                    % (jobs[min(len(res), len(jobs) - 1)], p.returncode, p.stderr[-6000:]))
    return res


def one(driver, tmp_path, data, name="input.gguf"):
    path = tmp_path / name
    path.write_bytes(data)
    return run_jobs(driver, tmp_path, ["gguf %s heap" % path])[0]


def raw_of(tname, shape, rng):
    n = int(np.prod(shape))
    if tname in R.BLOCK_TYPES:
        return R.random_blocks(tname, n // R.TYPES[tname][2], rng).tobytes()
    return rng.integers(0, 256, R.nbytes_of(tname, shape), dtype=np.uint8).tobytes()


def small_talker(rng, mat="Q4_K", layers=1, hidden=256, ffn=512, heads=2, kv=1, hd=128, vocab=40, tied=False, extra=()):
    """A small file with every tensor name of the qwen3 talker (the parser checks no width: the loader does)."""
    t = []
    for i in range(layers):
        for part, shape in (("attn_norm", (hidden,)), ("attn_q", (heads * hd, hidden)), ("attn_k", (kv * hd, hidden)),
                            ("attn_v", (kv * hd, hidden)), ("attn_output", (hidden, heads * hd)), ("attn_q_norm", (hd,)),
                            ("attn_k_norm", (hd,)), ("ffn_norm", (hidden,)), ("ffn_gate", (ffn, hidden)), ("ffn_up", (ffn, hidden)),
                            ("ffn_down", (hidden, ffn))):
            tn = "F32" if len(shape) == 1 else mat
            t.append(("blk.%d.%s.weight" % (i, part), tn, shape, raw_of(tn, shape, rng)))
    t.append(("output_norm.weight", "F32", (hidden,), raw_of("F32", (hidden,), rng)))
    t.append(("token_embd.weight", mat, (vocab, hidden), raw_of(mat, (vocab, hidden), rng)))
    if not tied:
        t.append(("output.weight", "Q6_K" if mat == "Q4_K" else mat, (vocab, hidden), raw_of("Q6_K" if mat == "Q4_K" else mat, (vocab, hidden), rng)))
    t.extend(extra)
    return t, R.qwen3_kvs(layers=layers, hidden=hidden, ffn=ffn, heads=heads, kv_heads=kv, head_dim=hd)


NAMES = {"attn_norm": "input_ln", "attn_q": "q_proj", "attn_k": "k_proj", "attn_v": "v_proj", "attn_output": "o_proj",
         "attn_q_norm": "q_norm", "attn_k_norm": "k_norm", "ffn_norm": "post_ln", "ffn_gate": "gate_proj", "ffn_up": "up_proj",
         "ffn_down": "down_proj"}


def container_name(n):
    if n.startswith("blk."):
        _, i, part, _ = n.split(".")
        return "talker.layers.%s.%s" % (i, NAMES[part])
    return {"output_norm.weight": "talker.norm", "token_embd.weight": "talker.codec_embedding", "output.weight": "talker.codec_head"}.get(n)


@pytest.mark.parametrize("version", [2, 3])
@pytest.mark.parametrize("alignment", [32, 64])
def test_parser_reports_what_the_writer_put_in(driver, tmp_path, version, alignment):
    rng = np.random.default_rng(100 + version + alignment)
    # 3- and 4-D tensors under names of the talker (plain types: a block type that is not a matrix is refused)
    tens, kvs = small_talker(rng, mat="Q4_K", layers=2)
    tens = [x for x in tens if x[0] not in ("blk.1.attn_q_norm.weight", "blk.1.attn_k_norm.weight")]
    tens += [("blk.1.attn_q_norm.weight", "F16", (2, 4, 16), raw_of("F16", (2, 4, 16), rng)),
             ("blk.1.attn_k_norm.weight", "BF16", (2, 2, 2, 16), raw_of("BF16", (2, 2, 2, 16), rng)),
             ("rope_freqs.weight", "F32", (64,), raw_of("F32", (64,), rng))]                 # no name of this model: skipped
    for i, mat in enumerate(("Q4_0", "Q8_0", "Q5_K", "Q6_K")):                             # every block type once
        nm = "blk.0.%s.weight" % ("attn_q", "attn_k", "attn_v", "ffn_down")[i]
        tens = [(n, mat, s, raw_of(mat, s, rng)) if n == nm else (n, tn, s, r) for n, tn, s, r in tens]
    data, place = R.gguf_bytes(kvs, tens, version=version, alignment=alignment)
    got = one(driver, tmp_path, data)
    assert got is not None
    tensors, meta = got
    want = {container_name(n): (R.TYPES[tn][1], tuple(s), place[n][0], place[n][1], fnv1a(r)) for n, tn, s, r in tens if container_name(n)}
    assert tensors == want
    assert {tn for _, tn, _, _ in tens} == set(R.TYPES)        # every type the parser reads was in the file
    assert meta == {"talker_layers": 2, "hidden": 256, "talker_ffn": 512, "n_heads": 2, "n_kv_heads": 1, "head_dim": 128,
                    "rms_eps": float(np.float32(1e-6)), "rope_theta": 1e6, "gguf_version": version, "gguf_alignment": alignment}
    for _, (dtype, shape, off, nb, _) in tensors.items():
        assert off % alignment == 0


def test_tied_embeddings_fall_back_to_token_embd(driver, tmp_path):
    rng = np.random.default_rng(5)
    tens, kvs = small_talker(rng, tied=True)
    got = one(driver, tmp_path, R.gguf_bytes(kvs, tens)[0])
    assert got is not None and got[0]["talker.codec_head"] == got[0]["talker.codec_embedding"]


def patched(data, offset, fmt, value):
    b = bytearray(data)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def catalogue():
    """name -> damaged file bytes; every refusal the parser knows has an entry"""
    rng = np.random.default_rng(11)
    tens, kvs = small_talker(rng)
    good, place = R.gguf_bytes(kvs, tens)
    c = {}
    c["bad magic"] = R.gguf_bytes(kvs, tens, magic=b"GGUL")[0]
    c["version 1"] = R.gguf_bytes(kvs, tens, version=1)[0]
    c["version 4"] = R.gguf_bytes(kvs, tens, version=4)[0]
    c["big-endian version"] = patched(good, 4, ">I", 3)
    c["tensor count beyond the file"] = R.gguf_bytes(kvs, tens, n_tensors=1 << 60)[0]
    c["kv count beyond the file"] = R.gguf_bytes(kvs, tens, n_kv=1 << 61)[0]
    c["one kv too many"] = R.gguf_bytes(kvs, tens, n_kv=len(kvs) + 1)[0]
    c["one tensor too many"] = R.gguf_bytes(kvs, tens, n_tensors=len(tens) + 1)[0]
    c["key length beyond the file"] = patched(good, 24, "<Q", 1 << 40)
    c["key length 2^64-1"] = patched(good, 24, "<Q", (1 << 64) - 1)
    # the first value is the architecture string: its length field follows the key and the type
    v0 = 24 + 8 + len("general.architecture") + 4
    c["string value beyond the file"] = patched(good, v0, "<Q", len(good))
    c["unknown value type"] = b"GGUF" + struct.pack("<IQQ", 3, 1, 1) + R.gstr("x") + struct.pack("<I", 13) + b"\0" * 64
    c["array of arrays"] = R.gguf_bytes([kvs[0], ("x", R.ARR, (R.ARR, []))], tens)[0]
    c["array count beyond the file"] = R.gguf_bytes([kvs[0]], tens)[0][:24] + R.kv_bytes(*kvs[0]) + R.gstr("x") + struct.pack("<IIQ", R.ARR, R.U32, 1 << 62)
    c["string array count beyond the file"] = R.gguf_bytes([kvs[0]], tens)[0][:24] + R.kv_bytes(*kvs[0]) + R.gstr("x") + struct.pack("<IIQ", R.ARR, R.STR, 1 << 62) + b"\0" * 64
    c["array of unknown element type"] = R.gguf_bytes([kvs[0], ("x", R.ARR, (R.U8, []))], tens)[0].replace(
        R.gstr("x") + struct.pack("<II", R.ARR, R.U8), R.gstr("x") + struct.pack("<II", R.ARR, 99))
    c["architecture llama"] = R.gguf_bytes(R.qwen3_kvs(layers=1, hidden=256, ffn=512, heads=2, kv_heads=1, arch="llama"), tens)[0]
    c["no architecture"] = R.gguf_bytes(kvs[1:], tens)[0]
    for a in (0, 1, 4, 24, 48, 1 << 31):
        c["alignment %d" % a] = R.gguf_bytes(kvs + [("general.alignment", R.U32, a)], tens)[0]
    c["rope base 10000"] = R.gguf_bytes(R.qwen3_kvs(layers=1, hidden=256, ffn=512, heads=2, kv_heads=1, theta=1e4), tens)[0]
    c["epsilon 1e-5"] = R.gguf_bytes(R.qwen3_kvs(layers=1, hidden=256, ffn=512, heads=2, kv_heads=1, eps=1e-5), tens)[0]
    for key, kw in (("block_count", dict(layers=3)), ("embedding_length", dict(hidden=512)), ("feed_forward_length", dict(ffn=1024)),
                    ("head_count", dict(heads=4)), ("head_count_kv", dict(kv_heads=2)), ("key_length", dict(head_dim=64))):
        args = dict(layers=1, hidden=256, ffn=512, heads=2, kv_heads=1, head_dim=128)
        args.update(kw)
        c["metadata contradicts the tensors: " + key] = R.gguf_bytes(R.qwen3_kvs(**args), tens)[0]
    # tensor infos: built by hand behind a valid header
    head = b"GGUF" + struct.pack("<IQQ", 3, 1, 1) + R.kv_bytes(*kvs[0])
    pad = lambda h: h + b"\0" * ((-len(h)) % 32)
    q = R.random_blocks("Q4_K", 2, rng).tobytes()
    c["0 dimensions"] = pad(head + R.gstr("token_embd.weight") + struct.pack("<I", 0) + struct.pack("<IQ", 0, 0)) + b"\0" * 64
    c["5 dimensions"] = pad(head + R.info_bytes("token_embd.weight", [2, 2, 2, 2, 2], 0, 0)) + b"\0" * 128
    c["dimension product overflows"] = pad(head + R.info_bytes("token_embd.weight", [1 << 33, 1 << 33], 0, 0)) + b"\0" * 64
    c["byte count overflows"] = pad(head + R.info_bytes("token_embd.weight", [1 << 31, 1 << 31, 2], 0, 0)) + b"\0" * 64
    c["row no multiple of the block"] = pad(head + R.info_bytes("token_embd.weight", [128, 4], 12, 0)) + q
    c["row no multiple of 32"] = pad(head + R.info_bytes("token_embd.weight", [48, 2], 8, 0)) + b"\0" * 102
    c["misaligned offset"] = pad(head + R.info_bytes("token_embd.weight", [256, 2], 12, 16)) + b"\0" * 16 + q
    c["tensor past the end"] = pad(head + R.info_bytes("token_embd.weight", [256, 2], 12, 0)) + q[:-1]
    c["offset past the end"] = pad(head + R.info_bytes("token_embd.weight", [256, 2], 12, 1 << 40)) + q
    c["offset near 2^64"] = pad(head + R.info_bytes("token_embd.weight", [256, 2], 12, (1 << 64) - 32)) + q
    c["data start past the end"] = head + R.info_bytes("token_embd.weight", [256, 2], 12, 0) + b"\0"
    for num, nm in ((3, "Q4_1"), (6, "Q5_0"), (10, "Q2_K"), (11, "Q3_K"), (15, "Q8_K"), (16, "IQ2_XXS"), (20, "IQ4_NL"), (24, "I8"), (28, "F64"),
                    (39, "MXFP4"), (40, "unknown"), (0xffffffff, "unknown")):
        c["ggml type %d (%s)" % (num, nm)] = pad(head + R.info_bytes("token_embd.weight", [256, 2], num, 0)) + b"\0" * 1024
    c["block type, 1-D"] = pad(head + R.info_bytes("output_norm.weight", [512], 12, 0)) + q
    c["block type, 3-D"] = pad(head + R.info_bytes("token_embd.weight", [256, 1, 2], 12, 0)) + q
    two = b"GGUF" + struct.pack("<IQQ", 3, 2, 1) + R.kv_bytes(*kvs[0])
    c["duplicate tensor name"] = pad(two + R.info_bytes("token_embd.weight", [256, 1], 12, 0) + R.info_bytes("token_embd.weight", [256, 1], 12, 160)) + q + b"\0" * 16 + q
    c["no tensor of the talker"] = pad(head + R.info_bytes("rope_freqs.weight", [64], 0, 0)) + b"\0" * 256
    c["empty file"] = b""
    c["magic only"] = b"GGUF"
    return good, c


def test_every_refusal_has_a_catalogue_entry_and_is_refused(driver, tmp_path):
    good, cat = catalogue()
    names = sorted(cat)
    jobs = []
    for i, nm in enumerate(names):
        p = tmp_path / ("bad_%03d.gguf" % i)
        p.write_bytes(cat[nm])
        jobs.append("gguf %s heap" % p)
    (tmp_path / "good.gguf").write_bytes(good)
    jobs.append("gguf %s heap" % (tmp_path / "good.gguf"))
    res = run_jobs(driver, tmp_path, jobs)
    accepted = [nm for nm, r in zip(names, res) if r is not None]
    assert not accepted, accepted
    assert res[-1] is not None and len(res[-1][0]) == 14        # (or "refuse everything" would pass)
    # one Q3_LOG line per refusal, naming number and name of an unread type
    p = tmp_path / "q2k.gguf"
    p.write_bytes(cat["ggml type 10 (Q2_K)"])
    lst = tmp_path / "single.txt"
    lst.write_text("gguf %s heap\n" % p)
    r = subprocess.run([driver, "jobs", str(lst)], capture_output=True, text=True, env=driver_env())
    logs = [ln for ln in r.stderr.splitlines() if ln.startswith("[qwen3tts]")]
    assert r.returncode == 0 and len(logs) == 1 and "ggml type 10 (Q2_K)" in logs[0], r.stderr


def test_every_prefix_and_header_mutants(driver, tmp_path):
    rng = np.random.default_rng(21)
    tens, kvs = small_talker(rng, mat="Q8_0", hidden=32, ffn=32, heads=1, kv=1, hd=32, vocab=2)
    kvs = R.qwen3_kvs(layers=1, hidden=32, ffn=32, heads=1, kv_heads=1, head_dim=32)
    good, place = R.gguf_bytes(kvs, tens)
    data0 = min(o for o, _ in place.values())
    p = tmp_path / "small.gguf"
    p.write_bytes(good)
    res = run_jobs(driver, tmp_path, ["gguf %s trunc %d" % (p, k) for k in range(len(good))] + ["gguf %s heap" % p])
    assert res[-1] is not None
    assert all(r is None for r in res[:data0])                 # no prefix of the header region parses
    assert all(r is None for r in res[:-1])                    # nor one that cuts the last tensor's data short
    jobs = []
    mrng = np.random.default_rng(22)
    for i in range(N_MUTANTS):
        b = bytearray(good)
        o = int(mrng.integers(0, data0))
        b[o] = int(mrng.choice([0, 1, 0x7f, 0x80, 0xff, int(mrng.integers(0, 256)), b[o] ^ (1 << int(mrng.integers(0, 8)))]))
        q = tmp_path / ("mut_%04d.gguf" % i)
        q.write_bytes(bytes(b))
        jobs.append("gguf %s heap" % q)
    res = run_jobs(driver, tmp_path, jobs)                     # refused or accepted-and-consistent, no report, exit 0
    assert any(r is None for r in res) and any(r is not None for r in res)


def test_open_auto_file_directory_and_npy_tables(driver, tmp_path):
    rng = np.random.default_rng(31)
    tens, kvs = small_talker(rng, hidden=256, ffn=256, heads=2, kv=1, vocab=3080)   # tables padded past the 3072 codec rows
    data, place = R.gguf_bytes(kvs, tens)
    f = tmp_path / "talker_q4_k_m.gguf"
    f.write_bytes(data)
    bare = tmp_path / "no_suffix.bin"           # found by its magic
    bare.write_bytes(data)
    d1 = tmp_path / "one"
    d1.mkdir()
    (d1 / "qwen3_tts_talker_q4_k_m.gguf").write_bytes(data)
    d2 = tmp_path / "two"
    d2.mkdir()
    (d2 / "a.gguf").write_bytes(data)
    (d2 / "b.gguf").write_bytes(data)
    aux = tmp_path / "embeddings"
    aux.mkdir()
    emb = rng.standard_normal((3072, 256)).astype(np.float16)
    head = rng.standard_normal((3072, 256)).astype(np.float16)
    np.save(aux / "codec_embedding.npy", emb)
    np.save(aux / "codec_head.npy", head)
    r_file, r_bare, r_dir, r_two, r_aux, r_dir_aux = run_jobs(driver, tmp_path, [
        "auto %s" % f, "auto %s" % bare, "auto %s" % d1, "auto %s" % d2, "auto %s %s" % (f, aux), "auto %s %s" % (d1, aux)])
    assert r_two is None
    assert r_file is not None and r_file == r_bare == r_dir
    tensors, meta = r_file
    raw = {n: r for n, _, _, r in tens}
    # only the codec rows of the padded tables: rows are contiguous runs of blocks
    q4 = 3072 * 256 // 256 * 144
    assert tensors["talker.codec_embedding"][:2] == (R.TYPES["Q4_K"][1], (3072, 256))
    assert tensors["talker.codec_embedding"][3:] == (q4, fnv1a(raw["token_embd.weight"][:q4]))
    q6 = 3072 * 256 // 256 * 210
    assert tensors["talker.codec_head"][:2] == (R.TYPES["Q6_K"][1], (3072, 256))
    assert tensors["talker.codec_head"][3:] == (q6, fnv1a(raw["output.weight"][:q6]))
    assert meta["talker_layers"] == 1 and meta["talker_ffn"] == 256 and meta["hidden"] == 256
    # the exact .npy tables win over the GGUF's quantised copies; everything else is the GGUF's
    for r in (r_aux, r_dir_aux):
        assert r is not None
        assert r[0]["talker.codec_embedding"] == (1, (3072, 256), -1, emb.nbytes, fnv1a(emb.tobytes()))
        assert r[0]["talker.codec_head"] == (1, (3072, 256), -1, head.nbytes, fnv1a(head.tobytes()))
        rest = {k: v for k, v in r[0].items() if k not in ("talker.codec_embedding", "talker.codec_head")}
        assert rest == {k: v for k, v in tensors.items() if k not in ("talker.codec_embedding", "talker.codec_head")}
    lst = tmp_path / "single.txt"
    lst.write_text("auto %s %s\n" % (f, aux))
    err = subprocess.run([driver, "jobs", str(lst)], capture_output=True, text=True, env=driver_env()).stderr
    assert err.count("not from the GGUF's quantised copy") == 2, err


# ---------------------------------------------------------------------------------------------------------------------
# the converter: one container from a deployment that holds only the GGUF

def test_from_reference_dirs_takes_the_talker_from_a_gguf(tmp_path):
    from qwen3_tts_axera_russian_amd import weights as W
    rng = np.random.default_rng(41)
    cfg = W.ModelConfig(talker_layers=2, cp_layers=0, cp_groups=0, hidden=256, talker_ffn=512, n_heads=2, n_kv_heads=1, talker_vocab=24,
                        text_vocab=10, text_dim=8)
    tens, kvs = small_talker(rng, layers=2, vocab=40)
    tens = [(n, tn, s, rng.standard_normal(s).astype(np.float32).tobytes() if tn == "F32" else r) for n, tn, s, r in tens]
    g = tmp_path / "talker_q4_k_m.gguf"
    g.write_bytes(R.gguf_bytes(kvs, tens)[0])
    emb = tmp_path / "embeddings"
    emb.mkdir()
    tables = {"text_embedding": (10, 8), "text_projection_linear_fc1_weight": (8, 8), "text_projection_linear_fc1_bias": (8,),
              "text_projection_linear_fc2_weight": (256, 8), "text_projection_linear_fc2_bias": (256,), "codec_embedding": (24, 256),
              "codec_head": (24, 256)}
    npy = {k: rng.standard_normal(s).astype(np.float32) for k, s in tables.items()}
    for k, a in npy.items():
        np.save(emb / (k + ".npy"), a)
    cp = tmp_path / "code_predictor"
    cp.mkdir()
    np.savez(cp / "code_predictor_weights.npz", final_norm=np.ones(256, np.float32))
    out = str(tmp_path / "deployed.q3w")
    W.from_reference_dirs(str(emb), str(cp), None, out, cfg, talker_gguf=str(g))
    _, t = W.read_pack(out)
    for n, tn, shape, raw in tens:
        want = R.dequant64(tn, raw).astype(np.float32).reshape(shape)
        cn = container_name(n)
        if cn in ("talker.codec_embedding", "talker.codec_head"):
            continue
        got = np.asarray(t[cn])
        if len(shape) == 1:
            assert got.dtype == np.float32
            np.testing.assert_array_equal(bits(got), bits(want))
        else:
            assert got.dtype == np.float16
            np.testing.assert_array_equal(got.view(np.uint16), R.f16_sat(want).view(np.uint16))
    # the codec tables stay the exact .npy ones
    np.testing.assert_array_equal(np.asarray(t["talker.codec_embedding"]), npy["codec_embedding"])
    np.testing.assert_array_equal(np.asarray(t["talker.codec_head"]), npy["codec_head"].astype(np.float16))
    # the tables of the GGUF itself: only the codec rows are converted
    _, tt = G.talker_tensors(str(g), talker_vocab=24)
    raw = {n: (tn, s, r) for n, tn, s, r in tens}
    tn, s, r = raw["output.weight"]
    np.testing.assert_array_equal(tt["talker.codec_head"], R.f16_sat(R.dequant64(tn, r, s[1])[:24].astype(np.float32)))
    with pytest.raises(ValueError):
        W.from_reference_dirs(str(emb), str(cp), "x.safetensors", out, cfg, talker_gguf=str(g))
