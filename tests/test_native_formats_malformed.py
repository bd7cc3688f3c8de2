"""Malformed and unusual weight files against the native readers (csrc/q3_formats.cpp: .npy, .npz, .safetensors;
Pack::open_bytes in csrc/q3_common.cpp: the Q3TTSW1 container), under AddressSanitizer and UBSan.

tests/formats_host_driver.cpp is built once per module from the driver and the two reader sources with ROCm's clang++ (the
one the product is built with: q3_common.h needs _Float16) and `-fsanitize=address,undefined -fno-sanitize-recover=undefined`.
It is a stand-alone program, run on the CPU: it calls no HIP function, is never loaded into Python, and nothing is preloaded
into it.  Every input is copied into a malloc'd buffer of exactly its size and parsed through the readers' bytes-level
entries, so the first byte read past the end of a file is a sanitizer report (it is not for a mapping).  An input either is
`refused`, or is `accepted` with every tensor consistent (checked by the driver in 128-bit arithmetic: nbytes == numel *
element size, data inside the input or an owned buffer) and every byte of it read.  Anything else -- a signal, a sanitizer
report, an uncaught exception, a non-zero exit, a time limit -- fails the input, with the driver's stderr shown.

  a. a catalogue of hand-made damaged files, each of which must be refused
  b. legitimate unusual files, which must stay accepted with the right bytes (or "refuse everything" would pass a.)
  c. every prefix of one small valid file per format
  d. 5000 seeded single-field mutants per format of the same files ("a few thousand" were asked for; at 0.1 ms a
     mutant under the sanitizers the count is not what costs time, so it was not brought down)
  e. h2f on all 65536 patterns and f2h_sat on ~450 000 floats against the compiler's _Float16 conversions

Files are written with numpy, zipfile, safetensors and struct.  CPU only.  Measured on an 8-core CPU machine: the whole
file 12-14 s, of which the sanitized build of the driver 4.5 s (once per module) and the slowest test function, the
20 000 mutants, 3-5 s (most of it writing the files)."""
import io
import json
import os
import random
import shutil
import struct
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen3_tts_axera_russian_amd", "csrc")
N_MUTANTS = 5000


def rocm_clang():
    """ROCm's clang++: beside hipcc, which is located as build.py locates it."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for c in (os.path.join(root, "lib", "llvm", "bin", "clang++"), os.path.join(root, "llvm", "bin", "clang++"),
              os.path.join(root, "bin", "amdclang++"), os.path.join(os.path.dirname(os.path.realpath(hipcc)), "clang++")):
        if os.path.exists(c):
            return c, root
    raise AssertionError("no clang++ beside %s" % hipcc)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx, root = rocm_clang()
    exe = str(tmp_path_factory.mktemp("formats_host") / "formats_host_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include"), "-Wno-unused-value",
                           os.path.join(ROOT, "tests", "formats_host_driver.cpp"), os.path.join(CSRC, "q3_formats.cpp"),
                           os.path.join(CSRC, "q3_common.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "lib"), "-Wl,-rpath," + os.path.join(root, "lib"), "-lamdhip64", "-lz"])
    return exe


def driver_env():
    return dict(os.environ, Q3_KEEP_HW_QUEUES="1")     # (the library's load-time note about hardware queues stays out of stderr)


def run_jobs(driver, workdir, jobs, timeout=300):
    """-> per job None (refused) or (tensors, meta) as tests/test_native_formats.py's inspect() gives them.  Fails, naming
    the job, on anything else."""
    lst = os.path.join(str(workdir), "jobs_%d.txt" % len(os.listdir(str(workdir))))
    with open(lst, "w") as f:
        f.write("\n".join(jobs) + "\n")
    p = subprocess.Popen([driver, "jobs", lst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace",
                         env=driver_env())
    try:
        out, err = p.communicate(timeout=timeout)
        rc = p.returncode
    except subprocess.TimeoutExpired:
        p.kill()
        out, err = p.communicate()
        rc = "time limit"
    res, lines, i = [], out.splitlines(), 0
    while i < len(lines):
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
                    tens[f[0]] = (int(f[1]), tuple(int(x) for x in f[3:3 + int(f[2])]), int(f[7], 16))
                i += 1
            if i == len(lines):
                break   # ended inside the inventory
            i += 1
            res.append((tens, meta))
        else:
            break       # the job that ended the driver
    if rc != 0 or len(res) != len(jobs):
        pytest.fail("input `%s`: the driver ended with %s, neither refusing nor accepting it\n%s"
                    % (jobs[min(len(res), len(jobs) - 1)], rc, err[-6000:]))
    return res


def one(driver, tmp_path, fmt, data, name="input"):
    path = tmp_path / name
    path.write_bytes(data)
    return run_jobs(driver, tmp_path, ["%s %s heap" % (fmt, path)])[0]


def fnv1a(b: bytes) -> int:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def entry(a, dtype_code=None):
    code = {np.dtype(np.float32): 0, np.dtype(np.float16): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3}
    return (code[a.dtype] if dtype_code is None else dtype_code, a.shape, fnv1a(a.tobytes()))


# ---------------------------------------------------------------------------------------------------------------------
# writers

def npy_bytes(a, version=None):
    f = io.BytesIO()
    np.lib.format.write_array(f, np.asarray(a), version=version)
    return f.getvalue()


def raw_npy(header: str, payload=b"", major=1):
    h = header.encode("latin1")
    return b"\x93NUMPY" + bytes([major, 0]) + struct.pack("<H" if major == 1 else "<I", len(h)) + h + payload


def npy_header_text(descr, shape):
    return "{'descr': '%s', 'fortran_order': False, 'shape': %s, }\n" % (descr, shape)


def raw_st(header, payload=b""):
    h = header if isinstance(header, bytes) else json.dumps(header).encode()
    return struct.pack("<Q", len(h)) + h + payload


ST_KEY = "talker.model.norm.weight"        # -> talker.norm (csrc/q3_formats.cpp, map_safetensors_key)


def raw_container(recs, size, meta=(), n_tensors=None, n_meta=None):
    """recs: (name, dtype, ndim, shape[4], offset, nbytes).  The bytes after the tables are 1, 2, 3, ..."""
    b = struct.pack("<8sIIIIQ", b"Q3TTSW1\0", 1, len(recs) if n_tensors is None else n_tensors,
                    len(meta) if n_meta is None else n_meta, 0, 256)
    for k, v in meta:
        b += struct.pack("<48sd", k.encode(), v)
    for name, dt, nd, shape, off, nb in recs:
        b += struct.pack("<96sII4QQQ", name.encode(), dt, nd, *shape, off, nb)
    assert len(b) <= size
    return b + bytes((i + 1) & 0xff for i in range(size - len(b)))


class Zip:
    """A zip archive written field by field, so that any one field can lie.  members: name -> (.npy bytes, method)."""

    def __init__(self, members):
        self.body, self.entries = b"", []
        for name, (data, method) in members.items():
            comp = data if method == 0 else zlib.compress(data, 9)[2:-4]       # raw deflate
            nm = name.encode()
            self.entries.append(dict(method=method, crc=zlib.crc32(data), csize=len(comp), usize=len(data), nlen=len(nm),
                                     name=nm, extra=b"", xlen=None, comment=b"", lho=len(self.body)))
            self.body += struct.pack("<IHHHHHIIIHH", 0x04034b50, 20, 0, method, 0, 0x21, zlib.crc32(data), len(comp), len(data),
                                     len(nm), 0) + nm + comp

    def central(self):
        cd = b""
        for e in self.entries:
            xlen = len(e["extra"]) if e["xlen"] is None else e["xlen"]
            cd += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014b50, 20, 20, 0, e["method"], 0, 0x21, e["crc"], e["csize"], e["usize"],
                              e["nlen"], xlen, len(e["comment"]), 0, 0, 0, e["lho"]) + e["name"] + e["extra"] + e["comment"]
        return cd

    def bytes(self, n_ent=None, cd_off=None, zip64=None):
        """zip64: None, or the offset the zip64 locator gives for the zip64 end record ("true": where it is)."""
        cd = self.central()
        n, off = len(self.entries), len(self.body)
        tail = b""
        if zip64 is not None:
            where = off + len(cd) if zip64 == "true" else zip64
            tail = struct.pack("<IQHHIIQQQQ", 0x06064b50, 44, 45, 45, 0, 0, n, n, len(cd), off) + struct.pack("<IIQI", 0x07064b50, 0, where, 1)
            n, off = 0xffff, 0xffffffff
        n = n if n_ent is None else n_ent
        off = off if cd_off is None else cd_off
        return self.body + cd + tail + struct.pack("<IHHHHIIH", 0x06054b50, 0, 0, n & 0xffff, n & 0xffff, len(cd), off, 0)


def z64_extra(*vals):
    return struct.pack("<HH", 1, 8 * len(vals)) + b"".join(struct.pack("<Q", v) for v in vals)


NPZ_ARRAYS = {"final_norm": np.arange(8, dtype=np.float32), "lm_head_0": np.arange(40, dtype=np.float32).reshape(5, 8) / 7}
NPZ_WANT = {"cp.norm": entry(NPZ_ARRAYS["final_norm"]), "cp.lm_head.0": entry(NPZ_ARRAYS["lm_head_0"])}


def good_zip(deflate_second=False):
    return Zip({"final_norm.npy": (npy_bytes(NPZ_ARRAYS["final_norm"]), 0),
                "lm_head_0.npy": (npy_bytes(NPZ_ARRAYS["lm_head_0"]), 8 if deflate_second else 0)})


def test_the_hand_written_zip_is_a_zip(driver, tmp_path):
    """The archives the catalogue damages are sound before the damage: numpy reads them, and so does the reader."""
    for name, z in {"stored": good_zip().bytes(), "deflated": good_zip(True).bytes(), "zip64": good_zip(True).bytes(zip64="true")}.items():
        got = np.load(io.BytesIO(z))
        for k, a in NPZ_ARRAYS.items():
            assert np.array_equal(got[k], a)
        res = one(driver, tmp_path, "npz", z, name + ".npz")
        assert res is not None and res[0] == NPZ_WANT, name


# ---------------------------------------------------------------------------------------------------------------------
# a. the catalogue: every one must be refused

def _zip_case(edit=None, **kw):
    z = good_zip(kw.pop("deflate", False))
    if edit:
        edit(z.entries[-1])
    return z.bytes(**kw)


def _deflate_bomb(e):
    e.update(csize=40, usize=0xffffffff, extra=z64_extra(1 << 32))       # 4 GiB from the member's first 40 bytes


F4 = np.arange(16, dtype=np.float32).tobytes()                           # 64 payload bytes
CATALOGUE = {
    # .npy
    "npy_f8_count_wraps": ("npy", lambda: raw_npy(npy_header_text("<f8", "(%d,)" % (2 ** 62 + 2)), F4)),
    "npy_f4_2p63_by_2": ("npy", lambda: raw_npy(npy_header_text("<f4", "(%d, 2)" % 2 ** 63), F4)),
    "npy_f4_2p32_by_2p32": ("npy", lambda: raw_npy(npy_header_text("<f4", "(%d, %d)" % (2 ** 32, 2 ** 32)), F4)),
    "npy_header_ends_after_fortran_order": ("npy", lambda: raw_npy("{'descr': '<f4', 'fortran_order':")),
    "npy_fortran_order_without_value_last": ("npy", lambda: raw_npy("{'descr': '<f4', 'shape': (16,), 'fortran_order':", F4)),
    "npy_five_dimensions": ("npy", lambda: raw_npy(npy_header_text("<f4", "(1, 2, 2, 2, 2)"), F4)),
    "npy_30_digit_dimension": ("npy", lambda: raw_npy(npy_header_text("<f4", "(%s,)" % ("1" + "0" * 29)), F4)),
    "npy_30_digit_dimension_wrapping_to_16": ("npy", lambda: raw_npy(npy_header_text("<f4", "(%d,)" % (2 ** 96 + 16)), F4)),
    # .safetensors
    "st_two_million_brackets": ("safetensors", lambda: raw_st(b'{"__metadata__":' + b"[" * 2000000)),
    "st_shape_2p32_by_2p32": ("safetensors", lambda: raw_st({ST_KEY: {"dtype": "F32", "shape": [2 ** 32, 2 ** 32], "data_offsets": [0, 0]}})),
    "st_end_before_begin": ("safetensors", lambda: raw_st({ST_KEY: {"dtype": "F32", "shape": [4], "data_offsets": [32, 16]}}, F4)),
    "st_end_past_the_file": ("safetensors", lambda: raw_st({ST_KEY: {"dtype": "F32", "shape": [32], "data_offsets": [0, 128]}}, F4)),
    "st_header_length_2p64_minus_1": ("safetensors", lambda: struct.pack("<Q", 2 ** 64 - 1) + raw_st(
        {ST_KEY: {"dtype": "F32", "shape": [16], "data_offsets": [0, 64]}}, F4)[8:]),
    "st_offset_of_20_digits": ("safetensors", lambda: raw_st(
        ('{"%s":{"dtype":"F32","shape":[16],"data_offsets":[%d,%d]}}' % (ST_KEY, 2 ** 64, 2 ** 64 + 64)).encode(), F4)),
    "st_unclosed_array_closed_as_object": ("safetensors", lambda: raw_st(b'{"__metadata__":[}' + b" " * 64, F4)),
    # .npz
    "npz_extra_length_ffff": ("npz", lambda: _zip_case(lambda e: e.update(xlen=0xffff))),
    "npz_name_length_past_the_end": ("npz", lambda: _zip_case(lambda e: e.update(nlen=0xffff))),
    "npz_local_header_near_2p64": ("npz", lambda: _zip_case(lambda e: e.update(lho=0xffffffff, extra=z64_extra(2 ** 64 - 16)))),
    "npz_csize_near_2p64": ("npz", lambda: _zip_case(lambda e: e.update(csize=0xffffffff, extra=z64_extra(2 ** 64 - 8)))),
    "npz_zip64_locator_near_2p64": ("npz", lambda: _zip_case(zip64=2 ** 64 - 56)),
    "npz_zip64_locator_at_minus_8": ("npz", lambda: _zip_case(zip64=2 ** 64 - 8)),
    "npz_4gib_from_40_deflated_bytes": ("npz", lambda: _zip_case(_deflate_bomb, deflate=True)),
    "npz_central_directory_near_2p64": ("npz", lambda: _zip_case(cd_off=0xffffffff)),
    # Q3TTSW1
    "q3w_offset_2p64_minus_16": ("container", lambda: raw_container([("w", 0, 1, (8, 0, 0, 0), 2 ** 64 - 16, 32)], 512)),
    "q3w_numel_times_4_wraps_to_nbytes": ("container", lambda: raw_container([("w", 0, 1, (2 ** 62 + 2, 0, 0, 0), 256, 8)], 512)),
    "q3w_numel_wraps_to_nbytes": ("container", lambda: raw_container([("w", 0, 2, (2 ** 32, 2 ** 32, 0, 0), 256, 0)], 512)),
    "q3w_4294967295_tensors": ("container", lambda: raw_container([("w", 0, 1, (8, 0, 0, 0), 256, 32)], 512, n_tensors=2 ** 32 - 1)),
    "q3w_4294967295_meta": ("container", lambda: raw_container([("w", 0, 1, (8, 0, 0, 0), 256, 32)], 512, n_meta=2 ** 32 - 1)),
}


@pytest.mark.parametrize("name", sorted(CATALOGUE))
def test_catalogue_is_refused(driver, tmp_path, name):
    fmt, make = CATALOGUE[name]
    assert one(driver, tmp_path, fmt, make()) is None, "%s was accepted" % name


def test_catalogue_codec_table_through_open_auto(driver, tmp_path):
    """The (2**63, 2) table as the file the loaders would find it in: open_auto's trimming of the codec tables to 3072 rows
    must not meet it (nbytes 0 for 3072 x 2 floats).  Beside it, the trimming of a sound table."""
    bad, ok, head = tmp_path / "bad", tmp_path / "ok", tmp_path / "head"
    for d in (bad, ok, head):
        d.mkdir()
    (bad / "codec_embedding.npy").write_bytes(CATALOGUE["npy_f4_2p63_by_2"][1]())
    table = (np.arange(4000 * 2, dtype=np.float32) / 3).reshape(4000, 2)
    np.save(ok / "codec_embedding.npy", table)
    np.save(ok / "codec_head.npy", table.astype(np.float64))              # converted: the trimmed tensor lies in an owned buffer
    np.save(head / "codec_head.npy", table)
    r_bad, r_aux, r_ok = run_jobs(driver, tmp_path, ["auto %s" % bad, "auto %s %s" % (head, bad), "auto %s" % ok])     # (aux: --embeddings_dir)
    assert r_bad is None and r_aux is None
    assert r_ok is not None and r_ok[0] == {"talker.codec_embedding": entry(table[:3072]), "talker.codec_head": entry(table[:3072])}


# ---------------------------------------------------------------------------------------------------------------------
# b. legitimate unusual files stay accepted, with the right bytes

def test_unusual_npy_files_are_accepted(driver, tmp_path):
    a = (np.arange(24, dtype=np.float32) / 5).reshape(2, 3, 4)
    cases = {
        "v1": (npy_bytes(a, (1, 0)), entry(a)),
        "v2": (npy_bytes(a, (2, 0)), entry(a)),
        "v3": (npy_bytes(a, (3, 0)), entry(a)),
        "0d": (npy_bytes(np.float32(3.5)), (0, (), fnv1a(np.float32(3.5).tobytes()))),
        "0d_f8": (npy_bytes(np.float64(3.5)), (0, (), fnv1a(np.float32(3.5).tobytes()))),
        "zero_length": (npy_bytes(np.zeros((0, 8), np.float32)), (0, (0, 8), fnv1a(b""))),
        "zero_length_f8": (npy_bytes(np.zeros((3, 0), np.float64)), (0, (3, 0), fnv1a(b""))),
        "zero_length_beside_2p63": (raw_npy(npy_header_text("<i8", "(%d, 0)" % 2 ** 63)), (3, (2 ** 63, 0), fnv1a(b""))),
        "f8": (npy_bytes(a.astype(np.float64) / 3), entry((a.astype(np.float64) / 3).astype(np.float32))),
        "f2": (npy_bytes(a.astype(np.float16)), entry(a.astype(np.float16))),
        "i8": (npy_bytes(np.arange(-3, 4)), entry(np.arange(-3, 4))),
        "no_fortran_order_key": (raw_npy("{'descr': '<f4', 'shape': (16,)}", F4), (0, (16,), fnv1a(F4))),
        "largest_dimension_that_fits": (raw_npy(npy_header_text("<f4", "(0, %d)" % (2 ** 64 - 1))), (0, (0, 2 ** 64 - 1), fnv1a(b""))),
    }
    for k, (data, _) in cases.items():
        (tmp_path / k).write_bytes(data)
    res = run_jobs(driver, tmp_path, ["npy %s" % (tmp_path / k) for k in cases])
    for (k, (_, want)), r in zip(cases.items(), res):
        assert r is not None, "%s was refused" % k
        assert r[0] == {"t": want}, k


def test_unusual_npz_files_are_accepted(driver, tmp_path):
    cases = {}
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", zipfile.ZIP_STORED, allowZip64=True) as z:         # as numpy's savez writes a member
        for k, a in NPZ_ARRAYS.items():
            with z.open(k + ".npy", "w", force_zip64=True) as m:
                np.lib.format.write_array(m, a)
    cases["force_zip64"] = f.getvalue()
    f = io.BytesIO()
    np.savez(f, **NPZ_ARRAYS)
    cases["savez"] = f.getvalue()
    f = io.BytesIO()
    np.savez_compressed(f, **NPZ_ARRAYS)
    cases["savez_compressed"] = f.getvalue()
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", zipfile.ZIP_DEFLATED) as z:                        # a comment after the end record, other members
        z.comment = b"exported " * 30
        z.writestr("README.txt", "not an array")
        for k, a in NPZ_ARRAYS.items():
            z.writestr(k + ".npy", npy_bytes(a))
    cases["commented"] = f.getvalue()
    cases["zip64_central_directory"] = good_zip(True).bytes(zip64="true")
    z = good_zip()
    z.entries[0]["extra"] = struct.pack("<HHI", 0x5455, 4, 7) + z64_extra()         # extras that are not zip64's, an empty zip64 one
    z.entries[1].update(lho=0xffffffff, extra=z64_extra(z.entries[1]["lho"]))
    cases["zip64_local_header_offset"] = z.bytes()
    # 128 KiB of zeros: near deflate's best ratio (1032)
    big = {"final_norm": NPZ_ARRAYS["final_norm"], "lm_head_0": np.zeros((4096, 8), np.float32)}
    f = io.BytesIO()
    np.savez_compressed(f, **big)
    cases["deflate_at_its_best_ratio"] = f.getvalue()
    for k, data in cases.items():
        (tmp_path / (k + ".npz")).write_bytes(data)
    res = run_jobs(driver, tmp_path, ["npz %s" % (tmp_path / (k + ".npz")) for k in cases])
    for k, r in zip(cases, res):
        assert r is not None, "%s was refused" % k
        want = dict(NPZ_WANT, **{"cp.lm_head.0": entry(big["lm_head_0"])}) if k == "deflate_at_its_best_ratio" else NPZ_WANT
        assert r[0] == want, k


def test_unusual_safetensors_files_are_accepted(driver, tmp_path):
    from safetensors.numpy import save_file
    a = (np.arange(16, dtype=np.float32) / 9)
    b = np.arange(12, dtype=np.float16).reshape(3, 4)
    want = {"talker.norm": entry(a), "talker.codec_head": entry(b)}
    tens = {ST_KEY: {"dtype": "F32", "shape": [16], "data_offsets": [0, 64]},
            "talker.codec_head.weight": {"dtype": "F16", "shape": [3, 4], "data_offsets": [64, 88]}}
    payload = a.tobytes() + b.tobytes()
    cases = {}
    save_file({ST_KEY: a, "talker.codec_head.weight": b, "speaker_encoder.x": np.zeros(3, np.float32)},
              str(tmp_path / "lib.safetensors"), metadata={"format": "pt", "note": "a {nested} \"quoted\" \\ value ]"})
    cases["lib"] = (tmp_path / "lib.safetensors").read_bytes()
    cases["padded_with_spaces"] = raw_st(json.dumps(tens).encode() + b" " * 97, payload)
    cases["spaces_everywhere"] = raw_st(json.dumps(tens, indent=3).encode().replace(b":", b" :\t") + b"\n\n", payload)
    cases["nested_metadata"] = raw_st(dict({"__metadata__": {"a": {"b": [1, {"c": None, "d": [[], {}]}, -2.5e3], "e": {}}, "s": "x"}}, **tens), payload)
    cases["nested_metadata_last"] = raw_st(dict(tens, **{"__metadata__": {"a": [[[["deep"]]]], "t": True}}), payload)
    cases["metadata_30_deep"] = raw_st(('{"__metadata__":' + "[" * 30 + "]" * 30 + "," + json.dumps(tens)[1:]).encode(), payload)
    cases["escaped_quotes"] = raw_st(dict({"__metadata__": {"q": "say \"{\" and \\\" ]", "\"k\"": "\\"}}, **tens), payload)
    cases["unknown_tensor_keys"] = raw_st({k: dict(v, extra={"x": [1, 2]}, flag=False) for k, v in tens.items()}, payload)
    cases["zero_length"] = raw_st(dict(tens, **{"talker.model.codec_embedding.weight": {"dtype": "BF16", "shape": [0, 8], "data_offsets": [88, 88]}}), payload)
    for k, data in cases.items():
        (tmp_path / (k + ".st")).write_bytes(data)
    res = run_jobs(driver, tmp_path, ["safetensors %s" % (tmp_path / (k + ".st")) for k in cases])
    for k, r in zip(cases, res):
        assert r is not None, "%s was refused" % k
        w = dict(want, **{"talker.codec_embedding": (4, (0, 8), fnv1a(b""))}) if k == "zero_length" else want
        assert r[0] == w, k


def test_containers_are_accepted(driver, tmp_path):
    t = {"a": np.arange(6, dtype=np.float32).reshape(2, 3), "b": np.arange(5, dtype=np.int64), "c": np.zeros((0, 4), np.float16),
         "d": np.array(7, np.int32)}
    W.write_pack(str(tmp_path / "w.q3w"), {"hidden": 8.0, "rms_eps": 1e-6}, t)
    # a tensor that ends with the file, one at the last byte's offset with nothing in it
    edge = raw_container([("w", 0, 1, (8, 0, 0, 0), 512 - 32, 32), ("z", 1, 2, (0, 9, 0, 0), 512, 0)], 512, meta=[("k", 2.5)])
    (tmp_path / "edge.q3w").write_bytes(edge)
    r, e = run_jobs(driver, tmp_path, ["container %s" % (tmp_path / "w.q3w"), "container %s" % (tmp_path / "edge.q3w")])
    assert r is not None and r[0] == {k: entry(a) for k, a in t.items()} and r[1] == {"hidden": 8.0, "rms_eps": 1e-6}
    assert e is not None and e[0] == {"w": (0, (8,), fnv1a(edge[-32:])), "z": (1, (0, 9), fnv1a(b""))} and e[1] == {"k": 2.5}


# ---------------------------------------------------------------------------------------------------------------------
# c. / d. one small valid file per format: every prefix, and seeded mutants of its structural bytes

def small_files(tmp_path):
    """-> fmt: (bytes, offsets of the structural bytes, (begin, end) of the text header or None, bytes a prefix needs)."""
    rng = np.random.default_rng(5)
    out = {}
    a = rng.standard_normal((30, 10)).astype(np.float32)
    b = npy_bytes(a)
    hdr = len(b) - a.nbytes
    out["npy"] = (b, list(range(hdr)), (10, hdr), len(b))
    # .npz: a stored and a deflated member (zipfile's own writer)
    f = io.BytesIO()
    arrays = {"final_norm": rng.standard_normal(64).astype(np.float32), "layer_0_q_proj": rng.standard_normal((12, 8)).astype(np.float32),
              "lm_head_0": (rng.integers(0, 4, (40, 8)) / 4).astype(np.float32)}
    with zipfile.ZipFile(f, "w") as z:
        with z.open("final_norm.npy", "w", force_zip64=True) as m:
            np.lib.format.write_array(m, arrays["final_norm"])
        z.writestr("layer_0_q_proj.npy", npy_bytes(arrays["layer_0_q_proj"]))
        z.writestr("lm_head_0.npy", npy_bytes(arrays["lm_head_0"]))
        z.writestr("codec_emb_0.npy", npy_bytes(arrays["lm_head_0"]), compress_type=zipfile.ZIP_DEFLATED)
    b = f.getvalue()
    with zipfile.ZipFile(io.BytesIO(b)) as z:
        infos, cd = z.infolist(), z.start_dir
    struct_off = list(range(cd, len(b)))
    for zi in infos:
        nlen, xlen = struct.unpack_from("<HH", b, zi.header_offset + 26)
        data = zi.header_offset + 30 + nlen + xlen
        struct_off += list(range(zi.header_offset, data))
        if zi.compress_type == 0:       # the member's own .npy header
            struct_off += list(range(data, data + 10 + struct.unpack_from("<H", b, data + 8)[0]))
    out["npz"] = (b, sorted(struct_off), None, len(b))
    # .safetensors
    from safetensors.numpy import save_file
    p = str(tmp_path / "small.safetensors")
    save_file({ST_KEY: rng.standard_normal(64).astype(np.float32), "talker.codec_head.weight": rng.standard_normal((20, 8)).astype(np.float16),
               "talker.model.layers.0.self_attn.q_proj.weight": rng.standard_normal((12, 8)).astype(np.float32),
               "speaker_encoder.x": np.zeros(5, np.float32)}, p, metadata={"format": "pt", "note": "a \"quoted\" value"})
    b = open(p, "rb").read()
    hlen = struct.unpack_from("<Q", b)[0]
    out["safetensors"] = (b, list(range(8 + hlen)), (8, 8 + hlen), len(b))
    # Q3TTSW1
    p = str(tmp_path / "small.q3w")
    t = {"talker.norm": rng.standard_normal(64).astype(np.float32), "cp.lm_head.0": rng.standard_normal((20, 8)).astype(np.float16),
         "ids": np.arange(33, dtype=np.int64)}
    W.write_pack(p, {"hidden": 8.0, "cp_groups": 1.0}, t)
    b = open(p, "rb").read()
    tables = 32 + 2 * 56 + 3 * 152
    need = max(sum(struct.unpack_from("<QQ", b, 32 + 2 * 56 + i * 152 + 136)) for i in range(3))      # offset + nbytes
    out["container"] = (b, list(range(tables)), None, need)
    for fmt, (b, _, _, _) in out.items():
        assert 1000 <= len(b) <= 3200, (fmt, len(b))
    return out


FORMATS = ["npy", "npz", "safetensors", "container"]


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_prefix(driver, tmp_path, fmt):
    data, _, _, need = small_files(tmp_path)[fmt]
    path = tmp_path / ("whole." + fmt)
    path.write_bytes(data)
    res = run_jobs(driver, tmp_path, ["%s %s heap" % (fmt, path)] + ["%s %s trunc %d" % (fmt, path, n) for n in range(len(data))])
    whole, prefixes = res[0], res[1:]
    assert whole is not None and len(whole[0]) >= 1
    assert len(prefixes) == len(data)
    for n, r in enumerate(prefixes):
        if n < need:
            assert r is None, "the first %d of %d bytes were accepted: they cut into a tensor's data" % (n, len(data))
        else:               # (only padding is missing)
            assert r is None or r == whole, n
    print("%s: %d prefixes, %d refused" % (fmt, len(prefixes), sum(r is None for r in prefixes)))


def mutants(data, structural, text, r, count):
    size = len(data)
    for _ in range(count):
        if text and r.random() < 0.25:      # the text headers: a span deleted or doubled
            a = r.randrange(text[0], text[1])
            n = r.randint(1, min(24, text[1] - a))
            yield data[:a] + data[a + n:] if r.random() < 0.5 else data[:a + n] + data[a:a + n] + data[a + n:]
            continue
        w = r.choice([1, 2, 4, 8])
        off = min(r.choice(structural), size - w)
        v = r.choice([0, 1, (1 << (8 * w - 1)) - 1, (1 << (8 * w)) - 1, size, size + 1, size - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 63,
                      r.getrandbits(8 * w)]) & ((1 << (8 * w)) - 1)
        yield data[:off] + v.to_bytes(w, "little") + data[off + w:]


def test_seeded_mutants(driver, tmp_path):
    files = small_files(tmp_path)
    for k, fmt in enumerate(FORMATS):
        data, structural, text, _ = files[fmt]
        d = tmp_path / ("mut_" + fmt)
        d.mkdir()
        jobs = []
        for i, m in enumerate(mutants(data, structural, text, random.Random(20240 + k), N_MUTANTS)):
            (d / ("%04d" % i)).write_bytes(m)
            jobs.append("%s %s heap" % (fmt, d / ("%04d" % i)))
        res = run_jobs(driver, tmp_path, jobs)
        refused = sum(r is None for r in res)
        print("%s: %d mutants, %d refused, %d accepted and consistent" % (fmt, len(res), refused, len(res) - refused))
        assert len(res) == N_MUTANTS and 0 < refused < N_MUTANTS, (fmt, refused)


# ---------------------------------------------------------------------------------------------------------------------
# e. the host fp16 conversions every F32 / BF16 weight goes through at load

def test_h2f_and_f2h_sat_against_the_compiler(driver):
    out = subprocess.run([driver, "fp16"], capture_output=True, text=True, timeout=120, env=driver_env())
    assert out.returncode == 0, out.stdout + out.stderr
    counts = dict(line.rsplit(" ", 1) for line in out.stdout.splitlines())
    assert counts == {"h2f patterns": "65536", "f2h_sat halves": str(3 * 63488), "f2h_sat midpoints": str(3 * 2 * 0x7bff),
                      "f2h_sat bf16": "65536", "f2h_sat edges": "51", "mismatches": "0"}
