#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of the library without a GPU.

    python scripts/kernel_code_diff.py OLD.so NEW.so [--gone REGEX] [--may-differ REGEX] > report.md

For every kernel symbol of the code objects bundled in the two shared libraries: the resource notes (VGPRs, AGPRs, SGPRs,
spills, scratch, static LDS) and the `llvm-objdump -d` text with the address / encoding column and pc-relative literal
operands removed.  Kernels matching --gone may be missing from NEW; kernels matching --may-differ may differ in code as
long as no resource grew.  Prints a markdown report; exit status 1 when anything else differs.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qwen3_tts_axera_russian_amd.build import code_objects, kernel_notes  # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
             "private_segment_fixed_size", "group_segment_fixed_size")


def disassembly(elf: bytes):
    """-> {symbol: [instruction text]} of one code object's .text"""
    with tempfile.NamedTemporaryFile(suffix=".elf") as f:
        f.write(elf)
        f.flush()
        text = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
    out, cur, pcrel = {}, None, 0
    for line in text.split("\n"):
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = line.split("//")[0].strip()   # the comment holds the address, the encoding and a branch's resolved target
        # s_getpc_b64 followed by s_add_u32 / s_addc_u32 with a literal: the distance to another symbol of the code object
        if ins.startswith("s_getpc_b64"):
            pcrel = 4
        elif pcrel:
            pcrel -= 1
            if re.match(r"s_addc?_u32 ", ins):
                ins = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <pcrel>", ins)
        cur.append(ins)
    for body in out.values():   # alignment padding behind the last instruction
        while body and body[-1] in ("s_nop 0", "s_code_end", "..."):
            body.pop()
    return out


def kernels_of(lib):
    """-> {kernel symbol: (resources dict, [instruction text])}"""
    res = {}
    for elf in code_objects(lib):
        dis = disassembly(elf)
        for name, kv in kernel_notes(elf).items():
            res[name] = ({k: int(kv.get(k, 0)) for k in RESOURCES}, dis.get(name, []))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--gone", default=None, help="kernels that may be missing from NEW")
    ap.add_argument("--may-differ", default=None, help="kernels whose code may differ while no resource grows")
    a = ap.parse_args()
    old, new = kernels_of(a.old), kernels_of(a.new)
    gone = sorted(k for k in old if k not in new)
    added = sorted(k for k in new if k not in old)
    bad_gone = [k for k in gone if not (a.gone and re.search(a.gone, k))]
    same, res_diff, code_diff = 0, [], []
    for k in sorted(set(old) & set(new)):
        (ro, co), (rn, cn) = old[k], new[k]
        if ro == rn and co == cn:
            same += 1
            continue
        differ_ok = bool(a.may_differ and re.search(a.may_differ, k)) and all(rn[x] <= ro[x] for x in RESOURCES)
        if ro != rn:
            res_diff.append((k, ro, rn, differ_ok))
        if co != cn:
            code_diff.append((k, co, cn, differ_ok))
    failed = bool(bad_gone or added or [x for x in res_diff + code_diff if not x[3]])
    print(f"# Kernel code: `{os.path.basename(a.old)}` (old) against `{os.path.basename(a.new)}` (new)\n")
    print(f"* kernels: {len(old)} old, {len(new)} new; {same} with identical resources and identical code")
    print(f"* missing from new: {len(gone)} ({len(bad_gone)} not allowed to be); only in new: {len(added)}")
    print(f"* differing resources: {len(res_diff)}; differing code: {len(code_diff)}")
    allowed = len({x[0] for x in res_diff + code_diff if x[3]})
    print(f"* verdict: {'FAIL' if failed else 'PASS'}{f' ({allowed} kernels differ as allowed, listed below)' if allowed and not failed else ''}\n")
    for title, names in (("Missing from new", gone), ("Only in new", added)):
        if names:
            print(f"## {title}\n")
            for k in names:
                print(f"* `{k}`")
            print()
    if res_diff:
        print("## Differing resources\n")
        for k, ro, rn, ok in res_diff:
            ch = ", ".join(f"{x} {ro[x]} -> {rn[x]}" for x in RESOURCES if ro[x] != rn[x])
            print(f"* `{k}`: {ch}{' (allowed: none grew)' if ok else ''}")
        print()
    if code_diff:
        print("## Differing code\n")
        for k, co, cn, ok in code_diff:
            print(f"### `{k}` ({len(co)} -> {len(cn)} instructions{', allowed' if ok else ''})\n\n```diff")
            print("\n".join(list(difflib.unified_diff(co, cn, "old", "new", lineterm="", n=2))[:200]))
            print("```\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
