"""Compare the gfx950 assembly of csrc/attention.hip and csrc/precise.hip between a git revision and the working tree, kernel by kernel.

    python tools/disasm_diff.py [--rev HEAD]

Both sides are compiled with the package flags and --save-temps; each kernel's instruction stream is compared with branch labels
normalised.  A kernel whose template gained a defaulted flag (e.g. attn_fwd_k<.., LO = false>) is matched to its old name.  The second
verdict ignores the immediate offsets of kernel-argument loads (s_load* ..., 0x..): a descriptor that grows at its tail moves the hidden
arguments behind it, and the fields of a descriptor that embeds it, without changing any instruction.
"""
from __future__ import annotations

import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mkg_analogy_amd import _build  # noqa: E402

FILES = ("attention.hip", "precise.hip")


def compile_s(src_root: str, inc_root: str, name: str, out: str) -> str:
    cmd = [_build.HIPCC] + [f for f in _build.FLAGS if not f.startswith("-I")] + ["-I" + inc_root, "-I" + src_root] + \
        _build.EXTRA.get(name, []) + ["--offload-device-only", "--save-temps", "-c", os.path.join(src_root, name), "-o", name + ".co"]
    subprocess.run(cmd, cwd=out, check=True, capture_output=True)
    return os.path.join(out, name.replace(".hip", "") + "-hip-amdgcn-amd-amdhsa-gfx950.s")


def kernels(path: str):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur = m.group(1); out[cur] = []; continue
        if line.startswith(".Lfunc_end"):
            cur = None; continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if s and (not s.startswith(".") or s.startswith(".LBB")):
            out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def strip_kernarg(body):
    return [re.sub(r"^(s_load_\w+ \S+, s\[\d+:\d+\]), 0x[0-9a-f]+$", r"\1, OFF", x) for x in body]


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--rev", default="HEAD")
    a = a.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        for sub in ("csrc", "include", "o_old", "o_new"):
            os.makedirs(os.path.join(old if sub in ("csrc", "include") else tmp, sub), exist_ok=True)
        for rel in [f"mkg_analogy_amd/csrc/{f}" for f in FILES] + ["mkg_analogy_amd/csrc/common.h", "include/mart_hip.h"]:
            dst = os.path.join(old, "include" if rel.startswith("include") else "csrc", os.path.basename(rel))
            with open(dst, "w") as f:
                f.write(subprocess.run(["git", "show", f"{a.rev}:{rel}"], cwd=ROOT, check=True, capture_output=True, text=True).stdout)
        ok = True
        for name in FILES:
            ka = kernels(compile_s(os.path.join(old, "csrc"), os.path.join(old, "include"), name, os.path.join(tmp, "o_old")))
            kb = kernels(compile_s(_build.CSRC, os.path.join(ROOT, "include"), name, os.path.join(tmp, "o_new")))
            alias = {}
            for m in kb:
                alias.setdefault(m, m)
                alias.setdefault(re.sub(r"ELb0EEEv", "EEEv", m, count=1), m)
                alias.setdefault(re.sub(r"ILb([01])ELb0EEEv", r"ILb\1EEEv", m, count=1), m)
                alias.setdefault(re.sub(r"ILb0EEEv", "E", m, count=1), m)          # a plain kernel that became template <bool LO = false>
            used = set()
            for n in sorted(ka):
                m = alias.get(n)
                if m is None:
                    print(f"{name}: MISSING {n}"); ok = False; continue
                used.add(m)
                same, same_k = ka[n] == kb[m], strip_kernarg(ka[n]) == strip_kernarg(kb[m])
                ok &= same_k
                nd = sum(1 for x in difflib.unified_diff(ka[n], kb[m], lineterm="", n=0) if x[:1] in "+-" and x[:3] not in ("+++", "---"))
                print(f"{name}: {'identical' if same else ('kernarg offsets only (' + str(nd) + ' lines)' if same_k else 'DIFFERENT')}  {n}")
            for m in sorted(set(kb) - used):
                print(f"{name}: new  {m}")
        print("verdict:", "existing kernels unchanged beyond kernel-argument offsets" if ok else "CHANGED")


if __name__ == "__main__":
    main()
