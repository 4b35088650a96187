"""The descriptors the ViLT path added or extended (mart_vilt_embed_desc, the rw_row_lo tails of mart_attn_fwd_desc / mart_attn_f32_desc)
against gcc's layout of include/mart_hip.h and the header's field order, on a GPU-less box."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mkg_analogy_amd import _lib
    return _lib


def _header_fields(cname):
    txt = open(os.path.join(ROOT, "include", "mart_hip.h")).read()
    end = txt.index("} " + cname + ";")
    body = re.sub(r"/\*.*?\*/", "", txt[txt.rindex("typedef struct {", 0, end) + len("typedef struct {"):end], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = re.sub(r"^(const\s+)?(unsigned\s+)?(long long|[a-z0-9_]+_t|[a-z]+)\s*\**", "", decl)
            fields += [n.strip().lstrip("*").strip() for n in names.split(",")]
    return fields


def test_vilt_descriptor_field_order(lib):
    for cname, cls in (("mart_vilt_embed_desc", lib.ViltEmbed), ("mart_attn_fwd_desc", lib.AttnFwd), ("mart_attn_f32_desc", lib.AttnF32)):
        assert _header_fields(cname) == [f[0] for f in cls._fields_], cname


def test_vilt_descriptor_layout_matches_gcc(lib, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    pairs = [("mart_vilt_embed_desc", lib.ViltEmbed), ("mart_attn_fwd_desc", lib.AttnFwd), ("mart_attn_f32_desc", lib.AttnF32),
             ("mart_attn_bwd_desc", lib.AttnBwd)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mart_hip.h"', 'int main(void) {']
    for cname, cls in pairs:
        for f in cls._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
    lines += ['  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    out = subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = {(l.split()[0], l.split()[1]): int(l.split()[2]) for l in out if l.strip()}
    for cname, cls in pairs:
        for f in cls._fields_:
            assert seen[(cname, f[0])] == getattr(cls, f[0]).offset, (cname, f[0])
        assert seen[(cname, "sizeof")] == ctypes.sizeof(cls), cname
