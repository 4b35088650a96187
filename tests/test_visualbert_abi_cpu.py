"""The descriptor the VisualBERT path added (mart_vbert_embed_desc) against gcc's layout of include/mart_hip.h and the header's field order, and
its two entry points among the library's exports, on a GPU-less box.  The ABI version stays 10: nothing existing changed."""
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


def test_vbert_descriptor_field_order(lib):
    assert _header_fields("mart_vbert_embed_desc") == [f[0] for f in lib.VbertEmbed._fields_]


def test_vbert_descriptor_layout_matches_gcc(lib, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cname, cls = "mart_vbert_embed_desc", lib.VbertEmbed
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mart_hip.h"', 'int main(void) {']
    for f in cls._fields_:
        lines.append(f'  printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += [f'  printf("sizeof %zu\\n", sizeof({cname}));', '  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    out = subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    for f in cls._fields_:
        assert seen[f[0]] == getattr(cls, f[0]).offset, f[0]
    assert seen["sizeof"] == ctypes.sizeof(cls)


def test_vbert_entry_points_exported(lib):
    so = ctypes.CDLL(lib.LIB_PATH)                      # plain dlopen: no GPU needed
    hdr = open(os.path.join(ROOT, "include", "mart_hip.h")).read()
    for name in ("mart_vbert_embed_fwd", "mart_vbert_embed_bwd"):
        assert name in lib.EXPORTS and hasattr(so, name)
        assert re.search(r"int\s+" + name + r"\(const mart_vbert_embed_desc\* d, void\* stream\);", hdr)
    so.mart_abi_version.restype = ctypes.c_int
    assert so.mart_abi_version() == lib.EXPECTED_ABI == 10
