"""mart_topk among the library's exports and in the ctypes table, against the declaration in include/mart_hip.h, on a GPU-less box (the ABI version
stays 10: a pure addition), and the host-side refusals of Fn.topk, which run before anything is launched."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mkg_analogy_amd import _lib
    return _lib


def test_topk_entry_point_exported(lib):
    so = ctypes.CDLL(lib.LIB_PATH)                      # plain dlopen: no GPU needed
    hdr = open(os.path.join(ROOT, "include", "mart_hip.h")).read()
    assert "mart_topk" in lib.EXPORTS and hasattr(so, "mart_topk")
    decl = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int mart_topk(const float* logits, int ld, int R, int C, int k, float* values , int32_t* indices , void* stream);" in decl
    res, args = lib._SIGS["mart_topk"]
    assert res is lib.i32 and args == [lib.vp, lib.i32, lib.i32, lib.i32, lib.i32, lib.vp, lib.vp, lib.vp]
    so.mart_abi_version.restype = ctypes.c_int
    assert so.mart_abi_version() == lib.EXPECTED_ABI == 10
    assert len(lib.EXPORTS) == 71 and len(re.findall(r"^(?:int|long long|const char\*)\s+mart_\w+\(", hdr, flags=re.M)) == 71


def test_topk_refuses_bad_arguments_without_a_launch(lib):
    """The C entry point checks its arguments before the launch: with null streams and host pointers nothing may be dereferenced."""
    so = ctypes.CDLL(lib.LIB_PATH)
    so.mart_topk.restype, so.mart_topk.argtypes = lib._SIGS["mart_topk"]
    so.mart_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for ld, R, C, k in ((8, 2, 8, 0), (8, 2, 8, 65), (8, 2, 8, 9), (7, 2, 8, 4), (8, 0, 8, 4), (100, 1, 100, 65)):
        assert so.mart_topk(p, ld, R, C, k, p, p, None) != 0
        assert b"topk" in so.mart_last_error()
    assert so.mart_topk(None, 8, 2, 8, 4, p, p, None) != 0


def test_functional_topk_refuses_on_the_host(lib):
    from mkg_analogy_amd import functional as Fn
    x = torch.zeros(3, 100)                              # a CPU tensor: every refusal below comes before the device is looked at
    for k in (65, 101, 0, -1):
        with pytest.raises(ValueError, match="topk"):
            Fn.topk(x, k)
    with pytest.raises(ValueError, match="topk"):
        Fn.topk(torch.zeros(3, 20), 21)                  # k > C below the 64 limit
    for bad in (torch.zeros(100), torch.zeros(2, 3, 100)):
        with pytest.raises(ValueError, match="2-D"):
            Fn.topk(bad, 5)
    with pytest.raises(ValueError, match="float32"):
        Fn.topk(torch.zeros(3, 100, dtype=torch.float64), 5)
    with pytest.raises(ValueError, match="HIP device"):
        Fn.topk(x, 5)                                    # valid arguments, but no CPU path: an error, never a fallback
