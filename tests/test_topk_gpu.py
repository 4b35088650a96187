"""mart_topk / Fn.topk: the k best columns of every row in the order of ``torch.sort(row, descending=True, stable=True)`` -- values descend,
equal values in ascending index order, NaN before +inf, -0.0 == +0.0 (include/mart_hip.h).  Every case is compared with that sort of the
IDENTICAL fp32 input on the host: indices exactly, values bit for bit (NaNs by position)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1, 1, 1), (3, 17, 17, 5), (3, 17, 17, 17), (6, 37, 40, 10), (2, 192, 192, 64), (5, 257, 259, 20), (4, 2063, 2063, 10),
          (257, 2063, 2064, 1), (3, 11292, 11292, 20), (2, 42007, 42008, 64)]
CONTENT_SHAPES = [(2063, 10), (257, 64)]


def _strided(x, ld):
    """x [R, C] on the device as rows of a buffer with leading dimension ld (shifted by one float: row starts not aligned to 16 bytes when ld is odd)."""
    R, C = x.shape
    buf = torch.full((R * ld + 1,), float("nan"), dtype=torch.float32, device="cuda")      # NaN around the rows: reading past a row would show
    view = buf[1:].view(R, ld)[:, :C] if ld > C else buf[:R * C].view(R, C)
    view.copy_(x)
    return view


def _check(x_host, k, ld=None, what=""):
    from mkg_analogy_amd import functional as Fn
    R, C = x_host.shape
    sv, si = torch.sort(x_host, dim=1, descending=True, stable=True)
    sv, si = sv[:, :k].contiguous(), si[:, :k].contiguous()
    xd = _strided(x_host.cuda(), C if ld is None else ld)
    assert xd.stride(0) == (C if ld is None else ld) or R == 1
    v, i = Fn.topk(xd, k)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and tuple(v.shape) == (R, k) and tuple(i.shape) == (R, k)
    v, i = v.cpu(), i.cpu()
    assert torch.equal(i, si), (what, i[(i != si).any(1)][:2], si[(i != si).any(1)][:2])
    nan = torch.isnan(sv)
    assert torch.equal(torch.isnan(v), nan), what
    assert torch.equal(v.view(torch.int32)[~nan], sv.view(torch.int32)[~nan]), what          # bitwise: -0.0 stays -0.0
    return v, i


@pytest.mark.parametrize("R,C,ld,k", SHAPES)
def test_shapes_seeded_normal(R, C, ld, k):
    g = torch.Generator().manual_seed(1000 + C + k)
    _check(torch.randn(R, C, generator=g), k, ld)


def _contents(C, k):
    g = torch.Generator().manual_seed(7 * C + k)
    base = torch.randn(C, generator=g)
    out = {"normal": base.clone(), "all_equal": torch.full((C,), 0.25)}
    out["eight_values"] = torch.randint(0, 8, (C,), generator=g).float() - 3.5              # a row quantised to 8 distinct values
    spread = [5, min(300, C - 7), min(301, C - 6), min(777, C - 3), C - 1]
    # a tie class of 5 members spread over the row; `above` strictly larger values in front of it in the order
    for name, above in (("tie_contains_kth", k - 3), ("tie_ends_at_kth", k - 5)):
        x = base.clamp(-3, 3).clone()
        x[spread] = 50.0
        free = [c for c in torch.randperm(C, generator=g).tolist() if c not in spread][:above]
        x[free] = 60.0 + torch.arange(above, dtype=torch.float32)
        out[name] = x
    z = base.clone().clamp(max=-0.5)
    z[::3], z[1::3] = 0.0, -0.0                                                               # the zeros are the largest values: interleaved signs
    out["signed_zeros"] = z
    inf = base.clone()
    inf[[3, C // 2, C - 2]] = float("inf")
    inf[[0, 9, C - 1]] = float("-inf")
    out["infinities"] = inf
    out["mostly_neg_inf"] = torch.full((C,), float("-inf"))
    out["mostly_neg_inf"][[4, C - 5]] = torch.tensor([1.0, 2.0])
    nan = base.clone()
    nan[[7, C - 3]] = float("nan")
    nan[11] = float("inf")
    out["two_nans"] = nan
    den = torch.zeros(C)
    n = min(C, 200)
    den[:n] = torch.arange(1, n + 1, dtype=torch.int32).view(torch.float32)[torch.randperm(n, generator=g)]     # the smallest positive denormals
    den[n:] = -(torch.arange(1, C - n + 1, dtype=torch.int32).view(torch.float32))          # ... and negative ones
    out["denormals"] = den
    run = base.clone().clamp(max=1.0)
    bits = torch.tensor(1.5).view(torch.int32) + torch.arange(100, dtype=torch.int32)          # 100 consecutive representable floats above 1.5
    pos = torch.randperm(C, generator=g)[:100]
    run[pos] = bits.view(torch.float32)
    out["consecutive_floats"] = run
    negrun = base.clone().clamp(max=-9.0)
    negrun[pos] = (torch.tensor(-1.5).view(torch.int32) + torch.arange(100, dtype=torch.int32)).view(torch.float32)
    out["consecutive_negative_floats"] = negrun
    return out


@pytest.mark.parametrize("C,k", CONTENT_SHAPES)
def test_contents(C, k):
    cases = _contents(C, k)
    assert len(torch.unique(cases["eight_values"])) == 8
    x = torch.stack(list(cases.values()))                   # one launch: every content is a row
    v, i = _check(x, k, C + 1, what=list(cases))
    names = list(cases)
    assert i[names.index("all_equal")].tolist() == list(range(k))
    spread = [5, min(300, C - 7), min(301, C - 6), min(777, C - 3), C - 1]
    assert i[names.index("tie_contains_kth")].tolist()[-3:] == spread[:3]                    # the class straddles place k: its lowest indices
    assert i[names.index("tie_ends_at_kth")].tolist()[-5:] == spread                          # the class ends exactly at place k
    assert torch.isnan(v[names.index("two_nans")][:2]).all() and i[names.index("two_nans")][:3].tolist() == [7, C - 3, 11]
    zr = i[names.index("signed_zeros")]
    assert zr.tolist() == [c for c in range(C) if c % 3 != 2][:k]                              # +0.0 and -0.0 are one tie class


def test_golden_tie_row():
    g = np.load(os.path.join(GOLD, "g3_loss_rank.npz"))
    x = torch.from_numpy(g["tie_logits"]).float()
    assert x.tolist() == [[1.0, 3.0, 3.0, 2.0]] and g["tie_ranks_all"].tolist() == [[4, 1, 2, 3]]
    v, i = _check(x, 4)
    assert i.tolist() == [[1, 2, 3, 0]]
    # the reference's double sort gives column c the rank tie_ranks_all[c]: the list is its inverse
    assert [g["tie_ranks_all"][0][c] for c in i[0].tolist()] == [1, 2, 3, 4]


def test_two_launches_bitwise_equal():
    from mkg_analogy_amd import functional as Fn
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(0, 50, (64, 11292), generator=g).float() / 7).cuda()               # many ties: the order cannot come from arrival order
    a, b = Fn.topk(x, 64), Fn.topk(x, 64)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_column_slice_of_a_wider_tensor():
    from mkg_analogy_amd import functional as Fn
    g = torch.Generator().manual_seed(4)
    wide = torch.randn(9, 3000, generator=g).cuda()
    part = wide[:, 131:131 + 2063]                              # row stride 3000, first element 524 bytes into the row
    assert not part.is_contiguous()
    ptr = part.data_ptr()
    v, i = Fn.topk(part, 10)
    vc, ic = Fn.topk(part.contiguous(), 10)
    assert part.data_ptr() == ptr and torch.equal(i, ic) and torch.equal(v.view(torch.int32), vc.view(torch.int32))
    _check(wide.cpu()[:, 131:131 + 2063].contiguous(), 10)


def test_label_position_equals_rank():
    from mkg_analogy_amd import functional as Fn
    g = torch.Generator().manual_seed(5)
    x = torch.stack([torch.randperm(2063, generator=g).float() / 64 - 16 for _ in range(32)])     # tie-free by construction, seeded
    assert all(len(torch.unique(r)) == 2063 for r in x)
    xd = x.cuda()
    v, i = Fn.topk(xd, 64)
    label = i[torch.arange(32), torch.arange(32) * 2]           # an entity at a known place of every list
    ranks = Fn.entity_ranks(xd, label)
    pos = (i == label[:, None]).int().argmax(1)
    assert torch.equal(pos, ranks - 1) and pos.tolist() == [2 * r for r in range(32)]


def test_refusals_launch_nothing():
    from mkg_analogy_amd import _lib as L, ops
    x = torch.randn(4, 100, device="cuda")
    v = torch.full((4, 64), -7.0, device="cuda")
    i = torch.full((4, 64), -7, device="cuda", dtype=torch.int32)
    call = lambda ld, C, k: L.lib().mart_topk(x.data_ptr(), ld, 4, C, k, v.data_ptr(), i.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for ld, C, k in ((100, 100, 0), (100, 100, 65), (100, 50, 51), (99, 100, 10), (100, 100, -1)):
        assert call(ld, C, k) != 0
        assert b"topk" in L.lib().mart_last_error()
        with pytest.raises(L.MartError, match="topk"):
            L.check(call(ld, C, k), "mart_topk")
    with pytest.raises(L.MartError):
        ops.topk(x, 0, v, i)
    torch.cuda.synchronize()
    assert bool((v == -7.0).all()) and bool((i == -7).all())     # nothing was written
    from mkg_analogy_amd import functional as Fn
    for k in (0, 65, 101):
        with pytest.raises(ValueError):
            Fn.topk(x, k)
