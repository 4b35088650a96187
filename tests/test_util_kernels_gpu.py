"""The memory-bound helpers of the bf16 training step (csrc/util.hip), each entry point on its own through mkg_analogy_amd.ops: the vector body,
the scalar tail (n % 4 != 0), the stride loop behind the 8192-block grid cap, duplicate-row semantics.  Casts, adds, gathers and the dropout
backward are compared bit for bit with the same torch expression on the CPU; mart_act_bwd and mart_scatter_add_rows_f32 against float64 with a
derived bound (see the tests).  The whole-model gates (bf16, a few percent) cannot see one wrong tail element; these can.

Measured on an MI355X: every bit-exact claim below holds; act_bwd worst case 1.00 bf16 ulp (gelu, quick-gelu), 0 (none, stored);
scatter_add_rows_f32 worst case 0.07 of its bound."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mkg_analogy_amd import ops as o
    o.require_gpu()
    return o


DEV = "cuda"
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
BIG = 8192 * 256 * 4 + 7                                   # past the 8192-block cap of the 4-elements-per-thread kernels: the stride loop runs, then a 3-element tail
NS = [1, 2, 3, 4, 5, 1023, 4099, BIG]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(got, ref, what):
    """bit-equal (so -0 != +0), NaNs compared by position"""
    got, ref = got.cpu(), ref.cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan), f"{what}: NaN positions differ"
    bad = (_bits(got) != _bits(ref)) & ~nan
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements differ, first at {int(bad.nonzero()[0])}"


def _specials():
    ties = torch.tensor([0x3F808000, 0x3F818000, 0x3F801000, 0x3F803000, 0x33000000], dtype=torch.int32).view(F32)   # bf16 ties (to even: down, up), fp16 ties, 2^-25 (fp16 tie to 0)
    vals = torch.tensor([0.0, -0.0, 1e-6, -3e-6, 2.5e-5, -6e-5, 5.9604645e-08, 6.1e-5, 65504.0, 65520.0, -65520.0, 65519.0, 1e5, -1e5,
                         float("nan"), float("inf"), float("-inf"), 3.39e38, -1e-30])
    return torch.cat([ties, -ties, vals])


def _values(n, seed):
    """n f32 values: random, with the special values at the front and again at the very end (the scalar tail), rotated by n so that the short sizes see different ones"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 4
    sp = _specials().roll(n)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n >= 2 * sp.numel():
        x[-sp.numel():] = sp
    return x


def _guarded(n, dtype, fill):
    """an n-element output with 8 guard elements behind it"""
    full = torch.full((n + 8,), fill, device=DEV, dtype=dtype)
    return full, full[:n]


def _guard_ok(full, n, fill, what):
    assert bool((full[n:].float().cpu() == fill).all()), f"{what}: wrote past the end"


CASTS = {"f32_bf16": (F32, BF), "bf16_f32": (BF, F32), "f32_f16": (F32, F16), "bf16_f16": (BF, F16)}


@pytest.mark.parametrize("kind", list(CASTS))
@pytest.mark.parametrize("offset", [0, 1])
def test_casts_bit_equal_to_torch(ops, kind, offset):
    """mart_cast_*: bit-equal to tensor.to(dtype) at every tail size and behind the grid cap; +-0, round-to-nearest-even ties, the fp16
    subnormal range, 65504 / 65520 / 1e5 (-> inf), NaN; ``offset`` = 1: the source view starts one element off 16-byte alignment."""
    sdt, ddt = CASTS[kind]
    fn = dict(f32_bf16=lambda s, d: ops.cast_f32_bf16(s, d), bf16_f32=lambda s, d: ops.cast_bf16_f32(s, d),
              f32_f16=lambda s, d: ops.cast_f32_f16(s, d), bf16_f16=lambda s, d: ops.cast_bf16_f16(s, d))[kind]
    for n in NS:
        x = _values(n, 100 + n % 97).to(sdt)
        buf = torch.empty(n + offset, device=DEV, dtype=sdt)
        src = buf[offset:]
        src.copy_(x)
        assert src.data_ptr() % 16 == (offset * x.element_size())
        full, dst = _guarded(n, ddt, 7.0)
        fn(src, dst)
        _same_bits(dst, x.to(ddt), f"cast_{kind} n={n} offset={offset}")
        _guard_ok(full, n, 7.0, f"cast_{kind} n={n}")


def test_cast_pad_f32_bf16(ops):
    R, C, lds, ldd = 5, 13, 16, 24
    x = _values(R * lds, 3).view(R, lds)
    dst = torch.full((R, ldd), float("nan"), device=DEV, dtype=BF)
    ops.cast_pad_f32_bf16(x.to(DEV)[:, :C], dst, R, C)
    ref = torch.zeros(R, ldd, dtype=BF)
    ref[:, :C] = x[:, :C].to(BF)
    _same_bits(dst, ref, "cast_pad_f32_bf16")


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("outs", ["f32", "bf16", "both"])
def test_add_f32_bf16(ops, with_b, outs):
    """out_f32 = a + float(b) bit for bit, out_bf16 = its round-to-nearest-even; b absent: a plain copy / cast"""
    for n in NS:
        g = torch.Generator().manual_seed(n % 1000)
        a = torch.randn(n, generator=g) * 3
        b = (torch.randn(n, generator=g) * 3).to(BF) if with_b else None
        ref = a + b.float() if with_b else a.clone()
        ff, of = _guarded(n, F32, 7.0) if outs != "bf16" else (None, None)
        fb, ob = _guarded(n, BF, 7.0) if outs != "f32" else (None, None)
        ops.add_f32_bf16(a.to(DEV), b.to(DEV) if with_b else None, out_f32=of, out_bf16=ob)
        if of is not None:
            _same_bits(of, ref, f"add_f32_bf16 f32 n={n}")
            _guard_ok(ff, n, 7.0, f"add_f32_bf16 f32 n={n}")
        if ob is not None:
            _same_bits(ob, ref.to(BF), f"add_f32_bf16 bf16 n={n}")
            _guard_ok(fb, n, 7.0, f"add_f32_bf16 bf16 n={n}")


def _z_grid():
    """4097 points on [-12, 12] and the edge values: signed zero, +-1e-30, the far tails"""
    return torch.cat([torch.linspace(-12, 12, 4097, dtype=torch.float64),
                      torch.tensor([0.0, -0.0, 1e-30, -1e-30, 20, -20, 50, -50, 88, -88, 100, -100], dtype=torch.float64)]).float()


def _act_grad64(z, act):
    """float64 derivative; the GELU CDF through erfc, which keeps its relative accuracy in the negative tail"""
    if act == "gelu":
        return 0.5 * torch.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if act == "qgelu":
        s = torch.sigmoid(1.702 * z)
        return s * (1.0 + 1.702 * z * (1.0 - s))
    if act == "stored":
        return z
    return torch.ones_like(z)


def _bf16_ulp(ref):
    """the spacing of bf16 at |ref| (float64 tensor), the subnormal spacing 2^-133 below 2^-126"""
    a = ref.abs()
    _, e = torch.frexp(a)
    ex = torch.where(a > 0, e - 1, torch.full_like(e, -126)).clamp(min=-126)
    return torch.ldexp(torch.ones_like(a), ex - 7)


@pytest.mark.parametrize("act", ["gelu", "qgelu", "none", "stored"])
def test_act_bwd_bf16(ops, act):
    """mart_act_bwd: bf16(dy * act'(z)), against the float64 derivative at the bf16 value of z, times dy, rounded to bf16, within ONE bf16 ulp of
    |ref| element by element: the kernel rounds once an f32 value that is accurate to ~1e-6 of itself.  That holds in the negative GELU tail only
    because the kernel takes the CDF from erfc there (0.5 (1 + erf) has an absolute 3e-8 against a derivative of 1e-6 at z = -5: up to 9 ulp)."""
    kind = dict(gelu=ops.ACT_GELU, qgelu=ops.ACT_QGELU, none=ops.ACT_NONE, stored=ops.ACT_STORED)[act]
    grid = _z_grid()
    worst = 0.0
    for n in NS:
        g = torch.Generator().manual_seed(7 + n % 1000)
        z = grid[torch.randint(0, grid.numel(), (n,), generator=g)].to(BF)
        if n >= grid.numel():
            z[:grid.numel()] = grid.to(BF)                      # every grid point at least once
            z[-16:] = grid[-16:].to(BF)                         # the edge values in the tail as well
        dy = torch.randn(n, generator=g).to(BF)
        ref = (_act_grad64(z.double(), act) * dy.double()).to(BF).double()
        full, out = _guarded(n, BF, 7.0)
        ops.act_bwd(dy.to(DEV), z.to(DEV), kind, out)
        got = out.cpu().double()
        assert bool(torch.isfinite(got).all())
        err = (got - ref).abs() / _bf16_ulp(ref)
        worst = max(worst, float(err.max()))
        bad = err > 1.0
        assert not bool(bad.any()), f"act_bwd {act} n={n}: {int(bad.sum())} beyond 1 ulp, worst {float(err.max()):.2f} ulp at z = {float(z[err.argmax()])}"
        _guard_ok(full, n, 7.0, f"act_bwd {act} n={n}")
    print(f"\nact_bwd {act}: worst |out - ref| = {worst:.2f} bf16 ulp")


@pytest.mark.parametrize("form", ["f32", "bf16", "both"])
def test_dropout_bwd_f32(ops, form):
    """out = (a + float(b)) * keep / (1 - p) with the mask of mart_dropout_mask(n, p, seed) and the kernel's own f32 factor 1.f / (1.f - p),
    bit for bit; p = 0: the plain sum."""
    one = torch.tensor(1.0)
    for n in NS:
        g = torch.Generator().manual_seed(n % 1000 + 1)
        a = torch.randn(n, generator=g) if form != "bf16" else None
        b = torch.randn(n, generator=g).to(BF) if form != "f32" else None
        v = (a if a is not None else 0.0) + (b.float() if b is not None else 0.0)
        da, db = (a.to(DEV) if a is not None else None), (b.to(DEV) if b is not None else None)
        for p, seed in ((0.1, 1234567 + n), (0.0, 5)):
            full, out = _guarded(n, F32, 7.0)
            ops.dropout_bwd_f32(da, db, out, n, p, seed)
            if p > 0:
                keep = torch.empty(n, device=DEV, dtype=torch.uint8)
                ops.dropout_mask(keep, p, seed)
                keep = keep.cpu().bool()
                assert 0.8 < float(keep.float().mean()) <= 1.0 or n < 100
                sc = one / (one - torch.tensor(p))                # f32, as the kernel
                ref = torch.where(keep, v * sc, torch.zeros_like(v))
            else:
                ref = v
            assert torch.equal(out.cpu(), ref), f"dropout_bwd_f32 {form} n={n} p={p}"
            _guard_ok(full, n, 7.0, f"dropout_bwd_f32 n={n}")


ROWS = [5, 5, 3, 2, 2, 0, 6, 5, 1]                       # repeated and descending


def test_gather_rows_f32(ops):
    H, ld = 100, 108
    src = torch.randn(7, ld, generator=torch.Generator().manual_seed(1))
    rows = torch.tensor(ROWS, dtype=torch.int32)
    dst = torch.full((len(ROWS), H), float("nan"), device=DEV)
    ops.gather_rows_f32(src.to(DEV)[:, :H], rows.to(DEV), dst)
    _same_bits(dst, src[rows.long(), :H], "gather_rows_f32")


def test_gather_rows_bf16(ops):
    H, ld = 136, 144
    src = torch.randn(7, ld, generator=torch.Generator().manual_seed(2)).to(BF)
    rows = torch.tensor(ROWS, dtype=torch.int32)
    dst = torch.full((len(ROWS), H), float("nan"), device=DEV, dtype=BF)
    ops.gather_rows_bf16(src.to(DEV)[:, :H], rows.to(DEV), dst)
    _same_bits(dst, src[rows.long(), :H], "gather_rows_bf16")


def test_scatter_add_rows_f32(ops):
    """dst[rows[r]] += src[r] with f32 atomics: row 5 is named three times and receives all three contributions, the columns past H and the
    rows nobody names keep their prefill bit for bit.  Bound: every one of the (at most three) adds into an element rounds a running sum that is
    no larger than |prefill| + sum |contributions|, 2^-24 relative each, in any order: 3 * 6e-8 < 1e-6 of that sum."""
    H, ld, Rd = 100, 104, 8
    g = torch.Generator().manual_seed(3)
    src = torch.randn(len(ROWS), H, generator=g)
    pre = torch.randn(Rd, ld, generator=g)
    rows = torch.tensor(ROWS, dtype=torch.int32)
    dst = pre.to(DEV)
    ops.scatter_add_rows_f32(src.to(DEV), rows.to(DEV), dst[:, :H])
    got = dst.cpu()
    ref = pre.double()
    mag = pre.double().abs()
    ref[:, :H] = ref[:, :H].index_add(0, rows.long(), src.double())
    mag[:, :H] = mag[:, :H].index_add(0, rows.long(), src.double().abs())
    assert float((ref[5, :H] - pre[5, :H].double() - src[[0, 1, 7]].double().sum(0)).abs().max()) < 1e-12      # the reference itself: three contributions
    err = (got.double() - ref).abs()
    print(f"\nscatter_add_rows_f32: worst |err| / (1e-6 * sum|terms|) = {float((err / (1e-6 * mag)).max()):.3f}")
    assert bool((err <= 1e-6 * mag).all())
    assert torch.equal(got[:, H:], pre[:, H:]) and torch.equal(got[[4, 7]], pre[[4, 7]])


def test_needed_rows_and_rows_dense(ops):
    """mart_needed_rows: column 0 = the first position of the token (absent: position 0 and status bit 1), then rel_idx[:, 0], rel_idx[:, 1], q_idx,
    a_idx, negative positions wrapped by L and the result clamped to [0, L).  mart_rows_dense: the promised rows from their compact copies, the
    first slot that names a row wins, ``fill`` everywhere else."""
    B, L, H, tok = 4, 16, 12, 103
    ids = torch.randint(200, 300, (B, L), generator=torch.Generator().manual_seed(5))
    ids[0, 3] = ids[0, 9] = tok
    ids[1, 15] = tok
    ids[3, 0] = tok                                                              # example 2 has no token
    rel = torch.tensor([[1, 2], [-1, 40], [0, 0], [-40, 15]])
    q, a = torch.tensor([5, -16, 7, 3]), torch.tensor([3, 4, -2, 0])
    rows = torch.full((B, 5), -7, dtype=torch.int32, device=DEV)
    mrow, status = torch.full((B,), -7, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.needed_rows(ids.to(DEV), tok, rel.to(DEV), q.to(DEV), a.to(DEV), rows, mrow, status)
    first = [3, 15, 0, 0]
    wrap = lambda v: min(max(v + L if v < 0 else v, 0), L - 1)
    ref = torch.tensor([[b * L + first[b]] + [b * L + wrap(int(v)) for v in (rel[b, 0], rel[b, 1], q[b], a[b])] for b in range(B)], dtype=torch.int32)
    assert torch.equal(rows.cpu(), ref) and torch.equal(mrow.cpu(), ref[:, 0]) and int(status) == 2
    one = torch.full((B, 1), -7, dtype=torch.int32, device=DEV)
    ops.needed_rows(ids.to(DEV), tok, None, None, None, one)
    assert torch.equal(one.cpu(), ref[:, :1])
    src = torch.randn(B * 5, H, generator=torch.Generator().manual_seed(6))
    dst = torch.full((B * L, H), 5.0, device=DEV)
    ops.rows_dense(src.to(DEV), rows, B, L, dst, fill=-3.0)
    dref = torch.full((B * L, H), -3.0)
    for slot in reversed(range(B * 5)):                                           # the first slot wins
        dref[int(ref.view(-1)[slot])] = src[slot]
    assert torch.equal(dst.cpu(), dref)


def test_deterministic_embedding_gradients(ops):
    """mart_text_embed_scatter_det and mart_vision_assemble_bwd_det (slice partials, reduced in order) against the float64 sums, beside their atomic
    twins mart_text_embed_scatter / mart_vision_assemble_bwd: an n-term f32 sum in any order is within n * 2^-24 * sum |terms|; the ordered forms
    repeat bit for bit."""
    B, L, H, V, P = 4, 64, 768, 37, 49
    g = torch.Generator().manual_seed(8)
    ids, tt = torch.randint(0, V, (B, L), generator=g), torch.randint(0, 2, (B, L), generator=g)
    ds = torch.randn(B * L, H, generator=g)
    dsv = torch.randn(B, 1 + 2 * P, H, generator=g)

    def sums(index, rows, x):
        z = torch.zeros(rows, H, dtype=torch.float64)
        return z.index_add(0, index, x.double()), z.index_add(0, index, x.double().abs()), torch.zeros(rows).index_add(0, index, torch.ones(index.numel()))
    pos_idx = torch.arange(L).repeat(B)
    refs = [sums(ids.view(-1), V, ds), sums(pos_idx, L, ds), sums(tt.view(-1), 2, ds)]
    vidx = torch.tensor([0] + list(range(1, P + 1)) + list(range(1, P + 1))).repeat(B)
    vref = sums(vidx, P + 1, dsv.view(-1, H))
    old, runs = ops.TN_DETERMINISTIC, {}
    try:
        for det in (True, False, True):
            ops.TN_DETERMINISTIC = det
            out = [torch.zeros(V, H, device=DEV), torch.zeros(L, H, device=DEV), torch.zeros(2, H, device=DEV)]
            ops.text_embed_scatter(ds.to(DEV), ids.to(DEV), tt.to(DEV), *out, B, L, H)
            dpe, dcls, dpos = torch.empty(B * 2 * P, H, device=DEV, dtype=BF), torch.zeros(H, device=DEV), torch.zeros(P + 1, H, device=DEV)
            ops.vision_assemble_bwd(dsv.to(DEV), dpe, dcls, dpos, B, P, H)
            for got, (ref, mag, cnt) in zip(out + [dpos], refs + [vref]):
                bound = cnt.double()[:, None] * 2.0 ** -24 * mag
                assert bool(((got.cpu().double() - ref).abs() <= bound).all()), f"deterministic={det}"
            cur = [t.cpu() for t in out + [dpos, dcls, dpe]]
            if det and det in runs:
                assert all(torch.equal(x, y) for x, y in zip(cur, runs[det]))
            runs[det] = cur
    finally:
        ops.TN_DETERMINISTIC = old
