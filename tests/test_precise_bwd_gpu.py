"""The fp32 verification-mode backward (csrc/precise.hip) kernel by kernel against float64, through mkg_analogy_amd.ops: mart_attn_bwd_f32, the
scalar forward attn_f32_k, the three split kernels (two and three terms) and the products on them, mart_act_f32 / mart_act_bwd_f32,
mart_colsum_f32, mart_patchify_f32, mart_vision_assemble_f32.

The control rule: wherever a float kernel is compared with float64, the test computes the reference (torch float64, CPU), the control (the
identical torch expression in float32, CPU) and both errors max|x - ref| / max|ref| per output tensor; the gate is E_kernel <= 8 x E_control (a
different summation order, the hardware exp2 / rcp), and never above a cap of 1e-5 (head dim 64) / 1e-4 (the head-dim-768 fusion shape).  Layouts,
splits and gathers are compared bit for bit (all of them held on an MI355X).  The figures measured on an MI355X stand in the docstrings, as
max control / max kernel error over the cases of a test."""
import math

import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mkg_analogy_amd import ops as o
    o.require_gpu()
    return o


DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _relerr(x, ref):
    return float((x.double() - ref).abs().max()) / float(ref.abs().max())


def _gate(what, got, ref, ctl, cap=None, norm=None):
    """E_kernel <= min(8 x E_control, cap); both errors printed.  ``norm`` replaces max|ref| as the scale where the issue defines another one."""
    n = float(ref.abs().max()) if norm is None else float(norm)
    ek, ec = float((got.double() - ref).abs().max()) / n, float((ctl.double() - ref).abs().max()) / n
    gate = 8 * ec if cap is None else min(8 * ec, cap)
    print(f"   {what}: control {ec:.2e}  kernel {ek:.2e}  gate {gate:.2e}")
    assert math.isfinite(ek) and ek <= gate, f"{what}: kernel error {ek:.3e} above the gate {gate:.3e} (control {ec:.3e})"
    return ek, ec


# ------------------------------------------------------------------------------------------------------------ attention backward
def _attn_autograd(dt, q, k, v, dctx, nh, scale, pk=None, pv=None, mask=None, sep=None, w0=None, w1=None, skip0=False):
    """Autograd through the _ref_attn formula of tests/test_precise_gpu.py in dtype ``dt`` (inputs [B, S, H] f32 CPU tensors): scale, reweight with
    torch.clamp(w0, 0, 0.5) / torch.clamp(w1, 0.5, 1) on the keys >= sep (query rows < sep / >= sep; row 0 exempt with ``skip0``), the -10000
    additive mask, softmax, @ V; loss = (out * dctx).sum().  Returns the gradients and, for the dw bound, A0 / A1 = sum |d(post-reweight score) *
    pre-reweight score| over each weight's region."""
    B, Sq, H = q.shape
    D = H // nh
    leaf = lambda t: None if t is None else t.to(dt).clone().requires_grad_(True)
    q_, k_, v_, pk_, pv_, w0_, w1_ = (leaf(t) for t in (q, k, v, pk, pv, w0, w1))
    sp = lambda x: x.view(B, -1, nh, D).transpose(1, 2)
    Q, K, V = sp(q_), sp(k_), sp(v_)
    if pk is not None:
        K, V = torch.cat([sp(pk_), K], 2), torch.cat([sp(pv_), V], 2)
    s_pre = Q @ K.transpose(-1, -2) * scale
    s, R0, R1 = s_pre, None, None
    if sep is not None:
        Sk = K.shape[2]
        qi, kj = torch.arange(Sq)[None, :, None], torch.arange(Sk)[None, None, :]
        se = sep.view(B, 1, 1)
        on = (kj >= se) & ((qi > 0) if skip0 else (qi >= 0))
        R0, R1 = (on & (qi < se))[:, None], (on & (qi >= se))[:, None]
        one = torch.ones((), dtype=dt)
        s = s_pre * torch.where(R0, torch.clamp(w0_, 0, 0.5), torch.where(R1, torch.clamp(w1_, 0.5, 1), one))
        s.retain_grad()
    s2 = s if mask is None else s + ((1 - mask)[:, None, None, :].to(dt) * -10000.0)
    out = (torch.softmax(s2, -1) @ V).transpose(1, 2).reshape(B, Sq, H)
    (out * dctx.to(dt)).sum().backward()
    res = dict(dq=q_.grad, dk=k_.grad, dv=v_.grad, dpk=None if pk is None else pk_.grad, dpv=None if pv is None else pv_.grad)
    if sep is not None:
        t = (s.grad * s_pre.detach()).abs()
        res.update(dw=torch.stack([w0_.grad.view(()), w1_.grad.view(())]), A=(float((t * R0).sum()), float((t * R1).sum())))
    return res


def _run_attn_bwd(ops, B, nh, D, Sq, Sk, scale, Lp=0, mask=None, sep=None, w=None, skip0=False, seed=0, qscale=1.0):
    """One call of mart_attn_bwd_f32 in the layout of engine_precise: q / k / v and dq / dk / dv are column slices of [B * S, 3H] buffers (ld != H),
    dq pre-filled with NaN (written), everything else pre-filled with values (accumulated).  Returns kernel outputs, float64 references (prefill +
    gradient) and float32 controls."""
    H = nh * D
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    qkv, dctx = r(B * Sq, 3 * H), r(B * Sq, H)
    qkv[:, :H] *= qscale
    pre = r(B * Lp, 3 * H) if Lp else None
    fill, pfill = 0.5 * r(B * Sq, 3 * H), (0.5 * r(B * Lp, 3 * H) if Lp else None)
    dqkv = fill.clone()
    dqkv[:, :H] = float("nan")
    dqkv = dqkv.to(DEV)
    dpre = pfill.to(DEV) if Lp else None
    dqd, dpd = qkv.to(DEV), (pre.to(DEV) if Lp else None)
    w0 = w1 = dw = None
    wfill = torch.tensor([0.25, -0.125])
    kw = {}
    if sep is not None:
        w0, w1 = torch.tensor([w[0]]), torch.tensor([w[1]])
        dw = wfill.to(DEV)
        kw = dict(sep=sep.to(DEV), sep_stride=1, w0=w0.to(DEV), w1=w1.to(DEV), rw_skip_row0=skip0)
    ops.attn_bwd_f32(dctx=dctx.to(DEV), dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:],
                     dpk=dpre[:, H:2 * H] if Lp else None, dpv=dpre[:, 2 * H:] if Lp else None, dw=dw,
                     q=dqd[:, :H], k=dqd[:, H:2 * H], v=dqd[:, 2 * H:], B=B, nh=nh, D=D, Sq=Sq, Sk=Sk, scale=scale,
                     pk=dpd[:, H:2 * H] if Lp else None, pv=dpd[:, 2 * H:] if Lp else None, Lp=Lp,
                     attn_mask=mask.to(DEV) if mask is not None else None, **kw)
    torch.cuda.synchronize()
    v3 = lambda t, S, j: t[:, j * H:(j + 1) * H].reshape(B, S, H)
    args = [v3(qkv, Sq, 0), v3(qkv, Sk, 1), v3(qkv, Sk, 2), dctx.view(B, Sq, H), nh, scale]
    akw = dict(pk=v3(pre, Lp, 1) if Lp else None, pv=v3(pre, Lp, 2) if Lp else None, mask=mask, sep=sep, w0=w0, w1=w1, skip0=skip0)
    r64, r32 = _attn_autograd(F64, *args, **akw), _attn_autograd(F32, *args, **akw)
    got = dict(dq=v3(dqkv.cpu(), Sq, 0), dk=v3(dqkv.cpu(), Sk, 1), dv=v3(dqkv.cpu(), Sk, 2))
    pf = dict(dq=0.0, dk=v3(fill, Sk, 1), dv=v3(fill, Sk, 2))
    if Lp:
        got.update(dpk=v3(dpre.cpu(), Lp, 1), dpv=v3(dpre.cpu(), Lp, 2))
        pf.update(dpk=v3(pfill, Lp, 1), dpv=v3(pfill, Lp, 2))
        assert torch.equal(dpre.cpu()[:, :H], pfill[:, :H])                     # the query block of the prefix buffer is nobody's output
    ref = {n: (pf[n].double() if torch.is_tensor(pf[n]) else 0.0) + r64[n] for n in got}
    ctl = {n: (pf[n] if torch.is_tensor(pf[n]) else 0.0) + r32[n] for n in got}
    if sep is not None:
        got["dw"], ref["dw"], ref["A"] = dw.cpu(), wfill.double() + r64["dw"], r64["A"]
        ref["wfill"] = wfill
    return got, ref, ctl


def _gate_grads(what, got, ref, ctl, cap):
    return {n: _gate(f"{what} {n}", got[n], ref[n], ctl[n], cap) for n in ("dq", "dk", "dv", "dpk", "dpv") if n in got}


def test_attn_bwd_vision_with_prefix(ops):
    """Sq = Sk = 33, Lp = 24: a ragged last 16-row query tile (one row), fewer than 64 keys; all five gradients.
    MI355X (control / kernel): dq 5.3e-7 / 4.8e-7, dk 1.5e-7 / 1.5e-7, dv 1.5e-7 / 1.4e-7, dpk 1.9e-7 / 1.5e-7, dpv 1.7e-7 / 1.7e-7."""
    print()
    got, ref, ctl = _run_attn_bwd(ops, 2, 2, 64, 33, 33, 0.125, Lp=24, seed=1)
    assert set(got) == {"dq", "dk", "dv", "dpk", "dpv"}
    _gate_grads("vision + prefix", got, ref, ctl, 1e-5)


def test_attn_bwd_vision_without_prefix(ops):
    """Sq = Sk = 70: a second pass of the 64-lane key loops.
    MI355X (control / kernel): dq 3.6e-7 / 3.0e-7, dk 2.4e-7 / 1.6e-7, dv 3.2e-7 / 2.7e-7."""
    print()
    got, ref, ctl = _run_attn_bwd(ops, 2, 2, 64, 70, 70, 0.125, seed=2)
    _gate_grads("vision, no prefix", got, ref, ctl, 1e-5)


@pytest.mark.parametrize("skip0", [False, True])
@pytest.mark.parametrize("w", [(0.31, 0.77), (0.5, 0.5), (0.0, 1.0), (0.6, 0.4)])
@pytest.mark.parametrize("L,sep", [(40, (17, 11)), (101, (30, 64))])
def test_attn_bwd_text_mask_reweight_dw(ops, L, sep, w, skip0):
    """Key mask (the last 7 keys of example 0), adaptive reweight and its weight gradients.  At the clamp bounds the sub-gradient is 1 (torch.clamp's
    backward, confirmed by the CPU autograd reference here), outside them both dw are exactly 0: the prefill comes back untouched.
    dw0 / dw1: |error| <= 1e-5 * A, A = float64 sum of |d(post-reweight score) * pre-reweight score| over the weight's region: every term carries
    ~1e-6 relative (expf of an argument of magnitude <= 16 known to 1 ulp, f32 sums); one dropped or mis-assigned query row shows at >= 1e-3 * A.
    The |ref|-relative form is unusable: dw1 cancels to 1e-3 of A.
    MI355X, over the 16 cases (control / kernel): dq 3.0e-7 .. 6.4e-7 / 2.9e-7 .. 6.4e-7, dk 1.6e-7 .. 2.5e-7 / 1.7e-7 .. 2.2e-7, dv 1.7e-7 .. 2.7e-7 /
    1.5e-7 .. 2.2e-7; |dw error| at most 1.7e-8 * A (1.5e-5 against a bound of 8.8e-3); outside the bounds dw came back bit-equal to its prefill."""
    print()
    mask = torch.ones(2, L, dtype=torch.int64)
    mask[0, L - 7:] = 0
    got, ref, ctl = _run_attn_bwd(ops, 2, 2, 64, L, L, 0.125, mask=mask, sep=torch.tensor(sep, dtype=torch.int64), w=w, skip0=skip0, seed=3 + L)
    _gate_grads(f"text L={L} w={w} skip0={skip0}", got, ref, ctl, 1e-5)
    inside = (0.0 <= w[0] <= 0.5, 0.5 <= w[1] <= 1.0)
    for i in (0, 1):
        e, A = abs(float(got["dw"][i]) - float(ref["dw"][i])), ref["A"][i]
        print(f"   dw{i}: ref {float(ref['dw'][i]) - float(ref['wfill'][i]):+.5e}  |err| {e:.2e}  bound 1e-5 * A = {1e-5 * A:.2e}")
        if inside[i]:
            assert A > 0 and abs(float(ref["dw"][i]) - float(ref["wfill"][i])) > 0          # the sub-gradient at (and inside) the bounds is 1
            assert e <= 1e-5 * A
        else:
            assert float(ref["dw"][i]) == float(ref["wfill"][i]) and float(got["dw"][i]) == float(ref["wfill"][i])


def test_attn_bwd_fusion_shared_dk_dv(ops):
    """The fusion op as engine_precise calls it: nh = 1, D = 768, Sq = 23, Sk = 99, scale 1, queries x 0.3, k = v = the visual rows and dk = dv = ONE
    buffer, which must receive dK + dV on top of its prefill.
    MI355X (control / kernel): dq 3.7e-6 / 3.2e-6, dk + dv 4.2e-6 / 4.4e-6 (gates 3.0e-5 / 3.4e-5, under the 1e-4 cap)."""
    print()
    B, H, Sq, Sk = 2, 768, 23, 99
    g = torch.Generator().manual_seed(9)
    c, vis, dctx = 0.3 * torch.randn(B * Sq, H, generator=g), torch.randn(B * Sk, H, generator=g), torch.randn(B * Sq, H, generator=g)
    fill = 0.5 * torch.randn(B * Sk, H, generator=g)
    dq, dvis = torch.full((B * Sq, H), float("nan"), device=DEV), fill.to(DEV)
    dv_ = vis.to(DEV)
    ops.attn_bwd_f32(dctx=dctx.to(DEV), dq=dq, dk=dvis, dv=dvis, q=c.to(DEV), k=dv_, v=dv_, B=B, nh=1, D=H, Sq=Sq, Sk=Sk, scale=1.0)
    torch.cuda.synchronize()

    def ref(dt):
        q_, v_ = c.to(dt).view(B, Sq, H).requires_grad_(True), vis.to(dt).view(B, Sk, H).requires_grad_(True)
        out = torch.softmax(q_ @ v_.transpose(-1, -2) * 1.0, -1) @ v_
        (out * dctx.to(dt).view(B, Sq, H)).sum().backward()
        return q_.grad, fill.to(dt).view(B, Sk, H) + v_.grad
    (q64, v64), (q32, v32) = ref(F64), ref(F32)
    _gate("fusion dq", dq.cpu().view(B, Sq, H), q64, q32, 1e-4)
    _gate("fusion dk + dv (one buffer)", dvis.cpu().view(B, Sk, H), v64, v32, 1e-4)


def test_attn_bwd_refusals(ops):
    """Each raises through the error check of the binding before anything is launched: a key mask together with a prefix (the kernel would index the
    [B, Sk] mask with keys up to Lp + Sk), head dim 32, and D = 64 with Lp + Sk = 811, one key past the 160 KB LDS bound of the score tiles."""
    from mkg_analogy_amd._lib import MartError
    B, nh, D, S, Lp = 1, 2, 64, 16, 8
    H = nh * D
    z = lambda *s: torch.zeros(*s, device=DEV)
    qkv, dqkv, pre, dpre, dctx = z(B * S, 3 * H), z(B * S, 3 * H), z(B * Lp, 3 * H), z(B * Lp, 3 * H), z(B * S, H)
    base = dict(dctx=dctx, dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:], q=qkv[:, :H], k=qkv[:, H:2 * H], v=qkv[:, 2 * H:],
                B=B, nh=nh, D=D, Sq=S, Sk=S, scale=0.125)
    ops.attn_bwd_f32(**base)                                                               # the plain call is accepted
    mask = torch.ones(B, Lp + S, dtype=torch.int64, device=DEV)                           # as long as the keys, whatever the kernel would read
    with pytest.raises(MartError, match="mask with prefix"):
        ops.attn_bwd_f32(**base, pk=pre[:, H:2 * H], pv=pre[:, 2 * H:], Lp=Lp, dpk=dpre[:, H:2 * H], dpv=dpre[:, 2 * H:], attn_mask=mask)
    with pytest.raises(MartError, match="head dim"):
        ops.attn_bwd_f32(**{**base, "nh": 4, "D": 32})
    Sk = 811
    kv, dkv = z(B * Sk, 3 * H), z(B * Sk, 3 * H)
    with pytest.raises(MartError, match="LDS"):
        ops.attn_bwd_f32(**{**base, "k": kv[:, H:2 * H], "v": kv[:, 2 * H:], "dk": dkv[:, H:2 * H], "dv": dkv[:, 2 * H:], "Sk": Sk})
    torch.cuda.synchronize()
    assert float(dqkv.abs().max()) == 0.0 and float(dkv.abs().max()) == 0.0 and float(dpre.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ the scalar forward kernel
def test_attn_fwd_scalar_fallback(ops):
    """attn_f32_k<64> / <768>, which mart_attn_fwd_f32 reaches only when the matrix-pipe kernels do not apply: D = 64 with a context view 4 bytes off
    16-byte alignment (fast = 0 and ctx & 15 != 0 skip attn_split_fwd_k and attn_f32_mfma_k), mask + reweight; D = 768 with Sk = 520 > 512 (skips
    fusion_f32_mfma_k).  Against float64 with the gates of the existing forward test: 2e-5 / 2e-4 absolute on unit-scale outputs.
    MI355X: max|err| 4.5e-7 (D = 64) and 2.0e-5 (D = 768)."""
    from tests.test_precise_gpu import _ref_attn
    g = torch.Generator().manual_seed(31)
    B, nh, H, L = 2, 2, 128, 40
    tq = torch.randn(B * L, 3 * H, generator=g)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[0, 33:] = 0
    sep, w0, w1 = torch.tensor([17, 11]), torch.tensor([0.31]), torch.tensor([0.77])
    buf = torch.full((B * L, H + 4), float("nan"), device=DEV)
    ctx = buf[:, 1:1 + H]
    assert ctx.data_ptr() % 16 == 4 and ctx.stride(0) % 4 == 0
    dt = tq.to(DEV)
    ops.attn_fwd_f32(q=dt[:, :H], k=dt[:, H:2 * H], v=dt[:, 2 * H:], ctx=ctx, B=B, nh=nh, D=64, Sq=L, Sk=L, scale=0.125,
                     attn_mask=mask.to(DEV), sep=sep.to(DEV), sep_stride=1, w0=w0.to(DEV), w1=w1.to(DEV))
    v3 = lambda j: tq[:, j * H:(j + 1) * H].reshape(B, L, H)
    ref = _ref_attn(v3(0), v3(1), v3(2), nh, 0.125, mask=mask, sep=sep, w0=w0, w1=w1)
    e1 = float((ctx.cpu().double().view(B, L, H) - ref).abs().max())
    b = buf.cpu()
    assert bool(b[:, 0].isnan().all()) and bool(b[:, 1 + H:].isnan().all())               # nothing written beside the view
    H2, Sq, Sk = 768, 17, 520
    c, vis = 0.3 * torch.randn(Sq, H2, generator=g), torch.randn(Sk, H2, generator=g)
    fus = torch.full((Sq, H2), float("nan"), device=DEV)
    dvis = vis.to(DEV)
    ops.attn_fwd_f32(q=c.to(DEV), k=dvis, v=dvis, ctx=fus, B=1, nh=1, D=H2, Sq=Sq, Sk=Sk, scale=1.0)
    ref2 = _ref_attn(c.view(1, Sq, H2), vis.view(1, Sk, H2), vis.view(1, Sk, H2), 1, 1.0)
    e2 = float((fus.cpu().double().view(1, Sq, H2) - ref2).abs().max())
    print(f"\nattn_f32_k scalar kernels max|err|: D = 64 misaligned ctx, mask + reweight {e1:.2e}; D = 768, 520 keys {e2:.2e}")
    assert e1 < 2e-5 and e2 < 2e-4


# ------------------------------------------------------------------------------------------------------------ splits
def _terms(x):
    """h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), every difference in f32"""
    h = x.to(BF)
    r1 = x - h.float()
    m = r1.to(BF)
    return h, m, (r1 - m.float()).to(BF)


def _kcat(x, role, terms):
    h, m, l = _terms(x)
    if terms == 3:
        return torch.cat([h, h, m, m, h, l] if role == 0 else [h, m, h, m, l, h], 1)
    return torch.cat([h, m, h] if role == 0 else [h, h, m], 1)


def _same(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got.cpu().view(torch.int16), ref.view(torch.int16))


def _x(rows, cols, seed):
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed)) * 3
    x[0, :4] = torch.tensor([0.0, -0.0, 1.0, -2.5])
    return x


@pytest.mark.parametrize("role", [0, 1])
def test_split_bf16x3_layouts_bit_exact(ops, role):
    """mart_split_bf16x3: three terms [h|h|m|m|h|l] / [h|m|h|m|l|h] (split3_k); two terms through split3_k (a source view one float off 16-byte
    alignment) and through split3_fast_k at rows = 171, K = 12, ld = 20 (K % 8 != 0, fewer quads than one 1024-quad group)."""
    x = _x(37, 72, 40)
    assert _same(ops.split_bf16x3(x.to(DEV)[:, 4:68], role, terms=3), _kcat(x[:, 4:68], role, 3))
    off = x.to(DEV)[:, 1:69]
    assert off.data_ptr() % 16 == 4
    assert _same(ops.split_bf16x3(off, role, terms=2), _kcat(x[:, 1:69], role, 2))
    assert _same(ops.split_bf16x3(off, role, terms=3), _kcat(x[:, 1:69], role, 3))
    y = _x(171, 20, 41)
    src = y.to(DEV)[:, :12]
    assert src.data_ptr() % 16 == 0
    assert _same(ops.split_bf16x3(src, role, terms=2), _kcat(y[:, :12], role, 2))


@pytest.mark.parametrize("terms", [2, 3])
@pytest.mark.parametrize("role", [0, 1])
def test_split_bf16x3_rows_gather_bit_exact(ops, role, terms):
    """mart_split_bf16x3_rows: split3_k with a gather (repeated and descending indices), two and three terms"""
    x = _x(9, 72, 42)
    idx = torch.tensor([8, 8, 5, 3, 3, 0, 7, 8, 1], dtype=torch.int32)
    got = ops.split_bf16x3_rows(x.to(DEV)[:, :64], idx.to(DEV), role, terms=terms)
    assert _same(got, _kcat(x[idx.long(), :64], role, terms))


@pytest.mark.parametrize("terms", [2, 3])
@pytest.mark.parametrize("role", [0, 1])
def test_split_bf16x3_stack_bit_exact(ops, role, terms):
    """mart_split_bf16x3_stack: [h;m;h] / [h;h;m] and the six-block form [h;h;m;m;h;l] / [h;m;h;m;l;h], strided source rows"""
    x = _x(77, 72, 43)
    h, m, l = _terms(x[:, :64])
    if terms == 3:
        ref = torch.cat([h, h, m, m, h, l] if role == 0 else [h, m, h, m, l, h], 0)
    else:
        ref = torch.cat([h, m, h] if role == 0 else [h, h, m], 0)
    assert _same(ops.split_bf16x3_stack(x.to(DEV)[:, :64], role, terms=terms), ref)


def test_split_products_vs_f64(ops):
    """The products the splits exist for.  gemm_nt on K-concatenated splits (M = 77, N = 64, K = 128) and gemm_tn on row-stacked splits (M = 77,
    NX = 64, NY = 128): three terms by the control rule (torch f32 matmul as the control), and no worse than two terms; two terms within their own
    derived bound: |x - h| <= 2^-9 |x| and |x - h - m| <= 2^-18 |x| (two bf16 roundings), so h h' + m h' + h m' misses m m' and the two remainders,
    3 * 2^-18 sum |x||y|; with the f32 accumulation of the 3K products that is the "2^-16 relative" of csrc/precise.hip: 2^-16 * max sum |x||y|.
    MI355X: gemm_nt three terms control 3.3e-7 / kernel 4.5e-7 (max|err| 1.9e-5 against 2.2e-4 with two terms, bound 1.7e-3); gemm_tn 2.9e-7 /
    2.9e-7 (1.2e-5 against 2.4e-4, bound 1.2e-3).  No shape was refused by the GEMMs."""
    print()
    g = torch.Generator().manual_seed(50)
    M, N, K = 77, 64, 128
    a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    ref, ctl, mag = a.double() @ w.double().T, a @ w.T, float((a.double().abs() @ w.double().abs().T).max())
    err = {}
    for terms in (2, 3):
        out = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm_nt(ops.split_bf16x3(a.to(DEV), 0, terms=terms), ops.split_bf16x3(w.to(DEV), 1, terms=terms), out)
        err[terms] = float((out.cpu().double() - ref).abs().max())
        if terms == 3:
            _gate("gemm_nt on three-term splits", out.cpu(), ref, ctl)
    print(f"   gemm_nt max|err|: two terms {err[2]:.2e} (bound {2.0 ** -16 * mag:.2e}), three terms {err[3]:.2e}")
    assert err[3] <= err[2] <= 2.0 ** -16 * mag
    NX, NY = 64, 128
    x, y = torch.randn(M, NX, generator=g), torch.randn(M, NY, generator=g)
    ref, ctl, mag = x.double().T @ y.double(), x.T @ y, float((x.double().abs().T @ y.double().abs()).max())
    for terms in (2, 3):
        out = torch.zeros(NX, NY, device=DEV)
        ops.gemm_tn(ops.split_bf16x3_stack(x.to(DEV), 0, terms=terms), ops.split_bf16x3_stack(y.to(DEV), 1, terms=terms), out)
        err[terms] = float((out.cpu().double() - ref).abs().max())
        if terms == 3:
            _gate("gemm_tn on three-term stacks", out.cpu(), ref, ctl)
    print(f"   gemm_tn max|err|: two terms {err[2]:.2e} (bound {2.0 ** -16 * mag:.2e}), three terms {err[3]:.2e}")
    assert err[3] <= err[2] <= 2.0 ** -16 * mag


# ------------------------------------------------------------------------------------------------------------ activations, column sums
def _z_grid():
    return torch.cat([torch.linspace(-12, 12, 4097, dtype=F64), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 20, -20, 50, -50, 88, -88, 100, -100], dtype=F64)]).float()


def _act(z, act):
    """value and derivative in the dtype of z; the GELU CDF as 0.5 erfc(-z / sqrt 2)"""
    if act == "gelu":
        cdf = 0.5 * torch.erfc(-z / math.sqrt(2.0))
        return z * cdf, cdf + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    s = torch.sigmoid(1.702 * z)
    return z * s, s * (1.0 + 1.702 * z * (1.0 - s))


@pytest.mark.parametrize("act", ["gelu", "qgelu"])
def test_act_f32_and_bwd(ops, act):
    """mart_act_f32 / mart_act_bwd_f32 (erf GELU, quick-GELU) on 4097 points of [-12, 12] and the edges 0, -0, +-1e-30, +-20 ... +-100: finite
    everywhere, value and dy * derivative by the control rule, each error normalised by its tensor's max|ref|.
    MI355X (control / kernel): gelu value 3.5e-9 / 4.4e-9, derivative 7.9e-8 / 7.0e-8; quick-gelu value 7.4e-9 / 7.4e-9, derivative 6.7e-7 / 6.7e-7
    (the 1 - sigmoid cancellation of the formula, in the kernel and the control alike)."""
    print()
    kind = dict(gelu=ops.ACT_GELU, qgelu=ops.ACT_QGELU)[act]
    z = _z_grid()
    dy = torch.randn(z.numel(), generator=torch.Generator().manual_seed(60))
    a64, g64 = _act(z.double(), act)
    a32, g32 = _act(z, act)
    a, dz = ops.act_f32(z.to(DEV), kind).cpu(), ops.act_bwd_f32(dy.to(DEV), z.to(DEV), kind).cpu()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(dz).all())
    _gate(f"act_f32 {act}", a, a64, a32)
    _gate(f"act_bwd_f32 {act}", dz, g64 * dy.double(), g32 * dy)


def test_act_f32_none_is_a_pass_through(ops):
    z = _z_grid()
    dy = torch.randn(z.numel(), generator=torch.Generator().manual_seed(61))
    assert torch.equal(ops.act_f32(z.to(DEV), ops.ACT_NONE).cpu().view(torch.int32), z.view(torch.int32))
    assert torch.equal(ops.act_bwd_f32(dy.to(DEV), z.to(DEV), ops.ACT_NONE).cpu(), dy)


@pytest.mark.parametrize("R", [255, 256, 4095, 4097])
def test_colsum_f32(ops, R):
    """mart_colsum_f32 on both sides of its 1 / 8 / 64 row-slice thresholds, R no multiple of the slice count, C = 100 (no multiple of the 64-column
    workgroup), ld = 104, accumulated onto a pre-filled output.  Control rule, normalised by max over columns of sum_r |src|.
    MI355X (control / kernel): R = 255 2.1e-8 / 3.3e-8, 256 1.9e-8 / 1.9e-8, 4095 6.9e-9 / 9.4e-9, 4097 9.0e-9 / 1.4e-8."""
    print()
    C, ld = 100, 104
    g = torch.Generator().manual_seed(R)
    src, pre = torch.randn(R, ld, generator=g), torch.randn(C, generator=g)
    full = torch.full((ld,), 7.0, device=DEV)
    full[:C] = pre.to(DEV)
    ops.colsum_f32(src.to(DEV)[:, :C], full[:C])
    s = src[:, :C]
    _gate(f"colsum_f32 R={R}", full[:C].cpu(), s.double().sum(0) + pre.double(), s.sum(0) + pre, norm=s.double().abs().sum(0).max())
    assert bool((full[C:].cpu() == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ layouts
def _patches(img, p):
    """[N, 3, S, S] -> [N * (S/p)^2, 3 p p]: patches row-major, columns in (c, ky, kx) order"""
    return F_.unfold(img, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, 3 * p * p)


def test_patchify_f32_bit_exact(ops):
    B, S, p = 2, 32, 16
    P, K = (S // p) ** 2, 3 * p * p
    g = torch.Generator().manual_seed(70)
    pix = torch.randn(B, 2, 3, S, S, generator=g)
    out = torch.full((B * 2 * P, K), float("nan"), device=DEV)
    ops.patchify_f32(pix.to(DEV), None, out, B, S, p)
    assert torch.equal(out.cpu(), _patches(pix.view(B * 2, 3, S, S), p))
    table = torch.randn(5, 3, S, S, generator=g)
    index = torch.tensor([4, -1, 2, 4], dtype=torch.int32)              # a missing slot (zero rows) and a repeated entry
    out = torch.full((B * 2 * P, K), float("nan"), device=DEV)
    ops.patchify_f32(table.to(DEV), index.to(DEV), out, B, S, p)
    imgs = torch.stack([table[i] if i >= 0 else torch.zeros(3, S, S) for i in index.tolist()])
    ref = _patches(imgs, p)
    assert torch.equal(out.cpu(), ref) and float(ref[P:2 * P].abs().max()) == 0.0


@pytest.mark.parametrize("tail_shift", [0, 1])
def test_vision_assemble_f32_bit_exact(ops, tail_shift):
    """s[b, t] = cls + pos[0] (t = 0), patch(b, t - 1) + pos[t] (first image), patch(b, t - 1) + pos[t - P - tail_shift] (second image)"""
    B, P, H = 2, 4, 64
    g = torch.Generator().manual_seed(71)
    patch, cls, pos = torch.randn(B * 2 * P, H, generator=g), torch.randn(H, generator=g), torch.randn(P + 1, H, generator=g)
    s = torch.full((B * (1 + 2 * P), H), float("nan"), device=DEV)
    ops.vision_assemble_f32(patch.to(DEV), cls.to(DEV), pos.to(DEV), s, B, P, H, tail_shift=tail_shift)
    pidx = torch.tensor([0] + list(range(1, P + 1)) + [t - P - tail_shift for t in range(P + 1, 2 * P + 1)])
    ref = torch.cat([cls.expand(B, 1, H), patch.view(B, 2 * P, H)], 1) + pos[pidx][None]
    assert torch.equal(s.cpu(), ref.reshape(-1, H))
