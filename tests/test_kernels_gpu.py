"""Kernel-level parity: every C-ABI entry point against a plain PyTorch fp32 reference of the same op,
on seeded inputs, called through ctypes (mkg_analogy_amd.ops).  GPU only."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mkg_analogy_amd import ops as o
    o.require_gpu()
    return o


DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def close(got, ref, atol, rtol, what=""):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = (err > tol)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} bad, max err {float(err.max()):.4g}, ref max {float(ref.abs().max()):.4g}"


# ----------------------------------------------------------------------------------------- NT GEMM
@pytest.mark.parametrize("M,N,K,cfg", [(300, 200, 128, 128), (1000, 768, 768, 128), (1000, 768, 768, 256),
                                       (3144, 2304, 768, 0), (64, 393, 768, 0), (257, 2063, 768, 0), (2048, 768, 3072, 256)])
def test_gemm_nt_plain(ops, M, N, K, cfg):
    A, B = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05)
    out = torch.empty(M, N, device=DEV, dtype=F32)
    ops.gemm_nt(A, B, out, tile_cfg=cfg)
    close(out, A.float() @ B.float().t(), 2e-3, 2e-3, "gemm_nt f32 out")
    outb = torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, B, outb, tile_cfg=cfg)
    close(outb, A.float() @ B.float().t(), 2e-2, 1e-2, "gemm_nt bf16 out")


@pytest.mark.parametrize("K,K2", [(64, 0), (192, 0), (64, 64), (128, 192), (832, 0)])
def test_gemm_nt_4phase_loop_edges(ops, K, K2):
    """The 4-phase loop of the 256x256 kernel (gemm_nt.hip PIPE 4: 16x16x32 MFMAs, half-tile LDS-DMA two K-tiles ahead, counted waits in the read
    segments) at the contraction lengths where its prologue / drain paths differ: one, two, three K-tiles, the dual-K switch on the first and in the
    middle of the ring, an odd tile count -- plain f32 output, the persistent bf16 lane over more tiles than CUs, a row gather on A and the
    general-epilogue kernel, all against torch and each other (bit-equal where the same loop computes the same sums)."""
    M, N = 256 * 270 + 33, 768
    Af, Bf = rnd(M, K + K2, seed=21), rnd(N, K + K2, seed=22, scale=0.06)      # the second operand pair shares the first one's row stride (API contract)
    A, B = Af[:, :K], Bf[:, :K]
    A2, B2 = (Af[:, K:], Bf[:, K:]) if K2 else (None, None)
    ref = A.float() @ B.float().t() + (A2.float() @ B2.float().t() if K2 else 0.0)
    bias = rnd(N, seed=25, dtype=F32)
    kw = dict(A2=A2, B2=B2) if K2 else {}
    of = torch.empty(M, N, device=DEV, dtype=F32)
    ops.gemm_nt(A, B, of, bias=bias, tile_cfg=256, **kw)
    close(of, ref + bias, 2e-3, 2e-3, "4-phase f32")
    ob, og = torch.empty(M, N, device=DEV, dtype=BF), torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, B, ob, bias=bias, tile_cfg=256, **kw)                  # persistent bf16 lane (813 tiles on 256 CUs)
    ops.gemm_nt(A, B, og, bias=bias, tile_cfg=2561, **kw)                 # general epilogue, same loop
    assert torch.equal(ob, og)
    assert torch.equal(ob, (of).to(BF))                                   # the f32 lane rounds the same sums
    for _ in range(3):                                                    # run-to-run identical (a race in the ring would show up here first)
        o2 = torch.empty_like(ob)
        ops.gemm_nt(A, B, o2, bias=bias, tile_cfg=256, **kw)
        assert torch.equal(ob, o2)
    if not K2:
        rows = torch.randperm(M, device=DEV)[:1000].to(torch.int32).contiguous()
        ogat = torch.empty(1000, N, device=DEV, dtype=F32)
        ops.gemm_nt(A, B, ogat, a_rows=rows, M=1000, tile_cfg=256)
        assert torch.equal(ogat + bias, of[rows.long()]) or float((ogat + bias - of[rows.long()]).abs().max()) < 1e-5


def test_gemm_nt_tile_blocked_weights_take_the_8_phase_kernel(ops):
    """b_blocked (weights stored as contiguous 256 x 64 blocks, mart_block_table) is served by the 8-phase loop's general-epilogue kernel -- the only
    product path that still runs it (the other one: operands beyond 2^31 elements): same product as the row-major call on the 4-phase loop, to the
    rounding of a different summation order, with bias + f32 residual + bf16 copy through the general epilogue."""
    M, N, K = 2000, 768, 768
    A, W = rnd(M, K, seed=31), rnd(N, K, seed=32, scale=0.05)
    Wb = torch.empty_like(W)
    table = torch.tensor([[0, 0, N, K]], dtype=torch.int64, device=DEV)
    ops.block_table(W, Wb, table, 1)
    assert torch.equal(Wb.view(-1), W.view(N // 256, 256, K // 64, 64).permute(0, 2, 1, 3).contiguous().view(-1))
    bias, res = rnd(N, seed=33, dtype=F32), rnd(M, N, seed=34, dtype=F32)
    o0, o1 = torch.empty(M, N, device=DEV, dtype=F32), torch.empty(M, N, device=DEV, dtype=F32)
    c0, c1 = torch.empty(M, N, device=DEV, dtype=BF), torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, W, o0, bias=bias, res_f32=res, C2=c0, tile_cfg=256)
    ops.gemm_nt(A, Wb.view(N, K), o1, bias=bias, res_f32=res, C2=c1, tile_cfg=256, b_blocked=True)
    close(o1, A.float() @ W.float().t() + bias + res, 2e-3, 2e-3, "blocked weights")
    assert float((o0 - o1).abs().max()) < 1e-4 and float((c0.float() - c1.float()).abs().max()) < 2e-2


def test_gemm_nt_bit_stable_under_memory_pressure(ops):
    """The 4-phase loop's counted waits leave LDS-DMA half-tiles in flight across barriers; its ordering does not depend on how long a half-tile takes
    to land (tests/test_kloop_schedule_cpu.py), so the product must be bit-identical when the memory system is saturated by another stream -- 100 runs of
    a bench-shaped product (13.8 rounds of tiles, persistent lane) and of an f32-residual product against their quiet-machine results while a second
    stream streams 1.2 GB copies through HBM."""
    M, N, K = 256 * 393, 2304, 768
    A, B = rnd(M, K, seed=41), rnd(N, K, seed=42, scale=0.05)
    bias = rnd(N, seed=43, dtype=F32)
    res = rnd(M, 768, seed=44, dtype=F32)
    ref = torch.empty(M, N, device=DEV, dtype=BF)
    ref2 = torch.empty(M, 768, device=DEV, dtype=F32)
    ops.gemm_nt(A, B, ref, bias=bias)
    ops.gemm_nt(A, B[:768], ref2, bias=bias[:768], res_f32=res)
    torch.cuda.synchronize()
    src = torch.empty(300 * 1024 * 1024, device=DEV, dtype=torch.float32)
    dst = torch.empty_like(src)
    side = torch.cuda.Stream()
    out, out2 = torch.empty_like(ref), torch.empty_like(ref2)
    bad = 0
    for it in range(100):
        with torch.cuda.stream(side):
            dst.copy_(src, non_blocking=True)
            src.copy_(dst, non_blocking=True)
        ops.gemm_nt(A, B, out, bias=bias)
        ops.gemm_nt(A, B[:768], out2, bias=bias[:768], res_f32=res)
        if it % 10 == 9:
            torch.cuda.synchronize()
            bad += int(not torch.equal(out, ref)) + int(not torch.equal(out2, ref2))
    torch.cuda.synchronize()
    assert bad == 0


def test_gemm_nt_asymmetric_identity(ops):
    """A = I against an asymmetric B catches a transposed / permuted C write."""
    K = 128
    A = torch.eye(K, device=DEV, dtype=BF)
    B = (torch.arange(256 * K, device=DEV).reshape(256, K) % 97).float().to(BF)
    out = torch.empty(K, 256, device=DEV, dtype=F32)
    ops.gemm_nt(A, B, out)
    assert torch.equal(out, B.float().t())


@pytest.mark.parametrize("cfg", [128, 256])
def test_gemm_nt_epilogues(ops, cfg):
    M, N, K = 520, 768, 256
    A, B = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=0.06)
    bias, bias2 = rnd(N, seed=5, dtype=F32), rnd(N, seed=6, dtype=F32)
    res = rnd(M, N, seed=7, dtype=F32)
    resb = rnd(M, N, seed=8)
    z = rnd(M, N, seed=9)
    lin = A.float() @ B.float().t()
    # bias + erf-gelu with pre-activation save
    out, pre = torch.empty(M, N, device=DEV, dtype=BF), torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, B, out, bias=bias, act=ops.ACT_GELU, preact=pre, tile_cfg=cfg)
    close(pre, lin + bias, 3e-2, 1e-2, "preact")
    close(out, torch.nn.functional.gelu(lin + bias), 3e-2, 1e-2, "gelu")
    # bias + bias2 + quick gelu
    ops.gemm_nt(A, B, out, bias=bias, bias2=bias2, act=ops.ACT_QGELU, tile_cfg=cfg)
    y = lin + bias + bias2
    close(out, y * torch.sigmoid(1.702 * y), 3e-2, 1e-2, "quick_gelu")
    # bias + f32 residual -> f32 out + bf16 copy
    of, c2 = torch.empty(M, N, device=DEV, dtype=F32), torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, B, of, bias=bias, res_f32=res, C2=c2, tile_cfg=cfg)
    close(of, lin + bias + res, 2e-3, 2e-3, "res_f32")
    close(c2, lin + bias + res, 3e-2, 1e-2, "C2")
    # bf16 residual
    ops.gemm_nt(A, B, out, res_bf16=resb, tile_cfg=cfg)
    close(out, lin + resb.float(), 3e-2, 1e-2, "res_bf16")
    # multiply by act'(z)
    for act, fn in ((ops.ACT_GELU, torch.nn.functional.gelu), (ops.ACT_QGELU, lambda t: t * torch.sigmoid(1.702 * t))):
        zz = z.float().clone().requires_grad_(True)
        fn(zz).sum().backward()
        ops.gemm_nt(A, B, out, mulz=z, mul_act=act, tile_cfg=cfg)
        close(out, lin * zz.grad, 3e-2, 1e-2, f"mulz act {act}")


@pytest.mark.parametrize("M,N", [(256 * 300 + 17, 768), (128 * 530 + 5, 256)])
def test_gemm_nt_persistent_loop_and_general_fallback(ops, M, N):
    """More tiles than CU slots: the persistent fast kernels walk several tiles per workgroup (M tail rows in the last
    one); every epilogue family against torch, and the general-epilogue kernel (tile_cfg 2561) against the fast ones."""
    K = 128
    A, B = rnd(M, K, seed=11), rnd(N, K, seed=12, scale=0.06)
    lin = A.float() @ B.float().t()
    bias = rnd(N, seed=13, dtype=F32)
    res = rnd(M, N, seed=14, dtype=F32)
    z = rnd(M, N, seed=15)
    outb, outg = torch.empty(M, N, device=DEV, dtype=BF), torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, B, outb, bias=bias)                                   # light mask: persistent
    close(outb, lin + bias, 3e-2, 1e-2, "persistent bf16")
    ops.gemm_nt(A, B, outg, bias=bias, tile_cfg=2561)                    # general epilogue, same tile
    assert torch.equal(outb, outg)
    ops.gemm_nt(A, B, outb, mulz=z, mul_act=ops.ACT_QGELU)               # persistent, streamed operand
    zz = z.float()
    sg = torch.sigmoid(1.702 * zz)
    close(outb, lin * (sg * (1 + 1.702 * zz * (1 - sg))), 3e-2, 1e-2, "persistent mulz")
    of, c2 = torch.empty(M, N, device=DEV, dtype=F32), torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, B, of, bias=bias, res_f32=res, C2=c2)                 # residual-stream fast lane
    close(of, lin + bias + res, 2e-3, 2e-3, "res_f32 fast")
    close(c2, lin + bias + res, 3e-2, 1e-2, "C2 fast")
    og = torch.empty(M, N, device=DEV, dtype=F32)
    ops.gemm_nt(A, B, og, bias=bias, res_f32=res, tile_cfg=2561)
    assert torch.equal(of, og)
    pre = torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, B, outb, bias=bias, act=ops.ACT_QGELU, preact=pre)
    y = lin + bias
    close(pre, y, 3e-2, 1e-2, "preact fast")
    close(outb, y * torch.sigmoid(1.702 * y), 3e-2, 1e-2, "qgelu fast")


@pytest.mark.parametrize("cfg", [0, 128, 2561])
@pytest.mark.parametrize("act", ["gelu", "qgelu"])
def test_gemm_nt_stored_activation_derivative(ops, cfg, act):
    """preact_grad: the forward epilogue writes act'(z) next to act(z); mul_act=ACT_STORED multiplies by that buffer.
    Fast lanes (tile_cfg 0 / 128: tail rows in the last tile), the general epilogue (2561), and the activation-only
    forward used under no_grad; all against autograd of the same function."""
    M, N, K = 256 * 260 + 9, 768, 128
    A, B = rnd(M, K, seed=21), rnd(N, K, seed=22, scale=0.06)
    bias = rnd(N, seed=23, dtype=F32)
    kind, fn = ((ops.ACT_GELU, torch.nn.functional.gelu) if act == "gelu" else (ops.ACT_QGELU, lambda t: t * torch.sigmoid(1.702 * t)))
    y = (A.float() @ B.float().t() + bias).requires_grad_(True)
    a_ref = fn(y)
    a_ref.sum().backward()
    out, g = torch.empty(M, N, device=DEV, dtype=BF), torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, B, out, bias=bias, act=kind, preact=g, preact_grad=True, tile_cfg=cfg)
    close(out, a_ref.detach(), 3e-2, 1e-2, "act(z)")
    close(g, y.grad, 3e-2, 1e-2, "act'(z)")
    out2 = torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(A, B, out2, bias=bias, act=kind, tile_cfg=cfg)           # forward under no_grad: activation only
    assert torch.equal(out, out2)
    # backward product: dz = (dA @ W^T) * g
    dA, W = rnd(M, K, seed=24), rnd(N, K, seed=25, scale=0.06)
    dz = torch.empty(M, N, device=DEV, dtype=BF)
    ops.gemm_nt(dA, W, dz, mulz=g, mul_act=ops.ACT_STORED, tile_cfg=cfg)
    close(dz, (dA.float() @ W.float().t()) * g.float(), 3e-2, 1e-2, "stored derivative product")
    with pytest.raises(RuntimeError):
        ops.gemm_nt(A, B, out, bias=bias, preact=g, preact_grad=True)      # no activation


def test_gemm_nt_dual_k_gather_batch(ops):
    M, N, K = 300, 512, 128
    A, B, A2, B2 = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=.1), rnd(M, K, seed=3), rnd(N, K, seed=4, scale=.1)
    out = torch.empty(M, N, device=DEV, dtype=F32)
    ops.gemm_nt(A, B, out, A2=A2, B2=B2)
    close(out, A.float() @ B.float().t() + A2.float() @ B2.float().t(), 2e-3, 2e-3, "dual-K")
    # gathers: rows of A and B picked by index, bias picked by the B row index
    g = torch.Generator().manual_seed(0)
    ar = torch.randint(0, M, (77,), generator=g).to(DEV).int()
    br = torch.randperm(N, generator=g)[:203].to(DEV).int()
    bias = rnd(N, seed=5, dtype=F32)
    og = torch.empty(77, 203, device=DEV, dtype=F32)
    ops.gemm_nt(A, B, og, a_rows=ar, b_rows=br, bias=bias, bias_by_brow=True)
    close(og, A.float()[ar.long()] @ B.float()[br.long()].t() + bias[br.long()], 2e-3, 2e-3, "gather")
    # batched with strides
    Bz, m, n = 5, 64, 393
    Ab, Bb = rnd(Bz, m, K, seed=6), rnd(Bz, n, K, seed=7, scale=.1)
    ob = torch.empty(Bz, m, 400, device=DEV, dtype=F32)
    ops.gemm_nt(Ab[0], Bb[0], ob[0], N=n, batch=Bz, stride_a=m * K, stride_b=n * K, stride_c=m * 400)
    close(ob[:, :, :n], torch.einsum("bmk,bnk->bmn", Ab.float(), Bb.float()), 2e-3, 2e-3, "batched")


# ----------------------------------------------------------------------------------------- TN GEMM
@pytest.mark.parametrize("M,NX,NY", [(256, 256, 256), (1000, 768, 768), (3144, 2304, 768), (3144, 768, 3072), (77, 300, 768)])
def test_gemm_tn(ops, M, NX, NY):
    ldx = ((NX + 7) // 8) * 8
    X = torch.zeros(M, ldx, device=DEV, dtype=BF)
    X[:, :NX] = rnd(M, NX, seed=1, scale=0.1)
    Y = rnd(M, NY, seed=2)
    out = torch.zeros(NX, NY, device=DEV, dtype=F32)
    cs = torch.zeros(NX, device=DEV, dtype=F32)
    ops.gemm_tn(X, Y, out, NX=NX, colsum=cs)
    ref = X[:, :NX].float().t() @ Y.float()
    close(out, ref, 5e-3 * math.sqrt(M / 256), 2e-3, "gemm_tn")
    close(cs, X[:, :NX].float().sum(0), 5e-3 * math.sqrt(M / 256), 2e-3, "colsum")
    # accumulation semantic: second call doubles
    ops.gemm_tn(X, Y, out, NX=NX)
    close(out, 2 * ref, 1e-2 * math.sqrt(M / 256), 2e-3, "gemm_tn accumulate")


def test_gemm_tn_scatter_and_batch(ops):
    M, NX, NY, V = 200, 203, 768, 1000
    X = torch.zeros(M, 208, device=DEV, dtype=BF)
    X[:, :NX] = rnd(M, NX, seed=1, scale=.1)
    Y = rnd(M, NY, seed=2)
    rows = torch.randperm(V)[:NX].to(DEV).int()
    out = torch.zeros(V, NY, device=DEV, dtype=F32)
    cs = torch.zeros(V, device=DEV, dtype=F32)
    ops.gemm_tn(X, Y, out, NX=NX, out_rows=rows, colsum=cs, colsum_by_row=True)
    ref = torch.zeros_like(out)
    ref[rows.long()] = X[:, :NX].float().t() @ Y.float()
    close(out, ref, 5e-3, 2e-3, "tn scatter")
    rc = torch.zeros_like(cs)
    rc[rows.long()] = X[:, :NX].float().sum(0)
    close(cs, rc, 5e-3, 2e-3, "tn scatter colsum")
    Bz, m, nx = 4, 64, 393
    Xb = torch.zeros(Bz, m, 448, device=DEV, dtype=BF)
    Xb[:, :, :nx] = rnd(Bz, m, nx, seed=3, scale=.1)
    Yb = rnd(Bz, m, 768, seed=4)
    ob = torch.zeros(Bz, nx, 768, device=DEV, dtype=F32)
    ops.gemm_tn(Xb[0], Yb[0], ob[0], NX=nx, batch=Bz, stride_x=m * 448, stride_y=m * 768, stride_o=nx * 768)
    close(ob, torch.einsum("bmx,bmy->bxy", Xb[:, :, :nx].float(), Yb.float()), 5e-3, 2e-3, "tn batched")


# ----------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("eps", [1e-5, 1e-12])
def test_layernorm_fwd_bwd(ops, eps):
    M, H = 1001, 768
    x = rnd(M, H, seed=1, dtype=F32, scale=2.0) + 0.3
    gamma, beta = 1 + 0.1 * rnd(H, seed=2, dtype=F32), 0.1 * rnd(H, seed=3, dtype=F32)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    of, ob = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV, dtype=BF)
    ops.ln_fwd(x_f32=x, gamma=gamma, beta=beta, eps=eps, M=M, H=H, mean=mean, rstd=rstd, out_f32=of, out_bf16=ob)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (H,), gr, br, eps)
    close(of, ref, 2e-5, 2e-5, "ln fwd f32")
    close(ob, ref, 2e-2, 1e-2, "ln fwd bf16")
    dy = rnd(M, H, seed=4, dtype=F32)
    dyb = rnd(M, H, seed=5)
    add = rnd(M, H, seed=6, dtype=F32)
    ref.backward(dy + dyb.float())
    ds, dsb = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV, dtype=BF)
    dg, db = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    ops.ln_bwd(dy_f32=dy, dy_bf16=dyb, s=x, mean=mean, rstd=rstd, gamma=gamma, M=M, H=H, add_f32=add, ds_f32=ds, ds_bf16=dsb,
               dgamma=dg, dbeta=db)
    close(ds, xr.grad + add, 1e-4, 1e-4, "ln bwd dx")
    close(dsb, xr.grad, 2e-2, 1e-2, "ln bwd dx bf16 (no add)")
    close(dg, gr.grad, 2e-3, 1e-4, "ln dgamma")
    close(db, br.grad, 2e-3, 1e-4, "ln dbeta")


@pytest.mark.parametrize("M", [4096, 4099, 33333])
def test_layernorm_vision_stream_shapes(ops, M):
    """The two operand sets of the vision stream take the straight-line, software-pipelined kernels (ln_fwd_fast_k: x f32 -> bf16;
    ln_bwd_fast_k: dy bf16 + x + residual gradient -> f32 total + bf16 copy, dgamma / dbeta through the workspace) from 4096 rows up.
    Ragged row counts exercise the clamped duplicate rows of the last round; compared with torch's fp32 layer_norm and with the general
    kernels (MART_LN_FAST is read once per process, so the general path is reached through an operand set it does not take)."""
    H, eps = 768, 1e-5
    x = rnd(M, H, seed=11, dtype=F32, scale=2.0) + 0.3
    gamma, beta = 1 + 0.1 * rnd(H, seed=12, dtype=F32), 0.1 * rnd(H, seed=13, dtype=F32)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ob = torch.empty(M, H, device=DEV, dtype=BF)
    ops.ln_fwd(x_f32=x, gamma=gamma, beta=beta, eps=eps, M=M, H=H, mean=mean, rstd=rstd, out_bf16=ob)                    # fast
    mean2, rstd2 = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    of2, ob2 = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV, dtype=BF)
    ops.ln_fwd(x_f32=x, gamma=gamma, beta=beta, eps=eps, M=M, H=H, mean=mean2, rstd=rstd2, out_f32=of2, out_bf16=ob2)   # general (f32 output as well)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (H,), gr, br, eps)
    close(ob, ref, 2e-2, 1e-2, "fast ln fwd bf16")
    close(ob, ob2, 1e-2, 4e-3, "fast vs general forward (the statistics are summed with 1/H folded in: last-ulp differences before the bf16 rounding)")
    close(mean, mean2, 1e-6, 1e-6, "row means"); close(rstd, rstd2, 1e-6, 1e-5, "row rstd")
    dyb = rnd(M, H, seed=15)
    add = rnd(M, H, seed=16, dtype=F32)
    ref.backward(dyb.float())
    ds, dsb = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV, dtype=BF)
    dg, db = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    ops.ln_bwd(dy_bf16=dyb, s=x, mean=mean, rstd=rstd, gamma=gamma, M=M, H=H, add_f32=add, ds_f32=ds, ds_bf16=dsb, bf16_total=True, dgamma=dg, dbeta=db)   # fast
    close(ds, xr.grad + add, 1e-4, 1e-4, "fast ln bwd dx + add")
    close(dsb, xr.grad + add, 2e-2, 1e-2, "fast ln bwd bf16 total")
    close(dg, gr.grad, 2e-3, 1e-3, "fast ln dgamma")
    close(db, br.grad, 2e-3, 1e-3, "fast ln dbeta")
    ds2, dg2, db2 = torch.empty(M, H, device=DEV), torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    ops.ln_bwd(dy_bf16=dyb, s=x, mean=mean, rstd=rstd, gamma=gamma, M=M, H=H, add_f32=add, ds_f32=ds2, dgamma=dg2, dbeta=db2)                            # general (no bf16 copy)
    close(ds, ds2, 1e-5, 1e-5, "fast vs general backward")
    close(dg, dg2, 1e-5, 1e-4, "dgamma fast vs general"); close(db, db2, 1e-5, 1e-4, "dbeta fast vs general")
    dg3, db3, ds3, dsb3 = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV), torch.empty_like(ds), torch.empty_like(dsb)
    ops.ln_bwd(dy_bf16=dyb, s=x, mean=mean, rstd=rstd, gamma=gamma, M=M, H=H, add_f32=add, ds_f32=ds3, ds_bf16=dsb3, bf16_total=True, dgamma=dg3, dbeta=db3)
    assert torch.equal(dg, dg3) and torch.equal(db, db3) and torch.equal(ds, ds3) and torch.equal(dsb, dsb3), "run-to-run"
    # round 6: the residual GRADIENT stream in bf16 -- bf16 residual operand in, bf16 total out, no f32 tensor (ln_bwd_fast_k<., ., GB16>); == the f32-stream
    # kernel fed the same (bf16-valued) residual operand, bit for bit, and the general kernel takes the operand too (small M / an f32 output requested)
    addb = add.to(BF)
    dsb4, dg4, db4 = torch.empty_like(dsb), torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    ops.ln_bwd(dy_bf16=dyb, s=x, mean=mean, rstd=rstd, gamma=gamma, M=M, H=H, add_bf16=addb, ds_bf16=dsb4, bf16_total=True, dgamma=dg4, dbeta=db4)
    ds5, dsb5, dg5, db5 = torch.empty_like(ds), torch.empty_like(dsb), torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    ops.ln_bwd(dy_bf16=dyb, s=x, mean=mean, rstd=rstd, gamma=gamma, M=M, H=H, add_f32=addb.float(), ds_f32=ds5, ds_bf16=dsb5, bf16_total=True, dgamma=dg5, dbeta=db5)
    # (the bf16-stream kernel owns 8 consecutive columns per lane -- 16-byte accesses -- so its row sums are taken in another order: the totals agree to a
    # rounding of the bf16 result, the column sums bit for bit where the order is the same)
    close(dsb4, dsb5, 2e-2, 1e-2, "bf16 gradient stream vs the f32-stream kernel on the same operands")
    assert float((dsb4.float() - dsb5.float()).abs().max()) <= 2.0 ** -6 * float(dsb5.float().abs().max())
    close(dg4, dg5, 1e-4, 1e-4, "dgamma, bf16 stream"); close(db4, db5, 1e-4, 1e-4, "dbeta, bf16 stream")
    dsb7, dg7, db7 = torch.empty_like(dsb), torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    ops.ln_bwd(dy_bf16=dyb, s=x, mean=mean, rstd=rstd, gamma=gamma, M=M, H=H, add_bf16=addb, ds_bf16=dsb7, bf16_total=True, dgamma=dg7, dbeta=db7)
    assert torch.equal(dsb4, dsb7) and torch.equal(dg4, dg7) and torch.equal(db4, db7), "run-to-run"
    close(dsb4, xr.grad + addb.float(), 2e-2, 1e-2, "bf16 gradient stream: total")
    ds6, dg6, db6 = torch.empty_like(ds), torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    ops.ln_bwd(dy_bf16=dyb, s=x, mean=mean, rstd=rstd, gamma=gamma, M=M, H=H, add_bf16=addb, ds_f32=ds6, dgamma=dg6, dbeta=db6)       # general kernel
    close(ds6, ds5, 1e-5, 1e-5, "general kernel with a bf16 residual operand")


def test_layernorm_reversed_sweep_knob():
    """MART_LN_REV=3 (last row first in both straight-line LayerNorm kernels; read once per process, hence the child process): the
    ragged-shape test above passes unchanged -- rows, statistics and the clamped duplicate rows map back to the same addresses."""
    import os, subprocess, sys
    if os.environ.get("MART_LN_REV"):
        pytest.skip("already running under the knob")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", "test_layernorm_vision_stream_shapes"],
                       env=dict(os.environ, MART_LN_REV="3"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_dropout_add_layernorm(ops):
    M, H, p, seed = 300, 768, 0.1, 1234567
    res = rnd(M, H, seed=1, dtype=F32)
    y = rnd(M, H, seed=2)
    gamma, beta = 1 + 0.1 * rnd(H, seed=3, dtype=F32), 0.1 * rnd(H, seed=4, dtype=F32)
    keep = torch.empty(M * H, device=DEV, dtype=torch.uint8)
    ops.dropout_mask(keep, p, seed)
    keep = keep.view(M, H).float()
    frac = float(keep.mean())
    assert abs(frac - (1 - p)) < 0.01, frac
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    s, of = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV)
    ops.ln_fwd(x_f32=res, y_bf16=y, p_drop=p, seed=seed, gamma=gamma, beta=beta, eps=1e-12, M=M, H=H, mean=mean, rstd=rstd, s_out=s, out_f32=of)
    sref = res + y.float() * keep / (1 - p)
    close(s, sref, 1e-5, 1e-5, "dropout+res sum")
    close(of, torch.nn.functional.layer_norm(sref, (H,), gamma, beta, 1e-12), 3e-5, 3e-5, "dropout+res LN")
    # backward: masked bf16 branch gradient
    dy = rnd(M, H, seed=5, dtype=F32)
    sr = sref.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(sr, (H,), gamma, beta, 1e-12).backward(dy)
    ds, dsb = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV, dtype=BF)
    ops.ln_bwd(dy_f32=dy, s=s, mean=mean, rstd=rstd, gamma=gamma, M=M, H=H, ds_f32=ds, ds_bf16=dsb, p_drop=p, seed=seed)
    close(ds, sr.grad, 1e-4, 1e-4, "ds")
    close(dsb, sr.grad * keep / (1 - p), 2e-2, 1e-2, "masked branch grad")


# ----------------------------------------------------------------------------------------- attention
def _attn_ref(q, k, v, scale, factor=None, maskadd=None, keep=None, p=0.0):
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if factor is not None:
        s = s * factor
    if maskadd is not None:
        s = s + maskadd
    a = torch.softmax(s, -1)
    if keep is not None:
        a = a * keep / (1 - p)
    return torch.einsum("bhqk,bhkd->bhqd", a, v)


def _heads(x, B, S, nh):          # [B*S, nh*64] -> [B,nh,S,64]
    return x.view(B, S, nh, 64).permute(0, 2, 1, 3)


@pytest.mark.parametrize("B,nh,S,Lp", [(2, 12, 99, 0), (2, 12, 393, 64), (3, 4, 130, 24), (1, 2, 64, 0), (2, 3, 300, 0), (1, 2, 257, 64), (3, 12, 100, 0), (2, 2, 128, 0), (2, 2, 33, 0),
                                        # round 5: the peeled last key tile runs ONE 32-key block when it holds <= 32 keys (key counts 1 / 31 / 32 / 33 past a multiple
                                        # of 64, with and without a prefix), and the fused backward's dQ pipeline is compiled for 14 or 16 chunks of 32 keys
                                        (1, 2, 65, 0), (1, 2, 95, 0), (1, 2, 96, 0), (1, 2, 97, 0), (2, 2, 129, 32), (2, 2, 128, 32), (1, 2, 393, 0),
                                        (1, 2, 448, 0), (1, 1, 449, 0), (1, 2, 448, 64), (1, 2, 416, 32),
                                        (1, 2, 130, 20),        # a prefix that is no multiple of 8: per-lane K staging in the fused backward
                                        # round 6: prefix lengths real MARS batches have (L = longest example of the batch): ONE 32-row half of the key stream
                                        # straddles the prefix / own boundary in the vision forward kernel (first / second half of a tile, short and long prefixes)
                                        (2, 12, 393, 57), (2, 3, 393, 37), (1, 2, 200, 101), (2, 2, 99, 5), (1, 2, 393, 96), (2, 2, 260, 33), (1, 3, 150, 63)])
def test_attention_vision(ops, B, nh, S, Lp):
    H = nh * 64
    qkv = rnd(B * S, 3 * H, seed=1, scale=1.0)
    tqkv = rnd(B * max(Lp, 1), 3 * H, seed=2, scale=1.0)
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    pk, pv = (tqkv[:, H:2 * H], tqkv[:, 2 * H:]) if Lp else (None, None)
    ctx = torch.zeros(B * S, H, device=DEV, dtype=BF)
    lse = torch.empty(B, nh, S, device=DEV)
    kw = dict(q=q, k=k, v=v, ctx=ctx, lse=lse, B=B, nh=nh, Sq=S, Sk=S, scale=0.125, pk=pk, pv=pv, Lp=Lp)
    ops.attn_fwd(**kw)
    qr, kr, vr = [t.float().clone().requires_grad_(True) for t in (q, k, v)]
    kk, vv = _heads(kr, B, S, nh), _heads(vr, B, S, nh)
    if Lp:
        pkr, pvr = [t.float().clone().requires_grad_(True) for t in (pk, pv)]
        kk = torch.cat([_heads(pkr, B, Lp, nh), kk], 2)
        vv = torch.cat([_heads(pvr, B, Lp, nh), vv], 2)
    o = _attn_ref(_heads(qr, B, S, nh), kk, vv, 0.125)
    oref = o.permute(0, 2, 1, 3).reshape(B * S, H)
    close(ctx, oref, 2e-2, 2e-2, "attn fwd")
    s = torch.einsum("bhqd,bhkd->bhqk", _heads(qr, B, S, nh), kk) * 0.125
    close(lse * math.log(2.0), torch.logsumexp(s, -1), 2e-3, 1e-3, "lse (saved in the log2 domain)")
    # backward
    dctx = rnd(B * S, H, seed=3)
    oref.backward(dctx.float())
    dqkv = torch.zeros(B * S, 3 * H, device=DEV, dtype=BF)
    dt = torch.zeros(B * max(Lp, 1), 3 * H, device=DEV, dtype=BF)
    delta = torch.empty(B, nh, S, device=DEV)
    ops.attn_bwd(dctx=dctx, delta=delta, dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:],
                 dpk=dt[:, H:2 * H] if Lp else None, dpv=dt[:, 2 * H:] if Lp else None, **kw)
    gs = float(qr.grad.abs().max())
    close(dqkv[:, :H], qr.grad, 2e-2 * max(gs, 1), 3e-2, "dq")
    close(dqkv[:, H:2 * H], kr.grad, 2e-2 * max(float(kr.grad.abs().max()), 1), 3e-2, "dk")
    close(dqkv[:, 2 * H:], vr.grad, 2e-2 * max(float(vr.grad.abs().max()), 1), 3e-2, "dv")
    if Lp:
        close(dt[:, H:2 * H], pkr.grad, 2e-2 * max(float(pkr.grad.abs().max()), 1), 3e-2, "dpk")
        close(dt[:, 2 * H:], pvr.grad, 2e-2 * max(float(pvr.grad.abs().max()), 1), 3e-2, "dpv")


def test_attention_rescale_branch(ops):
    """Online softmax with a deferred rescale: spike some keys in LATE tiles so the running maximum jumps by far more
    than the 2^8 threshold after probabilities were already accumulated (the branch is rare on random data)."""
    B, nh, S, H = 2, 4, 393, 256
    qkv = rnd(B * S, 3 * H, seed=1, scale=1.0)
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    kk = k.clone().view(B, S, H)
    qq = q.view(B, S, H)
    kk[0, 300] = (qq[0, 5].float() * 3.0).to(BF)         # row 5 of batch 0: score ~ 3|q|^2/8 at key 300 (tile 4)
    kk[1, 200] = (qq[1, 100].float() * 2.0).to(BF)       # another wave / tile
    kk[1, 390] = (qq[1, 101].float() * 4.0).to(BF)       # last (partial) tile
    k = kk.view(B * S, H)
    ctx = torch.zeros(B * S, H, device=DEV, dtype=BF)
    lse = torch.empty(B, nh, S, device=DEV)
    kw = dict(q=q, k=k, v=v, ctx=ctx, lse=lse, B=B, nh=nh, Sq=S, Sk=S, scale=0.125)
    ops.attn_fwd(**kw)
    qr, kr, vr = [t.float().clone().requires_grad_(True) for t in (q, k, v)]
    o = _attn_ref(_heads(qr, B, S, nh), _heads(kr, B, S, nh), _heads(vr, B, S, nh), 0.125)
    oref = o.permute(0, 2, 1, 3).reshape(B * S, H)
    close(ctx, oref, 2e-2, 2e-2, "attn fwd with forced rescale")
    s = torch.einsum("bhqd,bhkd->bhqk", _heads(qr, B, S, nh), _heads(kr, B, S, nh)) * 0.125
    assert float(s.max()) > 20.0
    close(lse * math.log(2.0), torch.logsumexp(s, -1), 2e-3, 1e-3, "lse with forced rescale")
    dctx = rnd(B * S, H, seed=3)
    oref.backward(dctx.float())
    dqkv = torch.zeros(B * S, 3 * H, device=DEV, dtype=BF)
    delta = torch.empty(B, nh, S, device=DEV)
    ops.attn_bwd(dctx=dctx, delta=delta, dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:], **kw)
    close(dqkv[:, :H], qr.grad, 2e-2 * max(float(qr.grad.abs().max()), 1), 3e-2, "dq (spiked)")
    close(dqkv[:, H:2 * H], kr.grad, 2e-2 * max(float(kr.grad.abs().max()), 1), 3e-2, "dk (spiked)")
    close(dqkv[:, 2 * H:], vr.grad, 2e-2 * max(float(vr.grad.abs().max()), 1), 3e-2, "dv (spiked)")


@pytest.mark.parametrize("B,nh,L,p", [(3, 12, 64, 0.0), (2, 12, 64, 0.1), (2, 4, 24, 0.0), (2, 2, 96, 0.1), (2, 4, 23, 0.1), (2, 3, 40, 0.1), (2, 2, 128, 0.1), (2, 3, 101, 0.1), (1, 2, 80, 0.0), (2, 2, 160, 0.1)])
def test_attention_text(ops, B, nh, L, p):
    H = nh * 64
    seed = 99
    qkv = rnd(B * L, 3 * H, seed=1, scale=1.0)
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    am = torch.ones(B, L, dtype=torch.long)
    am[0, L - 7:] = 0
    if B > 1:
        am[1, L - 2:] = 0
    am = am.to(DEV)
    sep = torch.zeros(B, 6, dtype=torch.long)
    sep[:, 2] = torch.tensor([L // 3 + i for i in range(B)])
    sep = sep.to(DEV)
    w0 = torch.tensor([0.25], device=DEV)
    w1 = torch.tensor([0.5], device=DEV)          # exactly on the clamp bound: gradient must pass
    ctx = torch.zeros(B * L, H, device=DEV, dtype=BF)
    lse = torch.empty(B, nh, L, device=DEV)
    kw = dict(q=q, k=k, v=v, ctx=ctx, lse=lse, B=B, nh=nh, Sq=L, Sk=L, scale=0.125, attn_mask=am, sep=sep[:, 2:], sep_stride=6,
              w0=w0, w1=w1, p_drop=p, seed=seed)
    ops.attn_fwd(**kw)
    keep = None
    if p > 0:
        keep = torch.empty(B * nh * L * L, device=DEV, dtype=torch.uint8)
        ops.dropout_mask(keep, p, seed)
        keep = keep.view(B, nh, L, L).float()
    qr, kr, vr = [t.float().clone().requires_grad_(True) for t in (q, k, v)]
    w0r, w1r = w0.clone().requires_grad_(True), w1.clone().requires_grad_(True)
    ar = torch.arange(L, device=DEV)
    s = sep[:, 2][:, None]
    col_hi = (ar[None] >= s)[:, None, :]
    row_lo = (ar[None] < s)[:, :, None]
    fac = torch.where(col_hi, torch.where(row_lo, torch.clamp(w0r, 0, .5), torch.clamp(w1r, .5, 1)), torch.ones((), device=DEV))[:, None]
    maskadd = ((1 - am) * -10000.0)[:, None, None, :].float()
    o = _attn_ref(_heads(qr, B, L, nh), _heads(kr, B, L, nh), _heads(vr, B, L, nh), 0.125, fac, maskadd, keep, p)
    oref = o.permute(0, 2, 1, 3).reshape(B * L, H)
    close(ctx, oref, 2e-2, 2e-2, "text attn fwd")
    dctx = rnd(B * L, H, seed=3)
    oref.backward(dctx.float())
    dqkv = torch.zeros(B * L, 3 * H, device=DEV, dtype=BF)
    pre = rnd(B * L, 3 * H, seed=4)                # pre-existing prefix grads in the k/v blocks (accum_dkv)
    dqkv[:, H:] = pre[:, H:]
    delta = torch.empty(B, nh, L, device=DEV)
    dw = torch.zeros(2, device=DEV)
    ops.attn_bwd(dctx=dctx, delta=delta, dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:], accum_dkv=True, dw=dw, **kw)
    close(dqkv[:, :H], qr.grad, 2e-2 * max(float(qr.grad.abs().max()), 1), 3e-2, "text dq")
    close(dqkv[:, H:2 * H], kr.grad + pre[:, H:2 * H].float(), 3e-2 * max(float(kr.grad.abs().max()), 1), 3e-2, "text dk (+accum)")
    close(dqkv[:, 2 * H:], vr.grad + pre[:, 2 * H:].float(), 3e-2 * max(float(vr.grad.abs().max()), 1), 3e-2, "text dv (+accum)")
    gw = torch.stack([w0r.grad[0], w1r.grad[0]])
    close(dw, gw, 2e-2 * max(float(gw.abs().max()), 1), 3e-2, "d adaptive_weight")


# ----------------------------------------------------------------------------------------- small kernels
def test_softmax_transpose(ops):
    R, Cc, ldp = 130, 393, 448
    sc = rnd(R, 400, seed=1, dtype=F32, scale=3.0)
    pr = torch.full((R, ldp), 7.0, device=DEV, dtype=BF)
    ops.softmax_fwd(sc[:, :Cc], pr, R, Cc)
    ref = torch.softmax(sc[:, :Cc], -1)
    close(pr[:, :Cc], ref, 4e-3, 1e-2, "softmax")
    assert float(pr[:, Cc:].abs().max()) == 0
    dp = rnd(R, 400, seed=2, dtype=F32)
    dsb = torch.full((R, ldp), 7.0, device=DEV, dtype=BF)
    ops.softmax_bwd(pr, dp[:, :Cc], dsb, R, Cc)
    pf = pr[:, :Cc].float()
    close(dsb[:, :Cc], pf * (dp[:, :Cc] - (pf * dp[:, :Cc]).sum(-1, keepdim=True)), 4e-3, 2e-2, "softmax bwd")
    assert float(dsb[:, Cc:].abs().max()) == 0
    x = rnd(3, 393, 768, seed=3)
    xt = torch.full((3, 768, 448), 5.0, device=DEV, dtype=BF)
    ops.transpose_bf16(x[0], xt[0], 393, 768, 448, batch=3, stride_i=393 * 768, stride_o=768 * 448)
    assert torch.equal(xt[:, :, :393], x.transpose(1, 2)) and float(xt[:, :, 393:].abs().max()) == 0
    # unaligned shapes / leading dimensions (scalar fall-back paths of the 16-byte transpose) and an unpadded destination
    for (R2, C2, ld2, Rp2) in ((37, 53, 61, 37), (64, 64, 64, 64), (65, 129, 136, 72), (393, 768, 2304, 393)):
        src = rnd(R2, ld2, seed=R2 + C2)
        dst = torch.full((C2, Rp2), 5.0, device=DEV, dtype=BF)
        ops.transpose_bf16(src[:, :C2], dst, R2, C2, Rp2)
        assert torch.equal(dst[:, :R2], src[:, :C2].t()), (R2, C2, ld2, Rp2)
        if Rp2 > R2:
            assert float(dst[:, R2:].abs().max()) == 0
    # table form: several matrices of one flat buffer in one launch (the per-step refresh of the transposed weight copies)
    shapes = [(768, 2304), (3072, 768), (40, 24), (100, 8)]
    offs, tot = [], 0
    for (r, c) in shapes:
        offs.append(tot); tot += r * c
    flat = rnd(tot, seed=77)
    flat_t = torch.zeros(tot, device=DEV, dtype=BF)
    table = torch.tensor([[o, o, r, c] for o, (r, c) in zip(offs, shapes)], dtype=torch.int64, device=DEV)
    ops.transpose_table(flat, flat_t, table, len(shapes))
    for o, (r, c) in zip(offs, shapes):
        assert torch.equal(flat_t[o:o + r * c].view(c, r), flat[o:o + r * c].view(r, c).t()), (r, c)


def test_embeddings(ops):
    B, S, p, H = 3, 224, 16, 768
    g = S // p
    P = g * g
    pix = rnd(B, 2, 3, S, S, seed=1, dtype=F32)
    pm = torch.empty(B * 2 * P, 3 * p * p, device=DEV, dtype=BF)
    ops.patchify(pix, pm, B, S, p)
    ref = pix.view(B * 2, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * 2 * P, 3 * p * p)
    close(pm, ref, 1e-2, 1e-2, "patchify")
    w = rnd(H, 3 * p * p, seed=2, scale=0.02)
    pe = torch.empty(B * 2 * P, H, device=DEV, dtype=BF)
    ops.gemm_nt(pm, w, pe)
    conv = torch.nn.functional.conv2d(pix.view(B * 2, 3, S, S).to(BF).float(), w.float().view(H, 3, p, p), stride=p)
    close(pe, conv.flatten(2).transpose(1, 2).reshape(B * 2 * P, H), 2e-2, 2e-2, "patch conv as GEMM")
    cls, pos = rnd(H, seed=3, dtype=F32), rnd(P + 1, H, seed=4, dtype=F32)
    s = torch.empty(B, 1 + 2 * P, H, device=DEV)
    ops.vision_assemble(pe, cls, pos, s, B, P, H)
    pev = pe.float().view(B, 2 * P, H)
    sref = torch.cat([cls.expand(B, 1, H), pev], 1) + torch.cat([pos, pos[1:]], 0)[None]
    close(s, sref, 1e-5, 1e-5, "assemble")
    ds = rnd(B, 1 + 2 * P, H, seed=5, dtype=F32)
    dpe = torch.empty(B * 2 * P, H, device=DEV, dtype=BF)
    dcls, dpos = torch.zeros(H, device=DEV), torch.zeros(P + 1, H, device=DEV)
    ops.vision_assemble_bwd(ds, dpe, dcls, dpos, B, P, H)
    close(dpe, ds[:, 1:].reshape(B * 2 * P, H), 2e-2, 1e-2, "dpatch")
    close(dcls, ds[:, 0].sum(0), 1e-4, 1e-5, "dcls")
    rp = torch.zeros_like(dpos)
    rp[0] = ds[:, 0].sum(0)
    rp[1:] = ds[:, 1:P + 1].sum(0) + ds[:, P + 1:].sum(0)
    close(dpos, rp, 1e-4, 1e-5, "dpos")
    # text
    V, L = 500, 64
    ids = torch.randint(0, V, (B, L)).to(DEV)
    tt = torch.randint(0, 2, (B, L)).to(DEV)
    word, posw, typ = rnd(V, H, seed=6, dtype=F32), rnd(512, H, seed=7, dtype=F32), rnd(2, H, seed=8, dtype=F32)
    gamma, beta = 1 + .1 * rnd(H, seed=9, dtype=F32), .1 * rnd(H, seed=10, dtype=F32)
    so, mean, rstd = torch.empty(B * L, H, device=DEV), torch.empty(B * L, device=DEV), torch.empty(B * L, device=DEV)
    of, ob = torch.empty(B * L, H, device=DEV), torch.empty(B * L, H, device=DEV, dtype=BF)
    ops.text_embed_fwd(ids=ids, tt=tt, word=word, pos=posw, type_=typ, gamma=gamma, beta=beta, eps=1e-12, p_drop=0.0, seed=1, B=B, Lq=L, H=H,
                       s_out=so, mean=mean, rstd=rstd, out_f32=of, out_bf16=ob)
    sr = word[ids] + typ[tt] + posw[:L][None]
    close(so, sr.view(B * L, H), 1e-5, 1e-5, "text embed sum")
    close(of, torch.nn.functional.layer_norm(sr, (H,), gamma, beta, 1e-12).view(B * L, H), 3e-5, 3e-5, "text embed LN")
    ds2 = rnd(B * L, H, seed=11, dtype=F32)
    dw, dp, dty = torch.zeros_like(word), torch.zeros_like(posw), torch.zeros_like(typ)
    ops.text_embed_scatter(ds2, ids, tt, dw, dp, dty, B, L, H)
    rw = torch.zeros_like(word).index_add_(0, ids.view(-1), ds2)
    close(dw, rw, 1e-4, 1e-5, "dword")
    close(dp[:L], ds2.view(B, L, H).sum(0), 1e-4, 1e-5, "dpos")
    close(dty, torch.zeros_like(typ).index_add_(0, tt.view(-1), ds2), 1e-3, 1e-5, "dtype")


def test_lsce_ignored_labels(ops, golden_dir):
    """LabelSmoothSoftmaxCEV1 through the C ABI with ignore_index rows (reference golden G3b, lit_models/utils.py:47-62): 'mean' divides by
    n_valid, ignored rows get loss 0 and a zero gradient row; 'sum' / per-row; a label outside [0, C) that is not ignore_index poisons the
    row (NaN), sets the status word and reads nothing out of bounds; every row ignored -> 0 / 0 = NaN as the reference."""
    import os
    from mkg_analogy_amd import functional as Fn
    from mkg_analogy_amd.lit_models.utils import LabelSmoothSoftmaxCEV1
    g = np.load(os.path.join(golden_dir, "g3b_lsce_ignore.npz"))
    label = torch.from_numpy(g["label"]).to(DEV)
    w = torch.from_numpy(g["none_weights"]).to(DEV)
    for red in ("mean", "sum", "none"):
        lg = torch.from_numpy(g["logits"]).to(DEV).requires_grad_(True)
        loss = LabelSmoothSoftmaxCEV1(lb_smooth=0.1, reduction=red, ignore_index=int(g["ignore_index"]))(lg, label)
        np.testing.assert_allclose(loss.detach().cpu().numpy(), g["loss_" + red], rtol=2e-6, atol=2e-5)
        (loss if red != "none" else (loss * w).sum()).backward()
        close(lg.grad, torch.from_numpy(g["grad_" + red]).to(DEV), 1e-6, 1e-4, f"lsce grad, ignored rows, reduction {red}")
        assert float(lg.grad[[1, 4]].abs().max()) == 0.0
    Fn.check_labels()                                              # nothing out of range so far
    lg = torch.from_numpy(g["logits"]).to(DEV)
    assert torch.isnan(LabelSmoothSoftmaxCEV1(0.1)(lg, torch.full((6,), -100, device=DEV, dtype=torch.long)))
    # the raw ABI with the bf16 output as the engine uses it: ignored rows zero, padding zero
    R, Cc = lg.shape
    rows, lse, red2 = torch.empty(R, device=DEV), torch.empty(R, device=DEV), torch.empty(2, device=DEV)
    ops.lsce_fwd(lg, label, 0.1, rows, lse, ignore_index=-100, loss_out=red2, reduction="mean")
    assert float(red2[1]) == 4.0 and float(rows[1]) == 0.0 and float(rows[4]) == 0.0
    dlb = torch.full((R, 64), 3.0, device=DEV, dtype=BF)
    ops.lsce_bwd(lg, label, lse, 0.1, torch.ones(1, device=DEV), 1.0, dl_bf16=dlb, ignore_index=-100, n_valid=red2[1:])
    assert float(dlb[:, Cc:].abs().max()) == 0 and float(dlb[[1, 4]].abs().max()) == 0
    close(dlb[:, :Cc].float(), torch.from_numpy(g["grad_mean"]).to(DEV), 4e-3, 1e-2, "lsce bf16 grad, ignored rows")
    # out-of-range labels (the reference's scatter_ raises): NaN row + status, and the trainer-side check raises once
    bad = label.clone()
    bad[0] = Cc
    bad[2] = -7
    loss = LabelSmoothSoftmaxCEV1(0.1)(lg.clone().requires_grad_(True), bad)
    assert torch.isnan(loss)
    with pytest.raises(IndexError):
        Fn.check_labels()
    Fn.check_labels()
    rk = torch.empty(R, device=DEV, dtype=torch.long)
    ops.rank(lg, bad, rk)
    assert int(rk[0]) == 0 and int(rk[2]) == 0 and int(rk[3]) >= 1


def test_loss_rank_kernels(ops, golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "g3_loss_rank.npz"))
    lg = torch.from_numpy(g["logits"]).to(DEV)
    label = torch.from_numpy(g["label"]).to(DEV)
    R, Cc = lg.shape
    rows, lse = torch.empty(R, device=DEV), torch.empty(R, device=DEV)
    ops.lsce_fwd(lg, label, 0.1, rows, lse)
    assert abs(float(rows.mean()) - float(g["lsce"])) < 2e-5
    dl = torch.empty(R, Cc, device=DEV)
    dlb = torch.full((R, 64), 3.0, device=DEV, dtype=BF)
    one = torch.ones(1, device=DEV)
    ops.lsce_bwd(lg, label, lse, 0.1, one, 1.0 / R, dl_bf16=dlb, dl_f32=dl)
    close(dl, torch.from_numpy(g["lsce_grad"]).to(DEV), 1e-6, 1e-4, "lsce grad (reference golden)")
    assert float(dlb[:, Cc:].abs().max()) == 0
    rk = torch.empty(R, device=DEV, dtype=torch.long)
    ops.rank(lg, label, rk)
    np.testing.assert_array_equal(rk.cpu().numpy(), g["ranks"])          # bit-exact ranks (reference golden)
    h = torch.from_numpy(g["h"]).to(DEV)
    rel, qh, ah = [torch.from_numpy(g[k]).to(DEV) for k in ("rel_idx", "q_head_idx", "a_head_idx")]
    lr_ = torch.empty(h.shape[0], device=DEV)
    ops.simloss_fwd(h, rel, qh, ah, lr_)
    assert abs(float(lr_.mean()) - float(g["sim"])) < 1e-6
    dh = torch.zeros_like(h)
    ops.simloss_bwd(h, rel, qh, ah, one, 1.0 / h.shape[0], dh)
    close(dh, torch.from_numpy(g["sim_grad"]).to(DEV), 1e-6, 1e-4, "sim grad (reference golden)")
    # big random case: ranks vs double sort
    big = rnd(64, 2063, seed=5, dtype=F32, scale=3)
    lab = torch.randint(0, 2063, (64,)).to(DEV)
    ops.rank(big, lab, rk2 := torch.empty(64, device=DEV, dtype=torch.long))
    _, o1 = torch.sort(big, dim=1, descending=True)
    _, o2 = torch.sort(o1, dim=1)
    assert torch.equal(rk2, o2[torch.arange(64, device=DEV), lab] + 1)


def test_adamw_and_misc(ops):
    n = 5000
    flat = 8192
    p0 = rnd(flat, seed=1, dtype=F32)
    g = rnd(flat, seed=2, dtype=F32) * 0.01
    master, m, v = p0.clone(), torch.zeros(flat, device=DEV), torch.zeros(flat, device=DEV)
    shadow = torch.zeros(flat, device=DEV, dtype=BF)
    chunks = torch.tensor([[0, 4096, 1], [4096, n - 4096, 0]], dtype=torch.int32).to(DEV)
    pr = [p0[:4096].clone().requires_grad_(True), p0[4096:n].clone().requires_grad_(True)]
    opt = torch.optim.AdamW([{"params": [pr[0]], "weight_decay": 0.01}, {"params": [pr[1]], "weight_decay": 0.0}], lr=5e-5, eps=1e-8)
    for step in range(1, 4):
        pr[0].grad, pr[1].grad = g[:4096].clone(), g[4096:n].clone()
        opt.step()
        ops.adamw(master=master, grad=g, m=m, v=v, shadow=shadow, chunks=chunks, n_chunks=2, lr=5e-5, beta1=0.9, beta2=0.999, eps=1e-8,
                  weight_decay=0.01, bc1=1 - 0.9 ** step, bc2=1 - 0.999 ** step)
    close(master[:4096], pr[0].detach(), 1e-6, 1e-6, "adamw decay group")
    close(master[4096:n], pr[1].detach(), 1e-6, 1e-6, "adamw no-decay group")
    assert torch.equal(master[n:], p0[n:])
    close(shadow[:n], master[:n], 1e-2, 1e-2, "bf16 shadow")
    # transposes of packed weights
    w = rnd(768 * 2304 + 3072 * 768, seed=3)
    wt = torch.zeros_like(w)
    table = torch.tensor([[0, 0, 2304, 768], [768 * 2304, 768 * 2304, 768, 3072]], dtype=torch.int64).to(DEV)
    ops.transpose_table(w, wt, table, 2)
    assert torch.equal(wt[:768 * 2304].view(768, 2304), w[:768 * 2304].view(2304, 768).t())
    assert torch.equal(wt[768 * 2304:].view(3072, 768), w[768 * 2304:].view(768, 3072).t())
    ids = torch.full((4, 16), 7, dtype=torch.long)
    ids[0, 3] = 103; ids[1, 15] = 103; ids[2, 0] = 103; ids[3, 9] = 103
    pos, row = torch.empty(4, dtype=torch.int32, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)
    ops.find_token(ids.to(DEV), 103, pos, row)
    assert pos.tolist() == [3, 15, 0, 9] and row.tolist() == [3, 31, 32, 57]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.find_token(ids.to(DEV), 103, pos, row, status=status)
    assert int(status) == 0
    ids[1, 15] = 7                                      # an example without the token: pos -1, row b*L+0, status bit 1
    ops.find_token(ids.to(DEV), 103, pos, row, status=status)
    assert pos.tolist() == [3, -1, 0, 9] and row.tolist() == [3, 16, 32, 57] and int(status) == 2


def test_adamw_rounds_the_decayed_weight_before_the_adam_term(ops):
    """Weights near 1.0 WITH weight decay (the vision ``layer_norm*.weight`` tensors: the reference's substring rule only exempts
    ``LayerNorm.weight``): torch rounds ``p * (1 - lr * wd)`` to fp32 and then subtracts the Adam term.  ulp(1.0) = 1.2e-7 is 0.3 % of an
    update of ~lr = 5e-5, so a kernel that contracts the two into one FMA lands one ulp off on about half of the elements every step, and the
    weight DELTAS of a trajectory leave the reference's by 1.5e-3 relative (tests/test_trajectory_gpu.py).  Reference: fp64, with that one
    rounding modelled.  The Adam term itself carries a few 2^-24 relative (1.5e-11 absolute): it moves a result across a rounding boundary
    with probability ~1.5e-11 / 1.2e-7 = 1.3e-4 per element and step -- at most 1 % of the elements may differ at all (25 x that, three
    steps), and none by more than one ulp per step.  Measured on MI355X: 0.63 %, max 0.99 ulp (the kernel forms 1 - beta2 in fp32, 1.3e-5
    relative in v, so its Adam term is further from fp64 than the estimate above assumes); with the contraction 48 %, 2.9 ulp."""
    n, lr, wd, b1, b2, eps = 4096, 5e-5, 0.01, 0.9, 0.999, 1e-8
    p0 = (1.0 + 0.05 * rnd(n, seed=11, dtype=F32)).contiguous()
    master, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    shadow = torch.zeros(n, device=DEV, dtype=BF)
    chunks = torch.tensor([[0, n, 1]], dtype=torch.int32).to(DEV)
    w, m64, v64 = p0.clone(), torch.zeros(n, device=DEV, dtype=torch.float64), torch.zeros(n, device=DEV, dtype=torch.float64)
    decay = torch.tensor(1.0 - lr * wd, dtype=F32, device=DEV)
    for step in range(1, 4):
        g = rnd(n, seed=20 + step, dtype=F32) * 0.01
        ops.adamw(master=master, grad=g, m=m, v=v, shadow=shadow, chunks=chunks, n_chunks=1, lr=lr, beta1=b1, beta2=b2, eps=eps,
                  weight_decay=wd, bc1=1 - b1 ** step, bc2=1 - b2 ** step)
        m64 = b1 * m64 + (1 - b1) * g.double()
        v64 = b2 * v64 + (1 - b2) * g.double() ** 2
        wdec = w * decay                                                    # fp32, rounded once
        w = (wdec.double() - (lr / (1 - b1 ** step)) * m64 / (v64.sqrt() / (1 - b2 ** step) ** 0.5 + eps)).float()
    ulp = 2.0 ** -23 * master.abs()
    diff = (master.double() - w.double()).abs()
    frac = float((master != w).float().mean())
    print(f"\nadamw at w ~ 1 with decay: {frac * 100:.2f} % of the elements differ from the fp64 reference, max {float((diff / ulp).max()):.2f} ulp")
    assert frac <= 0.01 and float((diff / ulp).max()) <= 3.0, (frac, float((diff / ulp).max()))


def test_device_side_batch_assembly(ops):
    """patchify_gather / gather_images == stacking rows of the image table on the host (zeros for missing slots)."""
    N, B, S, p = 7, 5, 224, 16
    table = rnd(N, 3, S, S, seed=1, dtype=F32)
    idx = torch.tensor([[0, 3], [6, -1], [-1, -1], [2, 2], [5, 1]], dtype=torch.int32, device=DEV)
    pix = torch.zeros(B, 2, 3, S, S, device=DEV)
    for b in range(B):
        for s_ in range(2):
            if idx[b, s_] >= 0:
                pix[b, s_] = table[idx[b, s_]]
    out = torch.empty_like(pix)
    ops.gather_images(table, idx, out, B, S)
    assert torch.equal(out, pix)
    P = (S // p) ** 2
    a, b_ = torch.empty(B * 2 * P, 3 * p * p, device=DEV, dtype=BF), torch.empty(B * 2 * P, 3 * p * p, device=DEV, dtype=BF)
    ops.patchify(pix, a, B, S, p)
    ops.patchify_gather(table, idx, b_, B, S, p)
    assert torch.equal(a, b_)


def test_row_subset_helpers(ops):
    """needed_rows / rows_lookup / rows_dense / the relaxation loss on compact rows / split-K sum / AdamW's folded zero-fill (round 6)."""
    from mkg_analogy_amd import functional as Fn
    B, L, H = 6, 24, 64
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(1000, 2000, (B, L), generator=g)
    mpos = [3, 23, 0, 11, 7, 9]
    for b, p in enumerate(mpos):
        ids[b, p] = 103
    ids[4, 7] = 5                                        # example 4 has no [MASK]
    rel = torch.tensor([[1, 5], [2, 6], [3, 7], [1, 8], [-1, 4], [0, 0]])
    qh, ah = torch.tensor([1, 1, 2, 3, 4, 5]), torch.tensor([4, 5, 6, 7, 4, -24])
    dev_ids = ids.to(DEV)
    st = Fn._status(dev_ids.device)
    st.zero_()
    rows = Fn.needed_rows(dev_ids, 103, (rel.to(DEV), qh.to(DEV), ah.to(DEV)))
    exp = torch.stack([torch.tensor([m if b != 4 else 0 for b, m in enumerate(mpos)]), rel[:, 0] % L, rel[:, 1] % L, qh % L, ah % L], 1) + torch.arange(B)[:, None] * L
    assert rows.dtype == torch.int32 and torch.equal(rows.cpu().long(), exp) and torch.equal(rows._mart_mask_row.cpu().long(), exp[:, 0])
    assert int(st) == 2
    st.zero_()
    r1 = Fn.needed_rows(dev_ids, 103)
    assert tuple(r1.shape) == (B, 1) and torch.equal(r1.cpu().long()[:, 0], exp[:, 0])
    st.zero_()
    # lookup: first slot wins; a row outside the promise -> slot 0 of its example + status bit 2
    flat = torch.tensor([exp[0, 3], exp[5, 1], exp[2, 0], 1 * L + 20], dtype=torch.int32, device=DEV)
    out = torch.empty(4, dtype=torch.int32, device=DEV)
    ops.rows_lookup(flat, rows, L, out, status=st)
    first = lambda b, f: b * 5 + [int(x) for x in exp[b]].index(int(f))
    assert out.tolist() == [first(0, exp[0, 3]), first(5, exp[5, 1]), first(2, exp[2, 0]), 5] and int(st) == 4
    st.zero_()
    # dense view: promised rows (first slot), NaN elsewhere; its backward takes a repeated position once
    comp = rnd(B * 5, H, seed=3, dtype=F32).requires_grad_(True)
    dense = Fn._DenseRowsFn.apply(comp, rows, B, L)
    ref = torch.full((B * L, H), float("nan"), device=DEV)
    for b in range(B):
        for j in reversed(range(5)):
            ref[int(exp[b, j])] = comp.detach()[b * 5 + j]
    assert torch.equal(torch.nan_to_num(dense.view(-1, H), nan=-7.0), torch.nan_to_num(ref, nan=-7.0))
    gd = rnd(B, L, H, seed=4, dtype=F32)
    dense.backward(gd)
    gref = torch.zeros(B * 5, H, device=DEV)
    for b in range(B):
        seen = set()
        for j in range(5):
            f = int(exp[b, j])
            if f not in seen:
                gref[b * 5 + j] = gd.view(-1, H)[f]
            seen.add(f)
    assert torch.equal(comp.grad, gref)
    # relaxation loss on the compact rows == on the dense tensor (values and gradients)
    tr = rnd(B, L, H, seed=5, dtype=F32)
    comp2 = torch.stack([tr.view(-1, H)[int(exp[b, j])] for b in range(B) for j in range(5)]).contiguous().requires_grad_(True)
    trd = tr.clone().requires_grad_(True)
    l_d = Fn.relaxation_loss(trd, rel.to(DEV), qh.to(DEV), ah.to(DEV))
    l_d.backward()
    l_c = Fn._SimLossFn.apply(comp2, rel.to(DEV), qh.to(DEV), ah.to(DEV), rows, L)
    l_c.backward()
    ar = torch.arange(B)
    cos = torch.nn.functional.cosine_similarity
    t_ = tr.cpu()
    l_ref = (torch.relu(cos(t_[ar, qh], t_[ar, ah])) + 1 - cos(t_[ar, rel[:, 0]], t_[ar, rel[:, 1]])).mean()
    assert abs(float(l_d) - float(l_ref)) < 1e-5 and abs(float(l_c) - float(l_d)) < 1e-6
    gsum = torch.zeros(B * L, H, device=DEV)
    for b in range(B):
        for j in range(5):
            gsum[int(exp[b, j])] += comp2.grad[b * 5 + j]
    close(gsum, trd.grad.view(-1, H), 1e-6, 1e-5, "relaxation-loss gradient, compact rows vs dense")
    # a position the pass was not promised: that example's loss is NaN (nothing read)
    bad = Fn._SimLossFn.apply(comp2.detach(), rel.to(DEV), torch.tensor([1, 1, 2, 3, 4, 6], device=DEV), ah.to(DEV), rows, L)
    assert torch.isnan(bad)
    # ordered split-K sum
    parts = rnd(5, 12, 64, seed=6, dtype=F32)
    o = torch.empty(12, 64, device=DEV)
    ops.sum_splits_f32(parts, o)
    close(o, parts.sum(0), 1e-6, 1e-6, "sum_splits")
    # AdamW with the zero-fill folded in: same update, gradients of the updated chunks read zero afterwards, the rest untouched
    n = 70000
    res = []
    for zg in (False, True):
        master, grad = rnd(n, seed=1, dtype=F32), rnd(n, seed=2, dtype=F32)
        m, v, sh = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV, dtype=BF)
        chunks = torch.tensor([[0, 65536, 1], [65536 + 256, 1000, 0]], dtype=torch.int32, device=DEV)
        ops.adamw(master=master, grad=grad, m=m, v=v, shadow=sh, chunks=chunks, n_chunks=2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01,
                  bc1=0.1, bc2=0.001, zero_grad=zg)
        res.append((master, grad, m))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2])
    g1, g0 = res[1][1], res[0][1]
    assert float(g1[:65536].abs().max()) == 0.0 and float(g1[65536 + 256:65536 + 1256].abs().max()) == 0.0
    assert torch.equal(g1[65536:65536 + 256], g0[65536:65536 + 256]) and torch.equal(g1[65536 + 1256:], g0[65536 + 1256:])
