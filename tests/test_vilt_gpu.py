"""ViLT backbone (ViltKGC) on the HIP path: the joint-embedding kernels and the attention reweight row bound (rw_row_lo) against torch
fp32, the training step and the forward pass against the unmodified reference (goldens G10 / G10b, tools/gen_goldens_vilt.py),
determinism of the backward pass, and a short Trainer.fit."""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("B,L", [(2, 64), (3, 37)])          # S = 354 / 327
def test_vilt_embed_fwd_bwd_vs_torch(B, L):
    from mkg_analogy_amd import ops
    torch.manual_seed(B)
    H, P, V, NT = 768, 144, 500, 40
    dev = "cuda"
    S = L + 2 * (1 + P)
    word, tpos, ttype = torch.randn(V, H) * .5, torch.randn(NT, H) * .5, torch.randn(2, H) * .5
    gamma, beta = 1 + 0.1 * torch.randn(H), 0.1 * torch.randn(H)
    cls, ipos, mod = torch.randn(H), torch.randn(1 + P, H), torch.randn(2, H)
    pe = torch.randn(B * 2 * P, H)
    ids = torch.randint(0, V, (B, L)); tt = torch.randint(0, 2, (B, L))
    perm = torch.stack([torch.stack([torch.randperm(P) for _ in range(B)]) for _ in range(2)])
    # torch reference
    ps = [t.clone().requires_grad_(True) for t in (word, tpos, ttype, gamma, beta, cls, ipos, mod, pe)]
    w_, tp_, ty_, g_, b_, c_, ip_, m_, pe_ = ps
    e = w_[ids] + ty_[tt]
    n = min(L, NT)
    e = torch.cat([e[:, :n] + tp_[:n], e[:, n:]], 1)
    xt = torch.nn.functional.layer_norm(e, (H,), g_, b_, 1e-12) + m_[0]
    imgs = []
    for i in range(2):
        pi = pe_.view(B, 2, P, H)[:, i]
        tok = torch.stack([pi[b, perm[i, b]] for b in range(B)]) + torch.stack([ip_[1 + perm[i, b]] for b in range(B)])
        imgs.append(torch.cat([(c_ + ip_[0]).expand(B, 1, H), tok], 1) + m_[1])
    x_ref = torch.cat([xt] + imgs, 1)
    gy = torch.randn(B, S, H)
    (x_ref * gy).sum().backward()
    # HIP
    cu = lambda t: t.to(dev).contiguous()
    x = torch.empty(B * S, H, device=dev)
    s_t, mean, rstd = torch.empty(B * L, H, device=dev), torch.empty(B * L, device=dev), torch.empty(B * L, device=dev)
    pd = cu(perm.to(torch.int32)); inv = cu(torch.argsort(perm, -1).to(torch.int32))
    ops.vilt_embed_fwd(ids=cu(ids), tt=cu(tt), word=cu(word), tpos=cu(tpos), ttype=cu(ttype), gamma=cu(gamma), beta=cu(beta), eps=1e-12, n_tpos=NT,
                       patch_f32=cu(pe), cls=cu(cls), ipos=cu(ipos), modality=cu(mod), perm=pd, B=B, L=L, P=P, H=H, x=x, s_text=s_t, mean=mean, rstd=rstd)
    torch.cuda.synchronize()
    assert float((x.view(B, S, H).cpu() - x_ref.detach()).abs().max()) < 2e-5
    z = lambda *s: torch.zeros(*s, device=dev)
    grads = dict(dgamma=z(H), dbeta=z(H), dtpos=z(NT, H), dttype=z(2, H), dcls=z(H), dipos=z(1 + P, H), dmodality=z(2, H))
    ds_t, dpatch = torch.empty(B * L, H, device=dev), torch.empty(B * 2 * P, H, device=dev, dtype=torch.bfloat16)
    ws = torch.empty((1 + P + 4 * L) * H, device=dev)
    ops.vilt_embed_bwd(ids=cu(ids), tt=cu(tt), gamma=cu(gamma), n_tpos=NT, modality=cu(mod), perm=pd, inv=inv, B=B, L=L, P=P, H=H, s_text=s_t,
                       mean=mean, rstd=rstd, dx=cu(gy.view(B * S, H)), ds_text=ds_t, dpatch=dpatch, ws=ws, **grads)
    torch.cuda.synchronize()
    ref = dict(dgamma=g_.grad, dbeta=b_.grad, dtpos=tp_.grad, dttype=ty_.grad, dcls=c_.grad, dipos=ip_.grad, dmodality=m_.grad)
    for k, r in ref.items():
        err = float((grads[k].cpu() - r).abs().max()) / max(1.0, float(r.abs().max()))
        assert err < 1e-5, (k, err)
    assert float((dpatch.float().cpu() - pe_.grad).abs().max()) <= 0.01 * float(pe_.grad.abs().max())
    dword = torch.zeros(V, H).index_add_(0, ids.reshape(-1), ds_t.cpu())
    assert float((dword - w_.grad).abs().max()) < 1e-4 * max(1.0, float(w_.grad.abs().max()))
    # a second pass adds exactly the same bits
    g2 = {k: torch.zeros_like(v) for k, v in grads.items()}
    ops.vilt_embed_bwd(ids=cu(ids), tt=cu(tt), gamma=cu(gamma), n_tpos=NT, modality=cu(mod), perm=pd, inv=inv, B=B, L=L, P=P, H=H, s_text=s_t,
                       mean=mean, rstd=rstd, dx=cu(gy.view(B * S, H)), ds_text=ds_t, dpatch=dpatch, ws=ws, **g2)
    assert all(torch.equal(g2[k], grads[k]) for k in grads)


@pytest.mark.parametrize("S,L", [(354, 64), (327, 37)])
def test_attention_row_lo_vs_torch(S, L):
    """ViLT reweight (modeling_vilt.py:370-375): rows [lo, s') x keys [s', S) by clamp(w0), rows [s', S) x keys [s', S) by clamp(w1);
    padded keys; forward, dq / dk / dv and d(w0) / d(w1)."""
    from mkg_analogy_amd import ops
    torch.manual_seed(S)
    B, nh, D = 2, 12, 64
    H = nh * D
    dev = "cuda"
    ni = S - L
    qkv = (torch.randn(B * S, 3 * H) * 0.5).to(torch.bfloat16)
    am = torch.ones(B, S, dtype=torch.int64)
    am[0, L - 5:L] = 0                                         # padded text keys
    sep = torch.tensor([30, L - 9]) + ni                       # s' = sep_idx[:, 2] + 290
    w = torch.tensor([0.3, 0.7])
    dctx = (torch.randn(B * S, H) * 0.5).to(torch.bfloat16)
    # torch fp32 reference on the same bf16 operands
    q, k, v = [qkv[:, i * H:(i + 1) * H].float().view(B, S, nh, D).transpose(1, 2).clone().requires_grad_(True) for i in range(3)]
    wr = w.clone().requires_grad_(True)
    sc = q @ k.transpose(-1, -2) / 8.0
    rows = torch.arange(S)[:, None]; keys = torch.arange(S)[None]
    fac = []
    for b in range(B):
        s_ = int(sep[b])
        f = torch.ones(S, S)
        f0 = ((rows >= ni + 1) & (rows < s_) & (keys >= s_)).float()
        f1 = ((rows >= s_) & (keys >= s_)).float()
        fac.append(1 + f0 * (wr[0].clamp(0, .5) - 1) + f1 * (wr[1].clamp(.5, 1) - 1))
    sc = sc * torch.stack(fac)[:, None] + ((1 - am[:, None, None, :].float()) * -10000.0)
    ctx_ref = (sc.softmax(-1) @ v).transpose(1, 2).reshape(B * S, H)
    (ctx_ref * dctx.float()).sum().backward()
    g = qkv.to(dev)
    ctx = torch.empty(B * S, H, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, nh, S, device=dev)
    w0, w1 = w[0:1].to(dev).contiguous(), w[1:2].to(dev).contiguous()
    kw = dict(q=g[:, :H], k=g[:, H:2 * H], v=g[:, 2 * H:], ctx=ctx, lse=lse, B=B, nh=nh, Sq=S, Sk=S, scale=0.125, attn_mask=am.to(dev),
              sep=sep.to(dev), sep_stride=1, w0=w0, w1=w1, rw_row_lo=ni + 1)
    ops.attn_fwd(**kw)
    dqkv = torch.empty(B * S, 3 * H, device=dev, dtype=torch.bfloat16)
    dw = torch.zeros(2, device=dev)
    ops.attn_bwd(dctx=dctx.to(dev), delta=torch.empty(B, nh, S, device=dev), dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:], dw=dw, **kw)
    torch.cuda.synchronize()
    e = float((ctx.float().cpu() - ctx_ref.detach()).abs().max())
    assert e < 2e-2 * max(1.0, float(ctx_ref.abs().max())), e
    for i, t in enumerate((q, k, v)):
        r = t.grad.transpose(1, 2).reshape(B * S, H)
        got = dqkv[:, i * H:(i + 1) * H].float().cpu()
        rel = float((got - r).norm() / r.norm())
        assert rel < 2e-2, ("qkv"[i], rel)
    # d(key.bias) = column sums of dK: a cancellation residue of the reweighted key block (zero for plain softmax attention), checked here against
    # the fp32 reference on identical operands so that a dK regression of the LO kernels cannot hide behind the scale the model test judges it on
    dkb = dqkv[:, H:2 * H].float().cpu().sum(0)
    dkb_ref = k.grad.transpose(1, 2).reshape(B * S, H).sum(0)
    err_kb = float((dkb - dkb_ref).norm())
    rel_kb = err_kb / float(dkb_ref.norm())
    on_dk = err_kb / float(k.grad.norm())
    print(f"\nrow_lo S={S}: d(key.bias) rel-L2 {rel_kb:.3e}, error / |dK| {on_dk:.3e} (|ref| {float(dkb_ref.norm()):.3e}, |dK| {float(k.grad.norm()):.3e})")
    # bf16 floor: dK is stored in bf16 and d(key.bias) is 19-34x smaller than |dK| here, so its relative error is that ratio times the rounding of
    # the summed rows (measured 6.0e-2 / 1.1e-1); on dK's own scale the error is 3.2e-3 / 3.4e-3
    assert on_dk < 1e-2, (rel_kb, on_dk)
    # ... and the gate tells a wrong row bound apart: the same backward without it misses the reference's d(key.bias) by far more
    ctx_n, lse_n, dq_n = torch.empty_like(ctx), torch.empty_like(lse), torch.empty_like(dqkv)
    kw_n = dict(kw, ctx=ctx_n, lse=lse_n, rw_row_lo=0)
    ops.attn_fwd(**kw_n)
    ops.attn_bwd(dctx=dctx.to(dev), delta=torch.empty(B, nh, S, device=dev), dq=dq_n[:, :H], dk=dq_n[:, H:2 * H], dv=dq_n[:, 2 * H:],
                 dw=torch.zeros(2, device=dev), **kw_n)
    torch.cuda.synchronize()
    err_kb_n = float((dq_n[:, H:2 * H].float().cpu().sum(0) - dkb_ref).norm())
    print(f"   without the row bound: d(key.bias) error / |dK| {err_kb_n / float(k.grad.norm()):.3e}")
    assert err_kb_n > 10 * err_kb, (err_kb, err_kb_n)
    rel_w = (dw.cpu() - wr.grad).abs() / wr.grad.abs().clamp_min(1e-3)
    assert float(rel_w.max()) < 2e-2, (dw.cpu(), wr.grad)
    # without the row bound the rows below it would be reweighted too: the test tells the two apart
    ctx0 = torch.empty_like(ctx)
    ops.attn_fwd(**dict(kw, ctx=ctx0, rw_row_lo=0))
    torch.cuda.synchronize()
    below = torch.cat([torch.arange(b * S, b * S + ni + 1) for b in range(B)])     # the rows under the bound
    r_lo = ctx_ref.detach()[below]
    e_with = float((ctx.float().cpu()[below] - r_lo).abs().mean())
    e_without = float((ctx0.float().cpu()[below] - r_lo).abs().mean())
    assert e_without > 4 * e_with, (e_with, e_without)


# ------------------------------------------------------------------ model vs the reference
def _build(B, L, gold):
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.lit_models import TransformerLitModel
    from mkg_analogy_amd.models import ViltKGC, vilt_config
    from tools.gen_goldens_vilt import weights
    g = np.load(os.path.join(GOLD, gold))
    torch.manual_seed(0)
    model = ViltKGC(vilt_config(vocab_size=30522))
    cfg = D.data_config(seed=1234)
    args = argparse.Namespace(label_smoothing=0.1, alpha=0.3, pretrain=0, lr=4e-5, weight_decay=0.01, optimizer="AdamW", warm_up_radio=0.1)
    lit = TransformerLitModel(model=model, args=args, tokenizer=D.FakeTokenizer(), data_config=cfg)      # resize -> 42006
    model.cuda()
    lit._init_relation_word()                                                                            # -> 42007
    sd = weights([(n, p.shape) for n, p in model.named_parameters()], cfg["analogy_relation_ids"])
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(("position_ids" in m or "decoder" in m) for m in missing), (missing, unexpected)
    batch = D.make_batch(B, L, image_size=384, seed=int(g["batch_seed"]))
    return model, lit, g, batch, cfg


@pytest.mark.parametrize("gold", ["g10_vilt_real.npz", "g10b_vilt_odd.npz"])
def test_vilt_step_and_forward_vs_reference(gold):
    g = np.load(os.path.join(GOLD, gold))
    B, L = int(g["B"]), int(g["L"])
    model, lit, g, batch, cfg = _build(B, L, gold)
    ids = torch.tensor(cfg["analogy_entity_ids"]).cuda()
    gb = {k: v.cuda() for k, v in batch.items()}
    sep_before = gb["sep_idx"].clone()
    model.eval()
    st = model.store
    st.zero_grad()
    torch.manual_seed(int(g["fwd_seed"]))
    loss = lit.training_step(dict(gb), 1)
    assert np.array_equal(model.engine.patch_order.numpy(), g["patch_order"])
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(gb["sep_idx"], sep_before)
    torch.manual_seed(int(g["fwd_seed"]))
    out, trans = model(input_ids=gb["input_ids"], attention_mask=gb["attention_mask"], token_type_ids=gb["token_type_ids"],
                       pixel_values=gb["pixel_values"], sep_idx=gb["sep_idx"], return_dict=True)
    ar = torch.arange(B, device="cuda")
    _, mi = (gb["input_ids"] == 103).nonzero(as_tuple=True)
    ml = out.logits[ar, mi][:, ids].float().cpu()
    ml_ref = torch.from_numpy(g["mask_logits"])
    e_l = float((ml - ml_ref).abs().max())
    gate = max(1e-2, 2 * float(g["bf16_control_dev"]))
    rows = torch.from_numpy(g["trans_row_index"]).cuda()
    tr = trans.detach()[ar[:, None], rows].float().cpu()
    tr_ref = torch.from_numpy(g["trans_rows"])
    rel_t = float((tr - tr_ref).norm() / tr_ref.norm())
    dl = abs(float(loss.detach()) - float(g["loss"]))
    print(f"\nvilt {gold}: loss hip {float(loss.detach()):.5f} ref {float(g['loss']):.5f}; trans rel-L2 {rel_t:.3e}; logits max|err| {e_l:.3e} "
          f"(gate {gate:.3e}, bf16-weight control {float(g['bf16_control_dev']):.3e})")
    assert e_l <= gate and rel_t < 4e-3 and dl < 5e-3
    names = [k[4:] for k in g.files if k.startswith("gs::")]
    assert len(names) >= 40
    gn = dict(zip([str(x) for x in g["grad_norm_names"]], g["grad_norm_vals"]))

    def cancels(n):
        # d(key.bias) = sum over keys of d(score) . q: zero for plain softmax attention (a per-row shift), here only the reweighted key block's
        # residue is left (layer 6: 1.2e-4, 60x below query.bias).  Its error is judged on the scale of the same layer's query.bias gradient.
        return n.endswith("attention.attention.key.bias")
    for n in names:
        got = st.g(n).detach().float().cpu().reshape(-1)
        step = max(1, got.numel() // 1024)
        got = got[::step][:1024]
        r = torch.from_numpy(g["gs::" + n])
        if r.norm().item() < 1e-7:
            assert got.norm().item() < 1e-3, n
            continue
        rel = ((got - r).norm() / r.norm()).item()
        cos = torch.nn.functional.cosine_similarity(got, r, dim=0).item()
        print(f"   grad {n}: rel-L2 {rel:.3e} cos {cos:.5f}")
        if cancels(n):
            assert (got - r).norm().item() < 0.12 * gn[n.replace("key.bias", "query.bias")], n
        elif got.numel() == 1:
            assert abs(float(got) - float(r)) < 0.12 * abs(float(r)) + 3e-3, n
        else:
            assert cos > 0.99 and rel < 0.12, n
    for n, ref in gn.items():
        got = float(st.g(n).double().norm())
        tol = 0.12 * (gn[n.replace("key.bias", "query.bias")] if cancels(n) else ref)
        assert abs(got - ref) <= tol + 1e-6, (n, got, ref)
    for n in ("vilt.pooler.dense.weight", "vilt.pooler.dense.bias"):
        assert float(st.g(n).abs().max()) == 0.0
    # evaluation ranks in the training configuration (bf16): exact wherever the label's logit gap exceeds twice the measured error
    lab = ml_ref[torch.arange(B), torch.from_numpy(g["in::label"])]
    amb = ((ml_ref - lab[:, None]).abs() < 2 * e_l).sum(1).numpy() - 1
    model.set_precision("bf16")
    torch.manual_seed(int(g["fwd_seed"]))
    ev = lit._eval(dict(gb), 0)
    assert np.all(np.abs(ev["entity_ranks"] - g["ranks"]) <= amb)
    # ---- fp32-accurate evaluation path (engine_precise.PreciseViltForward): north_star's 1e-3 gate on logits, exact ranks where the gap allows
    model.set_precision("fp32")
    with torch.no_grad():
        torch.manual_seed(int(g["fwd_seed"]))
        out32, trans32 = model(input_ids=gb["input_ids"], attention_mask=gb["attention_mask"], token_type_ids=gb["token_type_ids"],
                               pixel_values=gb["pixel_values"], sep_idx=gb["sep_idx"], return_dict=True)
    ml32 = out32.logits[ar, mi][:, ids].float().cpu()
    e32 = float((ml32 - ml_ref).abs().max())
    t32 = float((trans32[ar[:, None], rows].float().cpu() - tr_ref).abs().max())
    print(f"   fp32 path: logits max|err| {e32:.3e}  trans rows max|err| {t32:.3e}")
    assert e32 <= 1e-3 and t32 < 5e-3
    torch.manual_seed(int(g["fwd_seed"]))
    ev32 = lit._eval_at(dict(gb), 0)                          # the lit model's default evaluation precision: fp32
    gap = (ml_ref - lab[:, None]).abs()
    gap[torch.arange(B), torch.from_numpy(g["in::label"])] = 1e9
    safe = (gap.min(1).values > 2 * e32).numpy()
    assert safe.any()
    assert np.array_equal(ev32["entity_ranks"][safe], np.asarray(g["ranks"])[safe])
    model.set_precision("bf16")


def test_vilt_image_table_path_matches_pixels():
    """Batches that carry image_index into the device table (model.set_image_table) give the pixel_values forward, bit for bit, on both the
    bf16 and the fp32 evaluation path (same patch order: the same seed before each call)."""
    model, lit, g, batch, cfg = _build(3, 37, "g10b_vilt_odd.npz")
    model.eval()
    gb = {k: v.cuda() for k, v in batch.items()}
    B = 3
    table = batch["pixel_values"].reshape(B * 2, 3, 384, 384)
    index = torch.arange(B * 2, dtype=torch.int32).view(B, 2)
    index[1, 1] = -1                                          # a missing entity: zero image
    pix = gb["pixel_values"].clone()
    pix[1, 1] = 0.0
    model.set_image_table(table)
    kw = dict(input_ids=gb["input_ids"], attention_mask=gb["attention_mask"], token_type_ids=gb["token_type_ids"], sep_idx=gb["sep_idx"], return_dict=True)
    for prec in ("bf16", "fp32"):
        model.set_precision(prec)
        with torch.no_grad():
            torch.manual_seed(3)
            _, t_pix = model(pixel_values=pix, **kw)
            torch.manual_seed(3)
            _, t_idx = model(image_index=index.cuda(), **kw)
        torch.cuda.synchronize()
        assert torch.equal(t_pix, t_idx), prec
    model.set_precision("bf16")


def test_vilt_backward_bit_identical():
    model, lit, g, batch, cfg = _build(2, 64, "g10_vilt_real.npz")
    gb = {k: v.cuda() for k, v in batch.items()}
    model.eval()
    st = model.store
    outs = []
    for _ in range(2):
        st.zero_grad()
        torch.manual_seed(5)
        loss = lit.training_step(dict(gb), 1)
        loss.backward()
        torch.cuda.synchronize()
        outs.append(st.grad.detach().clone())
    assert torch.equal(outs[0], outs[1])


def test_vilt_trainer_fit_loss_falls():
    from mkg_analogy_amd.trainer import Trainer
    model, lit, g, batch, cfg = _build(8, 48, "g10_vilt_real.npz")
    from mkg_analogy_amd import data_synth as D
    b = D.make_batch(8, 48, image_size=384, seed=99)
    batches = [{k: v.cuda() for k, v in b.items()} for _ in range(5)]           # the same batch five times: the loss must fall
    lit.args.lr = 2e-4
    tr = Trainer(max_epochs=1, max_steps=5, world_size=1)
    losses, step = [], tr.train_step

    def rec(*a, **k):
        loss = step(*a, **k)
        losses.append(float(loss))
        return loss
    tr.train_step = rec
    tr.fit(lit, batches)
    print("\nvilt fit losses", losses)
    assert len(losses) == 5 and all(np.isfinite(losses)) and losses[-1] < losses[0]
