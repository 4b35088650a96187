"""VisualBERT backbone (VisualBertKGC) on the HIP path: the joint-embedding kernels (csrc/visual_bert.hip) and the attention kernels at joint shapes
with a non-prefix key mask against torch fp32, the training step and the forward pass against the unmodified reference (goldens G11 / G11b,
tools/gen_goldens_visualbert.py), determinism of the backward pass, a short Trainer.fit with dropout on, and a reload through the lit model."""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("input_ids", "attention_mask", "token_type_ids", "pixel_values", "visual_attention_mask", "sep_idx")


# ------------------------------------------------------------------ kernels
def _embed_case(B, L, V, seed):
    torch.manual_seed(seed)
    H, NW, NP = 768, 500, 64
    t = dict(word=torch.randn(NW, H) * .5, pos=torch.randn(NP, H) * .5, type=torch.randn(2, H) * .5, vpos=torch.randn(NP, H) * .5,
             vtype=torch.randn(2, H) * .5, gamma=1 + 0.1 * torch.randn(H), beta=0.1 * torch.randn(H), proj=torch.randn(B * V, H))
    ids, tt = torch.randint(0, NW, (B, L)), torch.randint(0, 2, (B, L))
    return H, t, ids, tt, torch.randn(B, L + V, H)


def _embed_ref(t, ids, tt, B, L, V, H, keep=None, p=0.0):
    """fp32 torch autograd of VisualBertEmbeddings.forward as MarT calls it; ``keep``: the dropout mask to apply (1 = kept)."""
    ps = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    e = ps["word"][ids] + ps["type"][tt] + ps["pos"][:L]
    v = ps["proj"].view(B, V, H) + ps["vpos"][0] + ps["vtype"][1]
    x = torch.nn.functional.layer_norm(torch.cat([e, v], 1), (H,), ps["gamma"], ps["beta"], 1e-12)
    if keep is not None:
        x = x * keep / (1.0 - p)
    return x, ps


def _embed_hip(t, ids, tt, B, L, V, H, p, seed, gy=None):
    from mkg_analogy_amd import ops
    dev = "cuda"
    S, M = L + V, B * (L + V)
    cu = lambda a: a.to(dev).contiguous()
    d = {k: cu(v) for k, v in t.items()}
    x, xb, xh = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev, dtype=torch.bfloat16), torch.empty(M, H, device=dev, dtype=torch.float16)
    s, mean, rstd = torch.empty(M, H, device=dev), torch.empty(M, device=dev), torch.empty(M, device=dev)
    common = dict(ids=cu(ids), tt=cu(tt), gamma=d["gamma"], p_drop=p, seed=seed, B=B, L=L, V=V, H=H, s=s, mean=mean, rstd=rstd)
    ops.vbert_embed_fwd(word=d["word"], pos=d["pos"], type_=d["type"], vpos=d["vpos"][0], vtype=d["vtype"][1], proj=d["proj"], beta=d["beta"],
                        eps=1e-12, x=x, x_bf16=xb, x_f16=xh, **common)
    torch.cuda.synchronize()
    out = dict(x=x, xb=xb, xh=xh)
    if gy is not None:
        z = lambda *sh: torch.zeros(*sh, device=dev)
        g = dict(dgamma=z(H), dbeta=z(H), dpos=z(t["pos"].shape[0], H), dtype=z(2, H), dvpos=z(H), dvtype=z(H))
        ds_t, dproj = torch.empty(B * L, H, device=dev), torch.empty(B * V, H, device=dev, dtype=torch.bfloat16)
        ws = torch.empty((B * V + 4 * S) * H, device=dev)
        ops.vbert_embed_bwd(dx=cu(gy.reshape(M, H)), ds_text=ds_t, dproj=dproj, ws=ws, **common, **g)
        torch.cuda.synchronize()
        out.update(g=g, ds_t=ds_t, dproj=dproj)
    return out


def _check_embed_grads(o, ps, ids, H):
    ref = dict(dgamma=ps["gamma"].grad, dbeta=ps["beta"].grad, dpos=ps["pos"].grad, dtype=ps["type"].grad, dvpos=ps["vpos"].grad[0],
               dvtype=ps["vtype"].grad[1])
    for k, r in ref.items():
        err = float((o["g"][k].cpu() - r).abs().max()) / max(1.0, float(r.abs().max()))
        assert err < 1e-5, (k, err)
    assert float(ps["vpos"].grad[1:].abs().max()) == 0.0 and float(ps["vtype"].grad[0].abs().max()) == 0.0     # only those two rows are read
    pg = ps["proj"].grad
    assert float((o["dproj"].float().cpu() - pg).abs().max()) <= 0.01 * float(pg.abs().max())
    dword = torch.zeros(ps["word"].shape[0], H).index_add_(0, ids.reshape(-1), o["ds_t"].cpu())
    assert float((dword - ps["word"].grad).abs().max()) < 1e-4 * max(1.0, float(ps["word"].grad.abs().max()))


@pytest.mark.parametrize("B,L,V", [(2, 7, 3), (3, 37, 72)])   # 20 rows: fewer than a launch's wave group, nothing a multiple of anything; S = 109
def test_vbert_embed_fwd_bwd_vs_torch(B, L, V):
    H, t, ids, tt, gy = _embed_case(B, L, V, seed=B)
    S = L + V
    x_ref, ps = _embed_ref(t, ids, tt, B, L, V, H)
    (x_ref * gy).sum().backward()
    o = _embed_hip(t, ids, tt, B, L, V, H, 0.0, 0, gy)
    assert float((o["x"].view(B, S, H).cpu() - x_ref.detach()).abs().max()) < 2e-5
    assert torch.equal(o["xb"], o["x"].to(torch.bfloat16)) and torch.equal(o["xh"], o["x"].to(torch.float16))     # the copies layer 0 reads
    _check_embed_grads(o, ps, ids, H)
    o2 = _embed_hip(t, ids, tt, B, L, V, H, 0.0, 0, gy)       # a second pass adds exactly the same bits
    assert all(torch.equal(o2["g"][k], o["g"][k]) for k in o["g"]) and torch.equal(o2["ds_t"], o["ds_t"]) and torch.equal(o2["dproj"], o["dproj"])


@pytest.mark.parametrize("B,L,V", [(2, 7, 3), (3, 37, 72)])
def test_vbert_embed_dropout(B, L, V):
    H, t, ids, tt, gy = _embed_case(B, L, V, seed=10 + B)
    S, p, seed = L + V, 0.1, 0x1234567
    o = _embed_hip(t, ids, tt, B, L, V, H, p, seed, gy)
    o2 = _embed_hip(t, ids, tt, B, L, V, H, p, seed, gy)
    assert torch.equal(o["x"], o2["x"]) and all(torch.equal(o2["g"][k], o["g"][k]) for k in o["g"]) and torch.equal(o2["dproj"], o["dproj"])
    x = o["x"].view(B, S, H).cpu()
    keep = (x != 0).float()
    n = keep.numel()
    p_eff = round(p * 65536) / 65536                          # the 16-bit threshold of the dropout generator
    frac = float(keep.mean())
    assert abs(frac - (1 - p_eff)) < 4 * (p_eff * (1 - p_eff) / n) ** 0.5, frac
    assert not torch.equal(o["x"], _embed_hip(t, ids, tt, B, L, V, H, p, seed + 1)["x"])
    # the same decisions as the LayerNorm kernel's dropout path takes for (seed, element index): a zero input row + y = ones -> keep / (1 - p)
    from mkg_analogy_amd import ops
    M = B * S
    ones, out = torch.ones(M, H, device="cuda"), torch.empty(M, H, device="cuda")
    ops.ln_fwd(x_f32=torch.zeros(M, H, device="cuda"), y_f32=ones, gamma=torch.ones(H, device="cuda"), beta=torch.zeros(H, device="cuda"), eps=1e-12, M=M, H=H,
               mean=torch.empty(M, device="cuda"), rstd=torch.empty(M, device="cuda"), s_out=out, out_f32=torch.empty(M, H, device="cuda"), p_drop=p, seed=seed)
    torch.cuda.synchronize()
    assert torch.equal((out.view(B, S, H).cpu() != 0).float(), keep)
    # kept elements are LN / (1 - p); the gradients are those of torch autograd under the same mask
    x_ref, ps = _embed_ref(t, ids, tt, B, L, V, H, keep=keep, p=p)
    assert float((x - x_ref.detach()).abs().max()) < 2e-5 / (1 - p)
    (x_ref * gy).sum().backward()
    _check_embed_grads(o, ps, ids, H)
    # the backward pass zeroes exactly the dropped elements: a gradient that lives on dropped elements only gives exact zeros everywhere,
    # one that lives on kept elements only gives what the full gradient gives
    od = _embed_hip(t, ids, tt, B, L, V, H, p, seed, gy * (1 - keep))
    assert all(float(v.abs().max()) == 0.0 for v in od["g"].values()) and float(od["ds_t"].abs().max()) == 0.0 and float(od["dproj"].float().abs().max()) == 0.0
    ok = _embed_hip(t, ids, tt, B, L, V, H, p, seed, gy * keep)
    assert all(torch.equal(ok["g"][k], o["g"][k]) for k in o["g"]) and torch.equal(ok["ds_t"], o["ds_t"]) and torch.equal(ok["dproj"], o["dproj"])


@pytest.mark.parametrize("L", [37, 64])                      # S = 109, and S = 136: crosses the 128-row tile
def test_attention_joint_shapes_vs_torch(L):
    """VisualBERT attention (modeling_visual_bert.py:234-285): rows [V + 1, s') x keys [s', S) by clamp(w0), rows [s', S) x keys [s', S) by clamp(w1);
    a key mask that is NOT a prefix -- text padding in the middle of the key range, one masked 36-key region block, one example with every region
    key masked; forward, dq / dk / dv and d(w0) / d(w1).  Bounds: those of test_vilt_gpu.test_attention_row_lo_vs_torch."""
    from mkg_analogy_amd import ops
    torch.manual_seed(L)
    B, nh, D, V = 3, 12, 64, 72
    H, S = nh * D, L + V
    dev = "cuda"
    qkv = (torch.randn(B * S, 3 * H) * 0.5).to(torch.bfloat16)
    am = torch.ones(B, S, dtype=torch.int64)
    am[0, L - 5:L] = 0                                         # padded text keys: in the middle of the joint key range
    am[1, L - 9:L] = 0
    am[1, L + 36:] = 0                                         # the second entity's 36 regions masked
    am[2, L:] = 0                                              # no entity: every region key masked
    sep = torch.tensor([30, L - 12, 25]) + V                   # s' = sep_idx[:, 2] + V
    w = torch.tensor([0.3, 0.7])
    dctx = (torch.randn(B * S, H) * 0.5).to(torch.bfloat16)
    q, k, v = [qkv[:, i * H:(i + 1) * H].float().view(B, S, nh, D).transpose(1, 2).clone().requires_grad_(True) for i in range(3)]
    wr = w.clone().requires_grad_(True)
    sc = q @ k.transpose(-1, -2) / 8.0
    rows = torch.arange(S)[:, None]; keys = torch.arange(S)[None]
    fac = []
    for b in range(B):
        s_ = int(sep[b])
        f0 = ((rows >= V + 1) & (rows < s_) & (keys >= s_)).float()
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
              sep=sep.to(dev), sep_stride=1, w0=w0, w1=w1, rw_row_lo=V + 1)
    ops.attn_fwd(**kw)
    dqkv = torch.empty(B * S, 3 * H, device=dev, dtype=torch.bfloat16)
    dw = torch.zeros(2, device=dev)
    ops.attn_bwd(dctx=dctx.to(dev), delta=torch.empty(B, nh, S, device=dev), dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:], dw=dw, **kw)
    torch.cuda.synchronize()
    e = float((ctx.float().cpu() - ctx_ref.detach()).abs().max())
    print(f"\njoint attention S={S}: ctx max|err| {e:.3e}")
    assert e < 2e-2 * max(1.0, float(ctx_ref.abs().max())), e
    for i, t in enumerate((q, k, v)):
        r = t.grad.transpose(1, 2).reshape(B * S, H)
        got = dqkv[:, i * H:(i + 1) * H].float().cpu()
        rel = float((got - r).norm() / r.norm())
        print(f"   d{'qkv'[i]} rel-L2 {rel:.3e}")
        assert rel < 2e-2, ("qkv"[i], rel)
    # masked keys receive no gradient beyond the bf16 floor of exp(-10000) = 0, and the masked region block gets exactly none of the probability mass
    dk_full = dqkv[:, H:2 * H].float().cpu().view(B, S, H)
    assert float(dk_full[2, L:].abs().max()) == 0.0 and float(dk_full[1, L + 36:].abs().max()) == 0.0 and float(dk_full[0, L - 5:L].abs().max()) == 0.0
    rel_w = (dw.cpu() - wr.grad).abs() / wr.grad.abs().clamp_min(1e-3)
    assert float(rel_w.max()) < 2e-2, (dw.cpu(), wr.grad)
    # the fp32 evaluation kernel on the same inputs (engine_precise: mart_attn_fwd_f32 with rw_row_lo)
    q32 = qkv.float().to(dev)
    c32 = torch.empty(B * S, H, device=dev)
    ops.attn_fwd_f32(q=q32[:, :H], k=q32[:, H:2 * H], v=q32[:, 2 * H:], ctx=c32, B=B, nh=nh, D=64, Sq=S, Sk=S, scale=0.125, attn_mask=am.to(dev),
                     sep=sep.to(dev), sep_stride=1, w0=w0, w1=w1, rw_row_lo=V + 1, fast=True)
    torch.cuda.synchronize()
    e32 = float((c32.cpu() - ctx_ref.detach()).abs().max())
    print(f"   fp32 kernel: ctx max|err| {e32:.3e}")
    # two-term bf16 splits carry 2^-16 = 1.5e-5 relative precision per operand (q, k, v are exact here: bf16 inputs); the probabilities and the
    # P V accumulation add a few of those on values up to max|v|: 2e-4 of the output scale bounds it with room for the exp2 / rcp approximations
    assert e32 < 2e-4 * max(1.0, float(ctx_ref.abs().max())), e32


# ------------------------------------------------------------------ model vs the reference
def _model(alpha=0.43, lr=4e-5):
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.lit_models import TransformerLitModel
    from mkg_analogy_amd.models import VisualBertKGC, visual_bert_config
    torch.manual_seed(0)
    model = VisualBertKGC(visual_bert_config(vocab_size=30522))
    cfg = D.data_config(seed=1234)
    args = argparse.Namespace(label_smoothing=0.1, alpha=alpha, pretrain=0, lr=lr, weight_decay=0.01, optimizer="AdamW", warm_up_radio=0.1)
    lit = TransformerLitModel(model=model, args=args, tokenizer=D.FakeTokenizer(), data_config=cfg)      # resize -> 42006
    return model, lit, cfg


def _batch(B, L, batch_seed, feat_seed, vmask):
    from mkg_analogy_amd import data_synth as D
    from tools.gen_goldens_visualbert import region_features
    b = D.make_batch(B, L, image_size=2, seed=batch_seed)
    b["visual_attention_mask"] = vmask
    b["pixel_values"] = region_features(B, feat_seed, vmask)
    return b


_BUILT = {}


def _build(gold):
    """Model + lit model with the golden's weights and the golden's batch; built once per golden and shared (tests restore what they change)."""
    if gold in _BUILT:
        return _BUILT[gold]
    from tools.gen_goldens_visualbert import weights
    g = np.load(os.path.join(GOLD, gold))
    model, lit, cfg = _model(alpha=float(g["alpha"]))
    model.cuda()
    lit._init_relation_word()                                                                            # -> 42007
    sd = weights([(n, p.shape) for n, p in model.named_parameters()], cfg["analogy_relation_ids"])
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(("position_ids" in m or "decoder" in m) for m in missing), (missing, unexpected)
    batch = _batch(int(g["B"]), int(g["L"]), int(g["batch_seed"]), int(g["feat_seed"]), torch.from_numpy(g["visual_attention_mask"]))
    for k in ("input_ids", "attention_mask", "sep_idx", "rel_idx", "label"):
        assert np.array_equal(batch[k].numpy(), g["in::" + k]), k
    _BUILT[gold] = (model, lit, g, batch, cfg, sd)
    return _BUILT[gold]


@pytest.mark.parametrize("gold", ["g11_visualbert_real.npz", "g11b_visualbert_odd.npz"])
def test_visualbert_step_and_forward_vs_reference(gold):
    """The project's gates for a backbone against its golden (tests/test_vilt_gpu.py): bf16 mask logits within max(1e-2, 2 x the golden's
    bf16-weight control), trans rel-L2 < 4e-3, loss within 5e-3, gradients cosine > 0.99 and rel < 0.12 per sampled tensor and 0.12 per norm;
    fp32 path: logits <= 1e-3, trans < 5e-3, exact ranks.  d(key.bias) is a cancellation residue (zero for plain softmax attention: only the
    reweighted key block leaves one) and is judged on the scale of the same layer's d(query.bias), as the ViLT test does;
    test_attention_joint_shapes_vs_torch holds dK itself to fp32 torch at these shapes."""
    model, lit, g, batch, cfg, _ = _build(gold)
    B, L, V = int(g["B"]), int(g["L"]), int(g["V"])
    ids = torch.tensor(cfg["analogy_entity_ids"]).cuda()
    gb = {k: v.cuda() for k, v in batch.items()}
    before = {k: gb[k].clone() for k in ("sep_idx", "rel_idx", "q_head_idx", "a_head_idx")}
    model.eval()
    model.set_precision("bf16")
    st = model.store
    st.zero_grad()
    loss = lit.training_step(dict(gb), 1)
    loss.backward()
    torch.cuda.synchronize()
    assert all(torch.equal(gb[k], before[k]) for k in before)            # the reference shifts sep_idx in place; this path leaves the caller's tensors
    out, trans = model(**{k: gb[k] for k in KEYS}, return_dict=True)
    assert tuple(trans.shape) == (B, L + V, 768) and torch.equal(gb["sep_idx"], before["sep_idx"])
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
    print(f"\nvisualbert {gold}: loss hip {float(loss.detach()):.5f} ref {float(g['loss']):.5f}; trans rel-L2 {rel_t:.3e}; logits max|err| {e_l:.3e} "
          f"(gate {gate:.3e}, bf16-weight control {float(g['bf16_control_dev']):.3e})")
    assert e_l <= gate and rel_t < 4e-3 and dl < 5e-3
    names = [k[4:] for k in g.files if k.startswith("gs::")]
    assert len(names) >= 40
    gn = dict(zip([str(x) for x in g["grad_norm_names"]], g["grad_norm_vals"]))
    assert len(g["none_grad"]) == 0 and set(gn) == set(st.slots)

    def cancels(n):
        return n.endswith("attention.self.key.bias")
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
    # evaluation ranks in the training configuration (bf16): exact wherever the label's logit gap exceeds twice the measured error
    lab = ml_ref[torch.arange(B), torch.from_numpy(g["in::label"])]
    amb = ((ml_ref - lab[:, None]).abs() < 2 * e_l).sum(1).numpy() - 1
    ev = lit._eval(dict(gb), 0)
    assert np.all(np.abs(ev["entity_ranks"] - g["ranks"]) <= amb)
    # ---- fp32-accurate evaluation path (engine_precise.PreciseVisualBertForward)
    model.set_precision("fp32")
    with torch.no_grad():
        out32, trans32 = model(**{k: gb[k] for k in KEYS}, return_dict=True)
    ml32 = out32.logits[ar, mi][:, ids].float().cpu()
    e32 = float((ml32 - ml_ref).abs().max())
    t32 = float((trans32[ar[:, None], rows].float().cpu() - tr_ref).abs().max())
    print(f"   fp32 path: logits max|err| {e32:.3e}  trans rows max|err| {t32:.3e}")
    assert e32 <= 1e-3 and t32 < 5e-3
    model.set_precision("bf16")
    ev32 = lit._eval_at(dict(gb), 0)                          # the lit model's default evaluation precision: fp32
    assert model.precision == "bf16"
    gap = (ml_ref - lab[:, None]).abs()
    gap[torch.arange(B), torch.from_numpy(g["in::label"])] = 1e9
    safe = (gap.min(1).values > 2 * e32).numpy()             # exact ranks wherever no other entity's logit sits within twice the measured error of the label's
    assert safe.any()
    assert np.array_equal(ev32["entity_ranks"][safe], np.asarray(g["ranks"])[safe])
    with pytest.raises(NotImplementedError, match="verification mode"):
        model.set_precision("fp32")
        try:
            model(**{k: gb[k] for k in KEYS}, return_dict=True)          # grad enabled: fp32 training is not built
        finally:
            model.set_precision("bf16")


def test_visualbert_backward_bit_identical():
    model, lit, g, batch, cfg, _ = _build("g11b_visualbert_odd.npz")
    gb = {k: v.cuda() for k, v in batch.items()}
    model.eval()
    st = model.store
    outs = []
    for _ in range(2):
        st.zero_grad()
        loss = lit.training_step(dict(gb), 1)
        loss.backward()
        torch.cuda.synchronize()
        outs.append(st.grad.detach().clone())
    assert float(outs[0].abs().max()) > 0
    for n, s in st.slots.items():
        assert torch.equal(outs[0][s.offset:s.offset + s.numel], outs[1][s.offset:s.offset + s.numel]), n
    assert torch.equal(outs[0], outs[1])


def test_visualbert_fit_then_reload_through_the_lit_model():
    """Trainer.fit for 5 steps at B = 4, L = 37 in train mode (hidden and attention dropout on): finite losses, the last below the first.  Then
    the reference's reload (main.py: lit_model.load_state_dict of a ``model.``-prefixed checkpoint): the next evaluation forward equals that of
    a fresh model built from those weights, on the bf16 and on the fp32 path."""
    from mkg_analogy_amd.trainer import Trainer
    from tools.gen_goldens_visualbert import visual_mask, weights
    model, lit, cfg = _model(lr=2e-4)
    lit._init_relation_word()                                 # -> 42007 (on the host: no store yet)
    sd = weights([(n, p.shape) for n, p in model.named_parameters()], cfg["analogy_relation_ids"])
    model.load_state_dict(sd, strict=False)
    model.cuda()
    vm = visual_mask(4, False)
    vm[1, 36:] = 0.0
    b = _batch(4, 37, 99, 98, vm)
    batches = [{k: v.cuda() for k, v in b.items()} for _ in range(5)]           # the same batch five times: the loss must fall
    tr = Trainer(max_epochs=1, max_steps=5, world_size=1)
    losses, step = [], tr.train_step

    def rec(*a, **k):
        loss = step(*a, **k)
        losses.append(float(loss))
        return loss
    tr.train_step = rec
    tr.fit(lit, batches)
    print("\nvisualbert fit losses", losses)
    assert model.training and len(losses) == 5 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    st = model.store
    trained = {n: st.m(n).detach().cpu().clone() for n in st.slots}
    assert any(not torch.equal(trained[n], sd[n]) for n in sd)

    def ev(m):
        m.eval()
        gb, ids = batches[0], torch.tensor(cfg["analogy_entity_ids"], device="cuda")
        _, mi = (gb["input_ids"] == 103).nonzero(as_tuple=True)
        res = {}
        for prec in ("bf16", "fp32"):
            m.set_precision(prec)
            with torch.no_grad():
                o, trans = m(**{k: gb[k] for k in KEYS}, return_dict=True)
                res[prec] = (o.logits[torch.arange(4, device="cuda"), mi][:, ids].float().clone(), trans.float().clone())
        m.set_precision("bf16")
        return res
    moved = ev(model)
    r = lit.load_state_dict({"model." + k: v for k, v in sd.items()}, strict=False)
    assert not r.unexpected_keys and model.store is st
    got = ev(model)
    fresh, fresh_lit, _ = _model()
    fresh_lit._init_relation_word()
    fresh.load_state_dict(sd, strict=False)
    fresh.cuda()
    want = ev(fresh)
    for prec in ("bf16", "fp32"):
        assert torch.equal(got[prec][0], want[prec][0]) and torch.equal(got[prec][1], want[prec][1]), prec
        assert not torch.equal(got[prec][0], moved[prec][0]), prec
