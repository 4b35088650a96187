"""fp32-accurate forward of the MKGformer path (evaluation / parity mode; see csrc/precise.hip).

Same schedule as ``engine.UnimoEngine.forward`` (UnimoEncoder.forward, MarT/models/modeling_unimo.py:589-658, and the
functions it calls), but every activation stays in fp32 and every dense contraction runs through the bf16 MFMA GEMM on
two-term operand splits (K' = 3K: hi*hi + lo*hi + hi*lo, fp32 accumulation), attention and the image-text fusion in
plain fp32 FMA arithmetic (``mart_attn_fwd_f32``).  LayerNorm, embeddings, GELU / quick-GELU epilogues, bias and residual
adds are the fp32 code of the fast path.  The reference computes in fp32; this mode is how the
``1e-3 on logits / exact ranked indices`` gate of BASELINE.json is met.  Forward only, dropout off.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .params import FlatStore

BF, F32 = torch.bfloat16, torch.float32


def _e(shape, dtype, dev):
    return torch.empty(shape, device=dev, dtype=dtype)


class _PreciseBase:
    """Operand handling shared by the fp32-accurate forwards: cached weight splits, split-GEMM linear, fp32 LayerNorm, scoring."""
    st: FlatStore

    def _init_base(self, store: FlatStore):
        self.st = store
        self._w3: Dict[str, Tuple[int, torch.Tensor]] = {}
        # Error-budget hook (tools/error_budget.py, docs/LAB_r01-r05.md section 5): the components named here run with their operands ROUNDED TO BF16
        # (as the training path stores them) while everything else stays fp32-accurate, so the logit error each component class
        # contributes can be measured in isolation.  Tags: vis_lin, vis_attn, txt_lin_lo (layers < 8), txt_lin_hi, txt_attn,
        # fusion, head_t, head_s.  Empty in normal use.
        self.degrade: set = set()
        self.terms = 2                                   # bf16 terms per operand split: 2 (three products) everywhere but the verification-mode training step
        # evaluation passes: LayerNorm and the unmasked attention write the [hi | lo | hi] A operand of the GEMM that follows them directly (no
        # separate split pass over an f32 copy), and that attention runs on two-term splits itself (csrc/attention.hip attn_split_fwd_k)
        self.fused_split = os.environ.get("MART_PRECISE_FUSED_SPLIT", "1") == "1" and os.environ.get("MART_ATTN_F32_SPLIT", "1") == "1"

    def _pre(self) -> bool:
        return self.fused_split and self.terms == 2 and not self.degrade

    def _rb(self, x: torch.Tensor, tag: Optional[str]) -> torch.Tensor:
        return x.to(BF).to(F32) if tag is not None and tag in self.degrade else x


class PreciseUnimoForward(_PreciseBase):
    def __init__(self, store: FlatStore, vision_cfg, text_cfg):
        self._init_base(store)
        self.vc, self.tc = vision_cfg, text_cfg
        self.H, self.nh, self.I = text_cfg.hidden_size, text_cfg.num_attention_heads, text_cfg.intermediate_size
        self.n_layers = text_cfg.num_hidden_layers
        assert self.H // self.nh == 64
        self.eps_t, self.eps_v = float(text_cfg.layer_norm_eps), 1e-5
        self.fuse_from, self.export_from = 8, 7

    # ------------------------------------------------------------------ operands
    def w3(self, names: Sequence[str], rounded: bool = False) -> torch.Tensor:
        """[sum(out), 3*in] bf16 weight split (role 1) of one or several adjacent matrices, cached per store version."""
        key = names[0] + f"+{len(names)}" + ("~bf16" if rounded else "")
        ver = getattr(self.st, "version", 0)
        hit = self._w3.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1]
        W = self.st.fused(list(names), self.st.master)
        W = W.reshape(W.shape[0], -1)
        if rounded:
            W = W.to(BF).to(F32)
        out = ops.split_bf16x3(W, 1, terms=self.terms)
        self._w3[key] = (ver, out)
        return out

    def lin(self, x: torch.Tensor, wnames: Sequence[str], bnames: Optional[Sequence[str]], N: int, tag: Optional[str] = None, split3: bool = False,
            **epi) -> torch.Tensor:
        """f32 [M, N] = epilogue(x @ W^T + b) with x f32 [M, K] (or bf16 [M, 3K]: already the split operand).  ``split3``: the result as the bf16
        [M, 3N] operand of the next GEMM, written by the epilogue (256-wide tiles: N % 256 == 0 and at least half a round of them)."""
        split3 = split3 and N % 256 == 0 and x.shape[0] * N >= 128 * 256 * 256 and x.shape[0] > 128
        out = _e((x.shape[0], 3 * N), BF, x.device) if split3 else _e((x.shape[0], N), F32, x.device)
        if split3:
            epi = dict(epi, c_split3=True, tile_cfg=256)
        bias = self.st.fused(list(bnames), self.st.master) if bnames else None
        deg = tag is not None and tag in self.degrade
        a3 = x if x.dtype == BF else ops.split_bf16x3(self._rb(x, tag), 0, terms=self.terms)      # bf16 input: already the [hi | lo | hi] operand
        ops.gemm_nt(a3, self.w3(wnames, rounded=deg), out, bias=bias, **epi)
        return out

    def _ln(self, x, wname, bname, eps, split3: bool = False):
        """fp32 LayerNorm; ``split3``: return the bf16 [M, 3H] A operand of the GEMM that consumes it instead of the f32 tensor."""
        M, H = x.shape
        mean, rstd = _e((M,), F32, x.device), _e((M,), F32, x.device)
        y = _e((M, 3 * H), BF, x.device) if split3 else _e((M, H), F32, x.device)
        ops.ln_fwd(x_f32=x, gamma=self.st.m(wname), beta=self.st.m(bname), eps=eps, M=M, H=H, mean=mean, rstd=rstd,
                   out_f32=None if split3 else y, out_split3=y if split3 else None)
        return y

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, image_table=None, image_index=None):
        st, H, nh, I = self.st, self.H, self.nh, self.I
        dev = input_ids.device
        B, Lq = input_ids.shape
        S, p = self.vc.image_size, self.vc.patch_size
        P = (S // p) ** 2
        Nv = 1 + 2 * P
        Mv, Mt = B * Nv, B * Lq
        Kp = 3 * p * p
        # ---- vision embeddings (modeling_unimo.py:119-132,711)
        patches = _e((B * 2 * P, Kp), F32, dev)
        if image_index is not None:
            ops.patchify_f32(image_table, image_index.contiguous().view(-1), patches, B, S, p)
        else:
            ops.patchify_f32(pixel_values.contiguous(), None, patches, B, S, p)
        pe = self.lin(patches, ["unimo.vision_embeddings.patch_embedding.weight"], None, H)
        s_v = _e((Mv, H), F32, dev)
        ops.vision_assemble_f32(pe, st.m("unimo.vision_embeddings.class_embedding"), st.m("unimo.vision_embeddings.position_embedding.weight"),
                                s_v, B, P, H)
        xv = self._ln(s_v, "unimo.vision_pre_layrnorm.weight", "unimo.vision_pre_layrnorm.bias", self.eps_v)
        # ---- text embeddings (:152-186)
        u = "unimo.text_embeddings."
        s_t, tmean, trstd, xt = _e((Mt, H), F32, dev), _e((Mt,), F32, dev), _e((Mt,), F32, dev), _e((Mt, H), F32, dev)
        ops.text_embed_fwd(ids=input_ids, tt=token_type_ids, word=st.m(u + "word_embeddings.weight"), pos=st.m(u + "position_embeddings.weight"),
                           type_=st.m(u + "token_type_embeddings.weight"), gamma=st.m(u + "LayerNorm.weight"), beta=st.m(u + "LayerNorm.bias"),
                           eps=self.eps_t, p_drop=0.0, seed=0, B=B, Lq=Lq, H=H, s_out=s_t, mean=tmean, rstd=trstd, out_f32=xt, out_bf16=None)
        t_qkv_prev = None
        for l in range(self.n_layers):
            # ---- vision layer l (CLIPEncoderLayer.forward :490-527)
            v = f"unimo.encoder.vision_layers.{l}."
            pre3 = self._pre()
            h1 = self._ln(xv, v + "layer_norm1.weight", v + "layer_norm1.bias", self.eps_v, split3=pre3)
            names = [v + f"self_attn.{n}" for n in ("q_proj", "k_proj", "v_proj")]
            qkv = self._rb(self.lin(h1, [n + ".weight" for n in names], [n + ".bias" for n in names], 3 * H, tag="vis_lin"), "vis_attn")
            ctx = _e((Mv, 3 * H), BF, dev) if pre3 else _e((Mv, H), F32, dev)
            pre = t_qkv_prev if l >= self.fuse_from else None
            ops.attn_fwd_f32(q=qkv[:, :H], k=qkv[:, H:2 * H], v=qkv[:, 2 * H:], ctx=None if pre3 else ctx, ctx_split3=ctx if pre3 else None,
                             B=B, nh=nh, D=64, Sq=Nv, Sk=Nv, scale=0.125,
                             pk=pre[:, H:2 * H] if pre is not None else None, pv=pre[:, 2 * H:] if pre is not None else None,
                             Lp=Lq if pre is not None else 0, fast=True)          # evaluation pass: two-term splits on the bf16 matrix pipe
            ctx = self._rb(ctx, "vis_attn")
            x1 = self.lin(ctx, [v + "self_attn.out_proj.weight"], [v + "self_attn.out_proj.bias"], H, tag="vis_lin", res_f32=xv)
            h2 = self._ln(x1, v + "layer_norm2.weight", v + "layer_norm2.bias", self.eps_v, split3=pre3)
            f = self.lin(h2, [v + "mlp.fc1.weight"], [v + "mlp.fc1.bias"], I, tag="vis_lin", act=ops.ACT_QGELU, split3=pre3)
            xv = self.lin(f, [v + "mlp.fc2.weight"], [v + "mlp.fc2.bias"], H, tag="vis_lin", res_f32=x1)
            # ---- text layer l (BertLayer.forward :540-577)
            t = f"unimo.encoder.text_layer.{l}."
            names = [t + f"attention.self.{n}" for n in ("query", "key", "value")]
            tl = "txt_lin_hi" if l >= self.fuse_from else "txt_lin_lo"
            tqkv = self._rb(self.lin(xt, [n + ".weight" for n in names], [n + ".bias" for n in names], 3 * H, tag=tl), "txt_attn")
            tctx = _e((Mt, H), F32, dev) if (not pre3 or l >= self.fuse_from) else None     # the fusion op reads the f32 context
            tctx3 = _e((Mt, 3 * H), BF, dev) if pre3 else None                            # the output projection its split operand
            on = sep_idx is not None
            ops.attn_fwd_f32(q=tqkv[:, :H], k=tqkv[:, H:2 * H], v=tqkv[:, 2 * H:], ctx=tctx, ctx_split3=tctx3, B=B, nh=nh, D=64, Sq=Lq, Sk=Lq, scale=0.125,
                             attn_mask=attention_mask, sep=sep_idx[:, 2:] if on else None, sep_stride=sep_idx.shape[1] if on else 0,
                             w0=st.m(t + "attention.self.adaptive_weight.0") if on else None,
                             w1=st.m(t + "attention.self.adaptive_weight.1") if on else None, fast=True)
            if tctx is not None:
                tctx = self._rb(tctx, "txt_attn")
            fus = None
            if l >= self.fuse_from:                                  # BertFusion.forward :400-414 (unscaled, unmasked, one "head" of 768)
                fus = _e((Mt, H), F32, dev)
                xvf = self._rb(xv, "fusion")
                ops.attn_fwd_f32(q=self._rb(tctx, "fusion"), k=xvf, v=xvf, ctx=fus, B=B, nh=1, D=H, Sq=Lq, Sk=Nv, scale=1.0)
                fus = self._rb(fus, "fusion")
            s1 = self.lin(tctx3 if pre3 else tctx, [t + "attention.output.dense.weight"], [t + "attention.output.dense.bias"], H, tag=tl, res_f32=xt)
            a = self._ln(s1, t + "attention.output.LayerNorm.weight", t + "attention.output.LayerNorm.bias", self.eps_t)
            h3 = pre3 and Mt > 128 and Mt * I >= 128 * 256 * 256                 # the GELU epilogue writes output.dense's split operand (256-wide tiles)
            ht = _e((Mt, 3 * I), BF, dev) if h3 else _e((Mt, I), F32, dev)
            hkw = dict(c_split3=True, tile_cfg=256) if h3 else {}
            deg = tl in self.degrade
            a3 = ops.split_bf16x3(self._rb(a, tl), 0, terms=self.terms)
            if fus is not None:
                ops.gemm_nt(a3, self.w3([t + "intermediate.dense.weight"], rounded=deg), ht, A2=ops.split_bf16x3(self._rb(fus, tl), 0, terms=self.terms),
                            B2=self.w3([t + "intermediate.fusion_dense.weight"], rounded=deg), bias=st.m(t + "intermediate.dense.bias"),
                            bias2=st.m(t + "intermediate.fusion_dense.bias"), act=ops.ACT_GELU, **hkw)
            else:
                ops.gemm_nt(a3, self.w3([t + "intermediate.dense.weight"], rounded=deg), ht, bias=st.m(t + "intermediate.dense.bias"), act=ops.ACT_GELU, **hkw)
            s2 = self.lin(ht, [t + "output.dense.weight"], [t + "output.dense.bias"], H, tag=tl, res_f32=a)
            xt = self._ln(s2, t + "output.LayerNorm.weight", t + "output.LayerNorm.bias", self.eps_t)
            t_qkv_prev = tqkv if l >= self.export_from else None
        # ---- MLM head transform (:972-975)
        hp = "cls.predictions.transform."
        y = self.lin(xt, [hp + "dense.weight"], [hp + "dense.bias"], H, tag="head_t", act=ops.ACT_GELU)
        trans = self._ln(y, hp + "LayerNorm.weight", hp + "LayerNorm.bias", self.eps_t)
        return trans.view(B, Lq, H)

    @torch.no_grad()
    def score(self, trans: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, word_name: str, bias_name: str) -> torch.Tensor:
        """logits[rows][:, ids] of the tied decoder (:958) on split operands."""
        H = trans.shape[-1]
        t3 = ops.split_bf16x3(self._rb(trans.reshape(-1, H), "head_s"), 0, terms=self.terms)
        out = _e((rows.numel(), ids.numel()), F32, trans.device)
        ops.gemm_nt(t3, self.w3([word_name], rounded="head_s" in self.degrade), out, a_rows=rows, b_rows=ids, bias=self.st.m(bias_name), bias_by_brow=True)
        return out


for _name in ("w3", "lin", "_ln", "score"):
    setattr(_PreciseBase, _name, PreciseUnimoForward.__dict__[_name])


class PreciseUnimoTrain(PreciseUnimoForward):
    """fp32-accurate forward WITH saved activations + backward (verification mode behind ``set_precision("fp32")``).

    The reference trains in fp32 (scripts/run_finetune_mkgformer.sh: PL precision 32); the bf16 training path can only be held to it at
    bf16 tolerances (and on plain N(0,0.02) weights only relative to a control).  This engine produces gradients that can be held to the
    reference's at ~1e-3: every dense contraction -- forward, data gradient (K-concatenated splits through mart_gemm_nt) and weight gradient
    (row-stacked splits through mart_gemm_tn, contraction over 3M rows) -- on two-term bf16 operand splits with fp32 accumulation,
    attention / fusion / LayerNorm / activations in fp32 (csrc/precise.hip).  Same interface as ``engine.UnimoEngine`` (forward -> (trans,
    None, saved), backward(saved, dtrans) accumulating into FlatStore.grad).  Dropout is not replayed here: eval-mode gradients only (what
    the reference goldens G1 / G7 / G8 are).  Autograd of modeling_unimo.py:589-658 and everything it calls."""

    grad_ready = None
    grad_ready_async = None
    save_for_backward = True

    def __init__(self, store: FlatStore, vision_cfg, text_cfg):
        super().__init__(store, vision_cfg, text_cfg)
        self._w3t: Dict[str, Tuple[int, torch.Tensor]] = {}
        # three-term splits / six products (exact to ~2^-24): on chaotic weights (plain N(0,0.02): the unscaled fusion softmax) two-term
        # products (2^-16) leave the gradients 1e-2 from the reference's, three-term ones ~1e-3; MART_PRECISE_TERMS=2 for the faster form
        self.terms = int(os.environ.get("MART_PRECISE_TERMS", "3"))

    # ------------------------------------------------------------------ operands / building blocks
    def w3t(self, names: Sequence[str]) -> torch.Tensor:
        """[in, 3*sum(out)] split (role 1) of W^T: the B operand of the data-gradient product dx = dy @ W."""
        key = names[0] + f"+{len(names)}"
        ver = getattr(self.st, "version", 0)
        hit = self._w3t.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1]
        W = self.st.fused(list(names), self.st.master)
        W = W.reshape(W.shape[0], -1)
        out = ops.split_bf16x3(W.t().contiguous(), 1, terms=self.terms)
        self._w3t[key] = (ver, out)
        return out

    def _pad64(self, x: torch.Tensor) -> torch.Tensor:
        K = x.shape[1]
        if K % 64 == 0:
            return x
        out = torch.zeros((x.shape[0], (K + 63) // 64 * 64), device=x.device, dtype=x.dtype)
        out[:, :K].copy_(x)
        return out

    def lin_bwd(self, dy: torch.Tensor, x: torch.Tensor, wnames: Sequence[str], bnames: Optional[Sequence[str]], need_dx: bool = True):
        """dW += dy^T x, db += colsum(dy); returns dx = dy @ W (f32) unless ``need_dx`` is False."""
        st = self.st
        gW = st.fused(list(wnames), st.grad)
        ops.gemm_tn(ops.split_bf16x3_stack(dy, 0, terms=self.terms), ops.split_bf16x3_stack(x, 1, terms=self.terms), gW.view(gW.shape[0], -1))
        if bnames:
            ops.colsum_f32(dy, st.fused(list(bnames), st.grad))
        if not need_dx:
            return None
        dx = _e((dy.shape[0], x.shape[1]), F32, dy.device)
        ops.gemm_nt(ops.split_bf16x3(dy, 0, terms=self.terms), self.w3t(wnames), dx)
        return dx

    def _ln_s(self, x, wname, bname, eps):
        M, H = x.shape
        y, mean, rstd = _e((M, H), F32, x.device), _e((M,), F32, x.device), _e((M,), F32, x.device)
        ops.ln_fwd(x_f32=x, gamma=self.st.m(wname), beta=self.st.m(bname), eps=eps, M=M, H=H, mean=mean, rstd=rstd, out_f32=y)
        return y, (x, mean, rstd, wname, bname)

    def _ln_b(self, dy, saved, add=None):
        x, mean, rstd, wname, bname = saved
        M, H = x.shape
        ds = _e((M, H), F32, x.device)
        ops.ln_bwd(dy_f32=dy, s=x, mean=mean, rstd=rstd, gamma=self.st.m(wname), M=M, H=H, add_f32=add, ds_f32=ds,
                   dgamma=self.st.g(wname), dbeta=self.st.g(bname))
        return ds

    # ------------------------------------------------------------------ forward (saves what the backward pass reads)
    def forward(self, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, train=False, seed=0, image_table=None, image_index=None):
        if train and (float(self.tc.hidden_dropout_prob) > 0 or float(self.tc.attention_probs_dropout_prob) > 0):
            raise NotImplementedError("precision='fp32' training steps are the verification mode: call model.eval() (dropout is not replayed)")
        st, H, nh, I = self.st, self.H, self.nh, self.I
        dev = input_ids.device
        B, Lq = input_ids.shape
        S, p = self.vc.image_size, self.vc.patch_size
        P = (S // p) ** 2
        Nv = 1 + 2 * P
        Mv, Mt = B * Nv, B * Lq
        Kp = 3 * p * p
        sv: Dict[str, object] = dict(B=B, L=Lq, P=P, Nv=Nv, ids=input_ids, tt=token_type_ids, am=attention_mask, sep=sep_idx)
        patches = _e((B * 2 * P, Kp), F32, dev)
        if image_index is not None:
            ops.patchify_f32(image_table, image_index.contiguous().view(-1), patches, B, S, p)
        else:
            ops.patchify_f32(pixel_values.contiguous(), None, patches, B, S, p)
        pe = self.lin(patches, ["unimo.vision_embeddings.patch_embedding.weight"], None, H)
        s_v = _e((Mv, H), F32, dev)
        ops.vision_assemble_f32(pe, st.m("unimo.vision_embeddings.class_embedding"), st.m("unimo.vision_embeddings.position_embedding.weight"),
                                s_v, B, P, H)
        xv, sv["vpre"] = self._ln_s(s_v, "unimo.vision_pre_layrnorm.weight", "unimo.vision_pre_layrnorm.bias", self.eps_v)
        sv["patches"] = patches
        u = "unimo.text_embeddings."
        s_t, tmean, trstd, xt = _e((Mt, H), F32, dev), _e((Mt,), F32, dev), _e((Mt,), F32, dev), _e((Mt, H), F32, dev)
        ops.text_embed_fwd(ids=input_ids, tt=token_type_ids, word=st.m(u + "word_embeddings.weight"), pos=st.m(u + "position_embeddings.weight"),
                           type_=st.m(u + "token_type_embeddings.weight"), gamma=st.m(u + "LayerNorm.weight"), beta=st.m(u + "LayerNorm.bias"),
                           eps=self.eps_t, p_drop=0.0, seed=0, B=B, Lq=Lq, H=H, s_out=s_t, mean=tmean, rstd=trstd, out_f32=xt, out_bf16=None)
        sv["temb"] = (s_t, tmean, trstd, u + "LayerNorm.weight", u + "LayerNorm.bias")
        t_qkv_prev = None
        on = sep_idx is not None
        for l in range(self.n_layers):
            v = f"unimo.encoder.vision_layers.{l}."
            h1, ln1 = self._ln_s(xv, v + "layer_norm1.weight", v + "layer_norm1.bias", self.eps_v)
            qn = [v + f"self_attn.{n}" for n in ("q_proj", "k_proj", "v_proj")]
            qkv = self.lin(h1, [n + ".weight" for n in qn], [n + ".bias" for n in qn], 3 * H)
            ctx = _e((Mv, H), F32, dev)
            pre = t_qkv_prev if l >= self.fuse_from else None
            vkw = dict(q=qkv[:, :H], k=qkv[:, H:2 * H], v=qkv[:, 2 * H:], B=B, nh=nh, D=64, Sq=Nv, Sk=Nv, scale=0.125,
                       pk=pre[:, H:2 * H] if pre is not None else None, pv=pre[:, 2 * H:] if pre is not None else None,
                       Lp=Lq if pre is not None else 0)
            ops.attn_fwd_f32(ctx=ctx, **vkw)
            x1 = self.lin(ctx, [v + "self_attn.out_proj.weight"], [v + "self_attn.out_proj.bias"], H, res_f32=xv)
            h2, ln2 = self._ln_s(x1, v + "layer_norm2.weight", v + "layer_norm2.bias", self.eps_v)
            z = self.lin(h2, [v + "mlp.fc1.weight"], [v + "mlp.fc1.bias"], I)
            f = ops.act_f32(z, ops.ACT_QGELU)
            xv = self.lin(f, [v + "mlp.fc2.weight"], [v + "mlp.fc2.bias"], H, res_f32=x1)
            sv[f"v{l}"] = dict(ln1=ln1, h1=h1, qn=qn, vkw=vkw, ctx=ctx, ln2=ln2, h2=h2, z=z, f=f)
            t = f"unimo.encoder.text_layer.{l}."
            tn = [t + f"attention.self.{n}" for n in ("query", "key", "value")]
            tqkv = self.lin(xt, [n + ".weight" for n in tn], [n + ".bias" for n in tn], 3 * H)
            tctx = _e((Mt, H), F32, dev)
            tkw = dict(q=tqkv[:, :H], k=tqkv[:, H:2 * H], v=tqkv[:, 2 * H:], B=B, nh=nh, D=64, Sq=Lq, Sk=Lq, scale=0.125,
                       attn_mask=attention_mask, sep=sep_idx[:, 2:] if on else None, sep_stride=sep_idx.shape[1] if on else 0,
                       w0=st.m(t + "attention.self.adaptive_weight.0") if on else None,
                       w1=st.m(t + "attention.self.adaptive_weight.1") if on else None)
            ops.attn_fwd_f32(ctx=tctx, **tkw)
            fus = fkw = None
            if l >= self.fuse_from:
                fus = _e((Mt, H), F32, dev)
                fkw = dict(q=tctx, k=xv, v=xv, B=B, nh=1, D=H, Sq=Lq, Sk=Nv, scale=1.0)
                ops.attn_fwd_f32(ctx=fus, **fkw)
            s1 = self.lin(tctx, [t + "attention.output.dense.weight"], [t + "attention.output.dense.bias"], H, res_f32=xt)
            a, lna = self._ln_s(s1, t + "attention.output.LayerNorm.weight", t + "attention.output.LayerNorm.bias", self.eps_t)
            zt = _e((Mt, I), F32, dev)
            if fus is not None:
                ops.gemm_nt(ops.split_bf16x3(a, 0, terms=self.terms), self.w3([t + "intermediate.dense.weight"]), zt, A2=ops.split_bf16x3(fus, 0, terms=self.terms),
                            B2=self.w3([t + "intermediate.fusion_dense.weight"]), bias=st.m(t + "intermediate.dense.bias"),
                            bias2=st.m(t + "intermediate.fusion_dense.bias"))
            else:
                ops.gemm_nt(ops.split_bf16x3(a, 0, terms=self.terms), self.w3([t + "intermediate.dense.weight"]), zt, bias=st.m(t + "intermediate.dense.bias"))
            ht = ops.act_f32(zt, ops.ACT_GELU)
            s2 = self.lin(ht, [t + "output.dense.weight"], [t + "output.dense.bias"], H, res_f32=a)
            xo, lno = self._ln_s(s2, t + "output.LayerNorm.weight", t + "output.LayerNorm.bias", self.eps_t)
            sv[f"t{l}"] = dict(x=xt, tn=tn, tkw=tkw, tctx=tctx, fus=fus, fkw=fkw, lna=lna, a=a, zt=zt, ht=ht, lno=lno, exported=l >= self.export_from)
            xt = xo
            t_qkv_prev = tqkv if l >= self.export_from else None
        hp = "cls.predictions.transform."
        zh = self.lin(xt, [hp + "dense.weight"], [hp + "dense.bias"], H)
        y = ops.act_f32(zh, ops.ACT_GELU)
        trans, lnh = self._ln_s(y, hp + "LayerNorm.weight", hp + "LayerNorm.bias", self.eps_t)
        sv["head"] = (xt, zh, lnh)
        return trans.view(B, Lq, H), None, sv

    # ------------------------------------------------------------------ backward
    def backward(self, sv, dtrans: torch.Tensor) -> None:
        st, H, nh, I = self.st, self.H, self.nh, self.I
        dev = dtrans.device
        B, Lq, P, Nv = sv["B"], sv["L"], sv["P"], sv["Nv"]
        Mv, Mt = B * Nv, B * Lq
        hp = "cls.predictions.transform."
        xt_f, zh, lnh = sv["head"]
        dy = self._ln_b(dtrans.contiguous().view(Mt, H).to(F32), lnh)
        dzh = ops.act_bwd_f32(dy, zh, ops.ACT_GELU)
        dxt = self.lin_bwd(dzh, xt_f, [hp + "dense.weight"], [hp + "dense.bias"])
        dxv = torch.zeros((Mv, H), device=dev, dtype=F32)
        dpre_next = None                                       # k / v gradient blocks that vision layer l+1 left for text layer l
        for l in reversed(range(self.n_layers)):
            t = f"unimo.encoder.text_layer.{l}."
            s = sv[f"t{l}"]
            ds2 = self._ln_b(dxt, s["lno"])                    # gradient w.r.t. (output.dense(ht) + a)
            dht = self.lin_bwd(ds2, s["ht"], [t + "output.dense.weight"], [t + "output.dense.bias"])
            dzt = ops.act_bwd_f32(dht, s["zt"], ops.ACT_GELU)
            da = self.lin_bwd(dzt, s["a"], [t + "intermediate.dense.weight"], [t + "intermediate.dense.bias"])
            da.add_(ds2)                                       # residual branch of BertOutput (elementwise f32 add)
            ds1 = self._ln_b(da, s["lna"])                     # gradient w.r.t. (attention.output.dense(ctx) + x)
            dtctx = self.lin_bwd(ds1, s["tctx"], [t + "attention.output.dense.weight"], [t + "attention.output.dense.bias"])
            if s["fus"] is not None:
                dfus = self.lin_bwd(dzt, s["fus"], [t + "intermediate.fusion_dense.weight"], [t + "intermediate.fusion_dense.bias"])
                dqf = _e((Mt, H), F32, dev)
                ops.attn_bwd_f32(dctx=dfus, dq=dqf, dk=dxv, dv=dxv, **s["fkw"])          # d(visual) from both roles accumulates into the vision-stream gradient
                dtctx.add_(dqf)
            dtqkv = dpre_next if dpre_next is not None else torch.zeros((Mt, 3 * H), device=dev, dtype=F32)
            dpre_next = None
            on = s["tkw"]["sep"] is not None
            ops.attn_bwd_f32(dctx=dtctx, dq=dtqkv[:, :H], dk=dtqkv[:, H:2 * H], dv=dtqkv[:, 2 * H:],
                             dw=st.g(t + "attention.self.adaptive_weight.0") if on else None, **s["tkw"])
            dx = self.lin_bwd(dtqkv, s["x"], [n + ".weight" for n in s["tn"]], [n + ".bias" for n in s["tn"]])
            dx.add_(ds1)
            dxt = dx
            # ---- vision layer l
            v = f"unimo.encoder.vision_layers.{l}."
            s = sv[f"v{l}"]
            df = self.lin_bwd(dxv, s["f"], [v + "mlp.fc2.weight"], [v + "mlp.fc2.bias"])
            dz = ops.act_bwd_f32(df, s["z"], ops.ACT_QGELU)
            dh2 = self.lin_bwd(dz, s["h2"], [v + "mlp.fc1.weight"], [v + "mlp.fc1.bias"])
            dx1 = self._ln_b(dh2, s["ln2"], add=dxv)
            dctx = self.lin_bwd(dx1, s["ctx"], [v + "self_attn.out_proj.weight"], [v + "self_attn.out_proj.bias"])
            dqkv = torch.zeros((Mv, 3 * H), device=dev, dtype=F32)
            dpk = dpv = None
            if s["vkw"]["Lp"]:
                dpre_next = torch.zeros((Mt, 3 * H), device=dev, dtype=F32)
                dpk, dpv = dpre_next[:, H:2 * H], dpre_next[:, 2 * H:]
            ops.attn_bwd_f32(dctx=dctx, dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:], dpk=dpk, dpv=dpv, **s["vkw"])
            dh1 = self.lin_bwd(dqkv, s["h1"], [n + ".weight" for n in s["qn"]], [n + ".bias" for n in s["qn"]])
            dxv = self._ln_b(dh1, s["ln1"], add=dx1)
            sv[f"v{l}"] = sv[f"t{l}"] = None
        # ---- embeddings
        dse = self._ln_b(dxt, sv["temb"])
        u = "unimo.text_embeddings."
        ops.text_embed_scatter(dse, sv["ids"], sv["tt"], st.g(u + "word_embeddings.weight"), st.g(u + "position_embeddings.weight"),
                               st.g(u + "token_type_embeddings.weight"), B, Lq, H)
        dsv = self._ln_b(dxv, sv["vpre"])
        # assemble backward (modeling_unimo.py:119-132): token t of every example shares position row (t <= P ? t : t - P); class token = row 0
        ps = torch.zeros(Nv * H, device=dev, dtype=F32)
        ops.colsum_f32(dsv.view(B, Nv * H), ps)
        ps = ps.view(Nv, H)
        st.g("unimo.vision_embeddings.class_embedding").add_(ps[0])
        gp = st.g("unimo.vision_embeddings.position_embedding.weight")
        gp[0].add_(ps[0])
        gp[1:P + 1].add_(ps[1:P + 1] + ps[P + 1:])
        dpe = dsv.view(B, Nv, H)[:, 1:].reshape(B * 2 * P, H).contiguous()
        self.lin_bwd(dpe, sv["patches"], ["unimo.vision_embeddings.patch_embedding.weight"], None, need_dx=False)

    # ------------------------------------------------------------------ scoring head with gradients
    def score_train(self, trans: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, word_name: str, bias_name: str) -> torch.Tensor:
        return _PreciseScoreFn.apply(trans, rows, ids, self, word_name, bias_name)


class _PreciseScoreFn(torch.autograd.Function):
    """logits[rows][:, ids] of the tied decoder on split operands (modeling_unimo.py:958), with the fp32-accurate backward."""

    @staticmethod
    def forward(ctx, trans, rows, ids, eng, word_name, bias_name):
        ctx.eng, ctx.rows, ctx.ids, ctx.names, ctx.shape = eng, rows, ids, (word_name, bias_name), trans.shape
        ctx.trans = trans.detach()
        with torch.no_grad():
            return PreciseUnimoForward.score(eng, trans.detach(), rows, ids, word_name, bias_name)

    @staticmethod
    def backward(ctx, dlogits):
        eng, rows, ids = ctx.eng, ctx.rows, ctx.ids
        word_name, bias_name = ctx.names
        st = eng.st
        H = ctx.shape[-1]
        dev = dlogits.device
        dl = eng._pad64(dlogits.contiguous().to(F32))                        # [R, Ap], zero columns past A
        R, Ap = dl.shape
        A = ids.numel()
        Wg = torch.zeros((Ap, H), device=dev, dtype=F32)
        ops.gather_rows_f32(st.m(word_name), ids, Wg[:A])
        drows = _e((R, H), F32, dev)
        ops.gemm_nt(ops.split_bf16x3(dl, 0, terms=eng.terms), ops.split_bf16x3(Wg.t().contiguous(), 1, terms=eng.terms), drows)
        dtrans = torch.zeros(ctx.shape, device=dev, dtype=F32)
        ops.scatter_add_rows_f32(drows, rows, dtrans.view(-1, H))
        trows = _e((R, H), F32, dev)
        ops.gather_rows_f32(ctx.trans.reshape(-1, H), rows, trows)
        ops.gemm_tn(ops.split_bf16x3_stack(dl, 0, terms=eng.terms), ops.split_bf16x3_stack(trows, 1, terms=eng.terms), st.g(word_name), NX=A, out_rows=ids)
        db = torch.zeros(Ap, device=dev, dtype=F32)
        ops.colsum_f32(dl, db)
        st.g(bias_name).index_add_(0, ids.long(), db[:A])
        return dtrans, None, None, None, None, None


class PreciseFlavaForward(_PreciseBase):
    """fp32-accurate twin of ``flava_engine.FlavaEngine.forward`` (MarT/models/modeling_flava.py:1373-1476, :2150-2204;
    SURVEY 8(a) row 19): three pre-LN stacks (image 1+P+P tokens with the tail-position quirk, text with the FLAVA variant
    of the adaptive reweight -- query row 0 exempt --, multimodal over 1 + image + text tokens without a mask), the two
    *_to_mm projections of the pre-final-layernorm streams, final multimodal layernorm, MLM head transform."""

    def __init__(self, store: FlatStore, config):
        self._init_base(store)
        self.cfg = config
        tc, ic, mc = config.text_config, config.image_config, config.multimodal_config
        self.H, self.nh, self.I = tc.hidden_size, tc.num_attention_heads, tc.intermediate_size
        assert self.H // self.nh == 64
        self.nt, self.ni, self.nm = tc.num_hidden_layers, ic.num_hidden_layers, mc.num_hidden_layers
        self.eps = float(tc.layer_norm_eps)

    def _block(self, p: str, x: torch.Tensor, B: int, S: int, **attn):
        """FlavaLayer.forward (:635-665): x + Attn(LN x); x + MLP(LN x)."""
        H, I = self.H, self.I
        a = p + "attention.attention."
        pre3 = self._pre()
        c3 = pre3                                        # the attention writes the output projection's operand itself
        h1 = self._ln(x, p + "layernorm_before.weight", p + "layernorm_before.bias", self.eps, split3=pre3)
        qkv = self.lin(h1, [a + f"{n}.weight" for n in ("query", "key", "value")], [a + f"{n}.bias" for n in ("query", "key", "value")], 3 * H)
        ctx = _e((x.shape[0], 3 * H), BF, x.device) if c3 else _e((x.shape[0], H), F32, x.device)
        ops.attn_fwd_f32(q=qkv[:, :H], k=qkv[:, H:2 * H], v=qkv[:, 2 * H:], ctx=None if c3 else ctx, ctx_split3=ctx if c3 else None,
                         B=B, nh=self.nh, D=64, Sq=S, Sk=S, scale=0.125, fast=True, **attn)
        x1 = self.lin(ctx, [p + "attention.output.dense.weight"], [p + "attention.output.dense.bias"], H, res_f32=x)
        h2 = self._ln(x1, p + "layernorm_after.weight", p + "layernorm_after.bias", self.eps, split3=pre3)
        f = self.lin(h2, [p + "intermediate.dense.weight"], [p + "intermediate.dense.bias"], I, act=ops.ACT_GELU, split3=pre3)
        return self.lin(f, [p + "output.dense.weight"], [p + "output.dense.bias"], H, res_f32=x1)

    @torch.no_grad()
    def forward(self, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, image_table=None, image_index=None):
        st, H = self.st, self.H
        dev = input_ids.device
        B, Lq = input_ids.shape
        ic = self.cfg.image_config
        S, p = ic.image_size, ic.patch_size
        P = (S // p) ** 2
        Nv = 1 + 2 * P
        Sm = 1 + Nv + Lq
        Mi, Mt, Mm = B * Nv, B * Lq, B * Sm
        Kp = 3 * p * p
        # ---- image embeddings (:308-343) + stack
        patches = _e((B * 2 * P, Kp), F32, dev)
        if image_index is not None:
            ops.patchify_f32(image_table, image_index.contiguous().view(-1), patches, B, S, p)
        else:
            ops.patchify_f32(pixel_values.contiguous(), None, patches, B, S, p)
        e = "flava.image_model.embeddings."
        pe = self.lin(patches, [e + "patch_embeddings.projection.weight"], [e + "patch_embeddings.projection.bias"], H)
        xi = _e((Mi, H), F32, dev)
        ops.vision_assemble_f32(pe, st.m(e + "cls_token"), st.m(e + "position_embeddings"), xi, B, P, H, tail_shift=1)
        for l in range(self.ni):
            xi = self._block(f"flava.image_model.encoder.layer.{l}.", xi, B, Nv)
        # ---- text embeddings (:406-438) + stack (reweight variant :494-496)
        t = "flava.text_model.embeddings."
        s_t, tmean, trstd, xt = _e((Mt, H), F32, dev), _e((Mt,), F32, dev), _e((Mt,), F32, dev), _e((Mt, H), F32, dev)
        ops.text_embed_fwd(ids=input_ids, tt=token_type_ids, word=st.m(t + "word_embeddings.weight"), pos=st.m(t + "position_embeddings.weight"),
                           type_=st.m(t + "token_type_embeddings.weight"), gamma=st.m(t + "LayerNorm.weight"), beta=st.m(t + "LayerNorm.bias"),
                           eps=self.eps, p_drop=0.0, seed=0, B=B, Lq=Lq, H=H, s_out=s_t, mean=tmean, rstd=trstd, out_f32=xt, out_bf16=None)
        on = sep_idx is not None
        for l in range(self.nt):
            pfx = f"flava.text_model.encoder.layer.{l}."
            a = pfx + "attention.attention."
            xt = self._block(pfx, xt, B, Lq, attn_mask=attention_mask, sep=sep_idx[:, 2:] if on else None,
                             sep_stride=sep_idx.shape[1] if on else 0, w0=st.m(a + "adaptive_weight.0") if on else None,
                             w1=st.m(a + "adaptive_weight.1") if on else None, rw_skip_row0=True)
        # ---- multimodal input [cls | image_to_mm(img) | text_to_mm(txt)] (:1430,1450,1455-1456) + stack (no mask :1456)
        xm = _e((B, Sm, H), F32, dev)
        xm[:, 0, :].copy_(st.m("flava.multimodal_model.cls_token").view(1, H))
        ops.gemm_nt(ops.split_bf16x3(xi, 0, terms=self.terms), self.w3(["flava.image_to_mm_projection.weight"]), xm[0, 1:],
                    bias=st.m("flava.image_to_mm_projection.bias"), M=Nv, batch=B, stride_a=Nv * 3 * H, stride_c=Sm * H)
        ops.gemm_nt(ops.split_bf16x3(xt, 0, terms=self.terms), self.w3(["flava.text_to_mm_projection.weight"]), xm[0, 1 + Nv:],
                    bias=st.m("flava.text_to_mm_projection.bias"), M=Lq, batch=B, stride_a=Lq * 3 * H, stride_c=Sm * H)
        xm = xm.view(Mm, H)
        for l in range(self.nm):
            xm = self._block(f"flava.multimodal_model.encoder.layer.{l}.", xm, B, Sm)
        # ---- final layernorm, text positions, MLM head transform (:1209, :2187-2188, :1676-1680)
        mm = self._ln(xm, "flava.multimodal_model.layernorm.weight", "flava.multimodal_model.layernorm.bias", self.eps)
        rows = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] * Sm + (1 + Nv) +
                torch.arange(Lq, device=dev, dtype=torch.int32)[None]).reshape(-1).contiguous()
        y = _e((Mt, H), F32, dev)
        ops.gemm_nt(ops.split_bf16x3(mm, 0, terms=self.terms), self.w3(["cls.transform.dense.weight"]), y, a_rows=rows, bias=st.m("cls.transform.dense.bias"),
                    act=ops.ACT_GELU)
        trans = self._ln(y, "cls.transform.LayerNorm.weight", "cls.transform.LayerNorm.bias", self.eps)
        return trans.view(B, Lq, H)


class PreciseFlavaTrain(PreciseFlavaForward):
    """fp32-accurate FLAVA forward WITH saved activations + backward (verification mode behind ``set_precision("fp32")`` with gradients enabled):
    the FLAVA twin of ``PreciseUnimoTrain``, built from the same pieces -- every contraction on three-term bf16 operand splits (six products, fp32
    accumulation), attention / LayerNorm / GELU and their gradients in fp32.  Autograd of MarT/models/modeling_flava.py:1373-1476 (FlavaModel.forward),
    :635-665 (FlavaLayer), :460-496 (self-attention with the row-0-exempt adaptive reweight), :2150-2204 (FlavaForMaskedLM.forward).  Same interface as
    ``flava_engine.FlavaEngine``; eval-mode gradients (all FLAVA dropouts are 0 in this configuration anyway)."""

    grad_ready = None
    grad_ready_async = None
    save_for_backward = True
    head_split = True
    w3t = PreciseUnimoTrain.w3t
    _pad64 = PreciseUnimoTrain._pad64
    lin_bwd = PreciseUnimoTrain.lin_bwd
    _ln_s = PreciseUnimoTrain._ln_s
    _ln_b = PreciseUnimoTrain._ln_b
    score = PreciseUnimoForward.score
    w3 = PreciseUnimoForward.w3
    lin = PreciseUnimoForward.lin

    def __init__(self, store: FlatStore, config):
        super().__init__(store, config)
        self._w3t: Dict[str, Tuple[int, torch.Tensor]] = {}
        self.terms = int(os.environ.get("MART_PRECISE_TERMS", "3"))

    def _block_s(self, p: str, x: torch.Tensor, B: int, S: int, **attn):
        H, I = self.H, self.I
        a = p + "attention.attention."
        h1, ln1 = self._ln_s(x, p + "layernorm_before.weight", p + "layernorm_before.bias", self.eps)
        qn = [a + n for n in ("query", "key", "value")]
        qkv = self.lin(h1, [n + ".weight" for n in qn], [n + ".bias" for n in qn], 3 * H)
        ctx = _e((x.shape[0], H), F32, x.device)
        kw = dict(q=qkv[:, :H], k=qkv[:, H:2 * H], v=qkv[:, 2 * H:], B=B, nh=self.nh, D=64, Sq=S, Sk=S, scale=0.125, **attn)
        ops.attn_fwd_f32(ctx=ctx, **kw)
        x1 = self.lin(ctx, [p + "attention.output.dense.weight"], [p + "attention.output.dense.bias"], H, res_f32=x)
        h2, ln2 = self._ln_s(x1, p + "layernorm_after.weight", p + "layernorm_after.bias", self.eps)
        z = self.lin(h2, [p + "intermediate.dense.weight"], [p + "intermediate.dense.bias"], I)
        f = ops.act_f32(z, ops.ACT_GELU)
        out = self.lin(f, [p + "output.dense.weight"], [p + "output.dense.bias"], H, res_f32=x1)
        return out, dict(ln1=ln1, h1=h1, qn=qn, kw=kw, ctx=ctx, ln2=ln2, h2=h2, z=z, f=f)

    def _block_b(self, p: str, s: dict, dx: torch.Tensor, dw=None) -> torch.Tensor:
        """d(loss)/d(block output) -> d(loss)/d(block input); parameter gradients accumulate into FlatStore.grad."""
        H = self.H
        df = self.lin_bwd(dx, s["f"], [p + "output.dense.weight"], [p + "output.dense.bias"])
        dz = ops.act_bwd_f32(df, s["z"], ops.ACT_GELU)
        dh2 = self.lin_bwd(dz, s["h2"], [p + "intermediate.dense.weight"], [p + "intermediate.dense.bias"])
        dx1 = self._ln_b(dh2, s["ln2"], add=dx)
        dctx = self.lin_bwd(dx1, s["ctx"], [p + "attention.output.dense.weight"], [p + "attention.output.dense.bias"])
        dqkv = torch.zeros((dx.shape[0], 3 * H), device=dx.device, dtype=F32)
        ops.attn_bwd_f32(dctx=dctx, dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:], dw=dw, **s["kw"])
        dh1 = self.lin_bwd(dqkv, s["h1"], [n + ".weight" for n in s["qn"]], [n + ".bias" for n in s["qn"]])
        return self._ln_b(dh1, s["ln1"], add=dx1)

    def forward(self, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, train=False, seed=0, image_table=None, image_index=None):
        st, H = self.st, self.H
        dev = input_ids.device
        B, Lq = input_ids.shape
        ic = self.cfg.image_config
        S, p = ic.image_size, ic.patch_size
        P = (S // p) ** 2
        Nv = 1 + 2 * P
        Sm = 1 + Nv + Lq
        Mi, Mt, Mm = B * Nv, B * Lq, B * Sm
        Kp = 3 * p * p
        sv: Dict[str, object] = dict(B=B, L=Lq, P=P, Nv=Nv, Sm=Sm, ids=input_ids, tt=token_type_ids)
        patches = _e((B * 2 * P, Kp), F32, dev)
        if image_index is not None:
            ops.patchify_f32(image_table, image_index.contiguous().view(-1), patches, B, S, p)
        else:
            ops.patchify_f32(pixel_values.contiguous(), None, patches, B, S, p)
        e = "flava.image_model.embeddings."
        pe = self.lin(patches, [e + "patch_embeddings.projection.weight"], [e + "patch_embeddings.projection.bias"], H)
        xi = _e((Mi, H), F32, dev)
        ops.vision_assemble_f32(pe, st.m(e + "cls_token"), st.m(e + "position_embeddings"), xi, B, P, H, tail_shift=1)
        sv["patches"] = patches
        taps = getattr(self, "taps", None)                    # tests: per-layer outputs (golden G9b)
        for l in range(self.ni):
            xi, sv[f"i{l}"] = self._block_s(f"flava.image_model.encoder.layer.{l}.", xi, B, Nv)
            if taps is not None:
                taps[f"i{l}"] = xi.view(B, Nv, H).clone()
        t = "flava.text_model.embeddings."
        s_t, tmean, trstd, xt = _e((Mt, H), F32, dev), _e((Mt,), F32, dev), _e((Mt,), F32, dev), _e((Mt, H), F32, dev)
        ops.text_embed_fwd(ids=input_ids, tt=token_type_ids, word=st.m(t + "word_embeddings.weight"), pos=st.m(t + "position_embeddings.weight"),
                           type_=st.m(t + "token_type_embeddings.weight"), gamma=st.m(t + "LayerNorm.weight"), beta=st.m(t + "LayerNorm.bias"),
                           eps=self.eps, p_drop=0.0, seed=0, B=B, Lq=Lq, H=H, s_out=s_t, mean=tmean, rstd=trstd, out_f32=xt, out_bf16=None)
        sv["temb"] = (s_t, tmean, trstd, t + "LayerNorm.weight", t + "LayerNorm.bias")
        on = sep_idx is not None
        for l in range(self.nt):
            pfx = f"flava.text_model.encoder.layer.{l}."
            a = pfx + "attention.attention."
            xt, sv[f"t{l}"] = self._block_s(pfx, xt, B, Lq, attn_mask=attention_mask, sep=sep_idx[:, 2:] if on else None,
                                            sep_stride=sep_idx.shape[1] if on else 0, w0=st.m(a + "adaptive_weight.0") if on else None,
                                            w1=st.m(a + "adaptive_weight.1") if on else None, rw_skip_row0=True)
            if taps is not None:
                taps[f"t{l}"] = xt.view(B, Lq, H).clone()
        sv["xi"], sv["xt"], sv["on"] = xi, xt, on
        xm = _e((B, Sm, H), F32, dev)
        xm[:, 0, :].copy_(st.m("flava.multimodal_model.cls_token").view(1, H))
        T = 3 if self.terms == 2 else 6
        ops.gemm_nt(ops.split_bf16x3(xi, 0, terms=self.terms), self.w3(["flava.image_to_mm_projection.weight"]), xm[0, 1:],
                    bias=st.m("flava.image_to_mm_projection.bias"), M=Nv, batch=B, stride_a=Nv * T * H, stride_c=Sm * H)
        ops.gemm_nt(ops.split_bf16x3(xt, 0, terms=self.terms), self.w3(["flava.text_to_mm_projection.weight"]), xm[0, 1 + Nv:],
                    bias=st.m("flava.text_to_mm_projection.bias"), M=Lq, batch=B, stride_a=Lq * T * H, stride_c=Sm * H)
        xm = xm.view(Mm, H)
        for l in range(self.nm):
            xm, sv[f"m{l}"] = self._block_s(f"flava.multimodal_model.encoder.layer.{l}.", xm, B, Sm)
            if taps is not None:
                taps[f"m{l}"] = xm.view(B, Sm, H).clone()
        mm, lnm = self._ln_s(xm, "flava.multimodal_model.layernorm.weight", "flava.multimodal_model.layernorm.bias", self.eps)
        rows = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] * Sm + (1 + Nv) +
                torch.arange(Lq, device=dev, dtype=torch.int32)[None]).reshape(-1).contiguous()
        seq = _e((Mt, H), F32, dev)
        ops.gather_rows_f32(mm, rows, seq)
        zh = self.lin(seq, ["cls.transform.dense.weight"], ["cls.transform.dense.bias"], H)
        y = ops.act_f32(zh, ops.ACT_GELU)
        trans, lnh = self._ln_s(y, "cls.transform.LayerNorm.weight", "cls.transform.LayerNorm.bias", self.eps)
        sv["head"] = (seq, zh, lnh, lnm, rows)
        return trans.view(B, Lq, H), None, sv

    def backward(self, sv, dtrans: torch.Tensor) -> None:
        st, H = self.st, self.H
        dev = dtrans.device
        B, Lq, P, Nv, Sm = sv["B"], sv["L"], sv["P"], sv["Nv"], sv["Sm"]
        Mi, Mt, Mm = B * Nv, B * Lq, B * Sm
        seq, zh, lnh, lnm, rows = sv["head"]
        dy = self._ln_b(dtrans.contiguous().view(Mt, H).to(F32), lnh)
        dzh = ops.act_bwd_f32(dy, zh, ops.ACT_GELU)
        dseq = self.lin_bwd(dzh, seq, ["cls.transform.dense.weight"], ["cls.transform.dense.bias"])
        dmm = torch.zeros((Mm, H), device=dev, dtype=F32)
        ops.scatter_add_rows_f32(dseq, rows, dmm)
        dx = self._ln_b(dmm, lnm)
        for l in reversed(range(self.nm)):
            dx = self._block_b(f"flava.multimodal_model.encoder.layer.{l}.", sv[f"m{l}"], dx)
            sv[f"m{l}"] = None
        dx3 = dx.view(B, Sm, H)
        st.g("flava.multimodal_model.cls_token").view(H).add_(dx3[:, 0, :].sum(0))
        dpi = dx3[:, 1:1 + Nv].reshape(Mi, H).contiguous()
        dpt = dx3[:, 1 + Nv:].reshape(Mt, H).contiguous()
        dxi = self.lin_bwd(dpi, sv["xi"], ["flava.image_to_mm_projection.weight"], ["flava.image_to_mm_projection.bias"])
        dxt = self.lin_bwd(dpt, sv["xt"], ["flava.text_to_mm_projection.weight"], ["flava.text_to_mm_projection.bias"])
        for l in reversed(range(self.nt)):
            pfx = f"flava.text_model.encoder.layer.{l}."
            dw = st.g(pfx + "attention.attention.adaptive_weight.0") if sv["on"] else None
            dxt = self._block_b(pfx, sv[f"t{l}"], dxt, dw=dw)
            sv[f"t{l}"] = None
        dse = self._ln_b(dxt, sv["temb"])
        t = "flava.text_model.embeddings."
        ops.text_embed_scatter(dse, sv["ids"], sv["tt"], st.g(t + "word_embeddings.weight"), st.g(t + "position_embeddings.weight"),
                               st.g(t + "token_type_embeddings.weight"), B, Lq, H)
        for l in reversed(range(self.ni)):
            dxi = self._block_b(f"flava.image_model.encoder.layer.{l}.", sv[f"i{l}"], dxi)
            sv[f"i{l}"] = None
        # assemble backward (FlavaImageEmbeddings :308-343): cls token = row 0; position rows: first image 1..P, second image 0..P-1 (the tail quirk)
        e = "flava.image_model.embeddings."
        ps = torch.zeros(Nv * H, device=dev, dtype=F32)
        ops.colsum_f32(dxi.view(B, Nv * H), ps)
        ps = ps.view(Nv, H)
        st.g(e + "cls_token").view(H).add_(ps[0])
        gp = st.g(e + "position_embeddings").view(-1, H)
        gp[0].add_(ps[0])
        gp[1:P + 1].add_(ps[1:P + 1])
        gp[0:P].add_(ps[P + 1:])
        dpe = dxi.view(B, Nv, H)[:, 1:].reshape(B * 2 * P, H).contiguous()
        self.lin_bwd(dpe, sv["patches"], [e + "patch_embeddings.projection.weight"], [e + "patch_embeddings.projection.bias"], need_dx=False)

    def score_train(self, trans: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, word_name: str, bias_name: str) -> torch.Tensor:
        return _PreciseScoreFn.apply(trans, rows, ids, self, word_name, bias_name)


class PreciseViltForward(_PreciseBase):
    """fp32-accurate twin of ``vilt_engine.ViltEngine.forward`` (MarT/models/modeling_vilt.py:760-869, :914-968) for evaluation passes: the joint
    embedding (csrc/vilt.hip, f32 patch projection on split operands), 12 blocks of ``PreciseFlavaForward._block`` with the ViLT reweight rows
    (``rw_row_lo``), final layernorm, MLM head transform on the text rows."""

    _block = PreciseFlavaForward._block

    def __init__(self, store: FlatStore, config):
        self._init_base(store)
        self.cfg = config
        self.H, self.nh, self.I = config.hidden_size, config.num_attention_heads, config.intermediate_size
        assert self.H // self.nh == 64
        self.nl = config.num_hidden_layers
        self.eps = float(config.layer_norm_eps)
        self.n_tpos = int(config.max_position_embeddings)

    @torch.no_grad()
    def forward(self, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, patch_order, image_table=None, image_index=None):
        st, H = self.st, self.H
        dev = input_ids.device
        B, L = input_ids.shape
        S_img, p = self.cfg.image_size, self.cfg.patch_size
        P = (S_img // p) ** 2
        ni = 2 * (1 + P)
        S = L + ni
        Kp = 3 * p * p
        patches = _e((B * 2 * P, Kp), F32, dev)
        if image_index is not None:
            ops.patchify_f32(image_table, image_index.contiguous().view(-1), patches, B, S_img, p)
        else:
            ops.patchify_f32(pixel_values.contiguous(), None, patches, B, S_img, p)
        e, t = "vilt.embeddings.", "vilt.embeddings.text_embeddings."
        pe = self.lin(patches, [e + "patch_embeddings.projection.weight"], [e + "patch_embeddings.projection.bias"], H)
        del patches
        x = _e((B * S, H), F32, dev)
        ops.vilt_embed_fwd(ids=input_ids, tt=token_type_ids, word=st.m(t + "word_embeddings.weight"), tpos=st.m(t + "position_embeddings.weight"),
                           ttype=st.m(t + "token_type_embeddings.weight"), gamma=st.m(t + "LayerNorm.weight"), beta=st.m(t + "LayerNorm.bias"),
                           eps=self.eps, n_tpos=self.n_tpos, patch_f32=pe, cls=st.m(e + "cls_token"), ipos=st.m(e + "position_embeddings"),
                           modality=st.m(e + "token_type_embeddings.weight"), perm=patch_order.to(device=dev, dtype=torch.int32).contiguous(),
                           B=B, L=L, P=P, H=H, x=x, s_text=_e((B * L, H), F32, dev), mean=_e((B * L,), F32, dev), rstd=_e((B * L,), F32, dev))
        from .vilt_engine import vilt_mask_and_sep
        mask, sep = vilt_mask_and_sep(attention_mask, sep_idx, ni)
        for l in range(self.nl):
            pfx = f"vilt.encoder.layer.{l}."
            a = pfx + "attention.attention."
            x = self._block(pfx, x, B, S, attn_mask=mask, sep=sep, sep_stride=1, w0=st.m(a + "adaptive_weight.0"), w1=st.m(a + "adaptive_weight.1"),
                            rw_row_lo=ni + 1)
        xl = self._ln(x, "vilt.layernorm.weight", "vilt.layernorm.bias", self.eps)
        rows = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] * S + torch.arange(L, device=dev, dtype=torch.int32)[None]).reshape(-1).contiguous()
        y = _e((B * L, H), F32, dev)
        ops.gemm_nt(ops.split_bf16x3_rows(xl, rows, 0, terms=self.terms), self.w3(["mlm_score.transform.dense.weight"]), y,
                    bias=st.m("mlm_score.transform.dense.bias"), act=ops.ACT_GELU)
        trans = self._ln(y, "mlm_score.transform.LayerNorm.weight", "mlm_score.transform.LayerNorm.bias", self.eps)
        return trans.view(B, L, H)


class PreciseVisualBertForward(_PreciseBase):
    """fp32-accurate twin of ``visual_bert_engine.VisualBertEngine.forward`` (MarT/models/modeling_visual_bert.py:854-911, :1664-1723) for
    evaluation passes: the visual projection on split operands, the joint embedding (csrc/visual_bert.hip, dropout off), 12 post-LN blocks with
    the VisualBERT reweight rows (``rw_row_lo``) and the joint, non-prefix key mask, MLM head transform on all S rows."""

    def __init__(self, store: FlatStore, config):
        self._init_base(store)
        self.cfg = config
        self.H, self.nh, self.I = config.hidden_size, config.num_attention_heads, config.intermediate_size
        assert self.H // self.nh == 64
        self.nl = config.num_hidden_layers
        self.eps = float(config.layer_norm_eps)

    def _block(self, p: str, x: torch.Tensor, B: int, S: int, **attn):
        """VisualBertLayer.forward: LN(x + dense(Attn(x))); LN(a + dense(GELU(dense(a))))."""
        H, I = self.H, self.I
        a_ = p + "attention.self."
        pre3 = self._pre()
        qkv = self.lin(x, [a_ + f"{n}.weight" for n in ("query", "key", "value")], [a_ + f"{n}.bias" for n in ("query", "key", "value")], 3 * H)
        ctx = _e((x.shape[0], 3 * H), BF, x.device) if pre3 else _e((x.shape[0], H), F32, x.device)
        ops.attn_fwd_f32(q=qkv[:, :H], k=qkv[:, H:2 * H], v=qkv[:, 2 * H:], ctx=None if pre3 else ctx, ctx_split3=ctx if pre3 else None,
                         B=B, nh=self.nh, D=64, Sq=S, Sk=S, scale=0.125, fast=True, **attn)
        s1 = self.lin(ctx, [p + "attention.output.dense.weight"], [p + "attention.output.dense.bias"], H, res_f32=x)
        a = self._ln(s1, p + "attention.output.LayerNorm.weight", p + "attention.output.LayerNorm.bias", self.eps)
        f = self.lin(a, [p + "intermediate.dense.weight"], [p + "intermediate.dense.bias"], I, act=ops.ACT_GELU, split3=pre3)
        s2 = self.lin(f, [p + "output.dense.weight"], [p + "output.dense.bias"], H, res_f32=a)
        return self._ln(s2, p + "output.LayerNorm.weight", p + "output.LayerNorm.bias", self.eps)

    @torch.no_grad()
    def forward(self, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, visual_attention_mask=None):
        from .visual_bert_engine import EMB, HEAD, VPROJ, WORD, vbert_mask_and_sep
        st, H = self.st, self.H
        dev = input_ids.device
        B, L = input_ids.shape
        V, Fd = int(pixel_values.shape[1]), int(pixel_values.shape[2])
        S = L + V
        M = B * S
        pe = self.lin(pixel_values.contiguous().view(B * V, Fd), [VPROJ], [EMB + "visual_projection.bias"], H)
        x = _e((M, H), F32, dev)
        ops.vbert_embed_fwd(ids=input_ids, tt=token_type_ids, word=st.m(WORD), pos=st.m(EMB + "position_embeddings.weight"),
                            type_=st.m(EMB + "token_type_embeddings.weight"), vpos=st.m(EMB + "visual_position_embeddings.weight")[0],
                            vtype=st.m(EMB + "visual_token_type_embeddings.weight")[1], proj=pe, gamma=st.m(EMB + "LayerNorm.weight"),
                            beta=st.m(EMB + "LayerNorm.bias"), eps=self.eps, B=B, L=L, V=V, H=H, x=x, s=_e((M, H), F32, dev),
                            mean=_e((M,), F32, dev), rstd=_e((M,), F32, dev))
        mask, sep = vbert_mask_and_sep(attention_mask, visual_attention_mask, sep_idx, V)
        for l in range(self.nl):
            p = f"visual_bert.encoder.layer.{l}."
            x = self._block(p, x, B, S, attn_mask=mask, sep=sep, sep_stride=1, w0=st.m(p + "attention.self.adaptive_weight.0"),
                            w1=st.m(p + "attention.self.adaptive_weight.1"), rw_row_lo=V + 1)
        y = self.lin(x, [HEAD + "dense.weight"], [HEAD + "dense.bias"], H, act=ops.ACT_GELU)
        trans = self._ln(y, HEAD + "LayerNorm.weight", HEAD + "LayerNorm.bias", self.eps)
        return trans.view(B, S, H)
