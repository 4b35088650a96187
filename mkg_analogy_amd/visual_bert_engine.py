"""Manual forward/backward schedule of the VisualBERT path MarT runs (reference: MarT/models/modeling_visual_bert.py:854-911
VisualBertModel.forward, :1664-1723 VisualBertForMaskedLM.forward) on the HIP kernels.

One stack of 12 post-LN BERT blocks over the joint sequence [text (L) | regions (V = 72: two entities x 36 Faster R-CNN regions)], S = L + V:
  embeddings  region features [B, V, 2048] -> visual_projection (GEMM, K = 2048, f32 result) -> csrc/visual_bert.hip: text rows word + type +
              position, region rows projection + visual position row 0 + visual type row 1, ONE LayerNorm and ONE dropout over the concatenation,
  attention   scores / 8, additive mask over [attention_mask | visual_attention_mask] (NOT a prefix: text padding sits in the middle of the key
              range and whole 36-key region blocks can be masked), the adaptive-analogy reweight shifted into region territory:
              s' = sep_idx[:, 2] + V, rows [V + 1, s') x keys [s', S) scaled by clamp(w0, 0, .5), rows [s', S) x keys [s', S) by clamp(w1, .5, 1)
              (:255-260; the attention kernels' rw_row_lo), attention-probability dropout,
  block       attention.output.dense + dropout + residual + LayerNorm, intermediate.dense + erf GELU, output.dense + dropout + residual + LayerNorm,
  head        transform (dense, erf GELU, LayerNorm) on all S rows -- trans_hidden_states is [B, S, H] and the lit model reads rows in region
              territory (lit_models/transformer.py:98-102) --, decoder tied to the word embedding.  No pooler (add_pooling_layer=False).
The post-LN block is written here on purpose (engine.py's text layer carries the MKGformer fusion, the row-subset pass and a two-stream schedule).
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional

import torch

from . import ops
from .params import FlatStore

BF, F32, HF = torch.bfloat16, torch.float32, torch.float16
WORD, BIAS = "visual_bert.embeddings.word_embeddings.weight", "cls.predictions.bias"
HEAD = "cls.predictions.transform."
EMB = "visual_bert.embeddings."
VPROJ = EMB + "visual_projection.weight"


def _e(shape, dtype, dev):
    return torch.empty(shape, device=dev, dtype=dtype)


def _qkv(p: str, kind: str) -> List[str]:
    return [p + f"attention.self.{n}.{kind}" for n in ("query", "key", "value")]


def _layer_names(p: str) -> List[str]:
    return _qkv(p, "weight") + _qkv(p, "bias") + [
        p + "attention.self.adaptive_weight.0", p + "attention.self.adaptive_weight.1",
        p + "attention.output.dense.weight", p + "attention.output.dense.bias", p + "attention.output.LayerNorm.weight", p + "attention.output.LayerNorm.bias",
        p + "intermediate.dense.weight", p + "intermediate.dense.bias",
        p + "output.dense.weight", p + "output.dense.bias", p + "output.LayerNorm.weight", p + "output.LayerNorm.bias"]


def vbert_layout_order(n: int) -> List[str]:
    """Backward-completion order: head, encoder (top down), embeddings, decoder bias, tied word embedding last."""
    o = [HEAD + "dense.weight", HEAD + "dense.bias", HEAD + "LayerNorm.weight", HEAD + "LayerNorm.bias"]
    for l in reversed(range(n)):
        o += _layer_names(f"visual_bert.encoder.layer.{l}.")
    o += [EMB + "LayerNorm.weight", EMB + "LayerNorm.bias", EMB + "position_embeddings.weight", EMB + "token_type_embeddings.weight",
          EMB + "visual_token_type_embeddings.weight", EMB + "visual_position_embeddings.weight", VPROJ, EMB + "visual_projection.bias", BIAS, WORD]
    return o


def vbert_f16_weight(name: str) -> bool:
    """GEMM weights that get an fp16 forward shadow: the visual projection and the encoder's four products per layer (as vilt_f16_weight)."""
    if name == VPROJ:
        return True
    return name.startswith("visual_bert.encoder.layer.") and name.endswith(".weight") and "LayerNorm" not in name and "adaptive_weight" not in name


def vbert_gemm_groups(n: int):
    g = [("head", (HEAD + "dense.weight",))]
    for l in range(n):
        p = f"visual_bert.encoder.layer.{l}."
        g += [(f"l{l}.qkv", tuple(_qkv(p, "weight"))), (f"l{l}.ao", (p + "attention.output.dense.weight",)),
              (f"l{l}.int", (p + "intermediate.dense.weight",)), (f"l{l}.out", (p + "output.dense.weight",))]
    return g


def vbert_mask_and_sep(attention_mask: torch.Tensor, visual_attention_mask: Optional[torch.Tensor], sep_idx: torch.Tensor, V: int):
    """The joint key mask [attention_mask | visual_attention_mask] (int64, 1 = attended; a missing visual mask is all ones, :831-832) and the
    reweight split s' = sep_idx[:, 2] + V (:864-866), both NEW tensors: the reference shifts the caller's sep_idx in place, this path leaves it
    as it was."""
    B = attention_mask.shape[0]
    dev = attention_mask.device
    if visual_attention_mask is None:
        vm = torch.ones((B, V), device=dev, dtype=torch.int64)
    else:
        assert tuple(visual_attention_mask.shape) == (B, V), "visual_attention_mask must be [B, V]"
        vm = (visual_attention_mask.to(dev) != 0).to(torch.int64)
    mask = torch.cat([(attention_mask != 0).to(torch.int64), vm], 1).contiguous()
    return mask, (sep_idx[:, 2] + V).contiguous()


class VisualBertEngine:
    def __init__(self, store: FlatStore, config):
        self.st, self.cfg = store, config
        self.H, self.nh, self.I = config.hidden_size, config.num_attention_heads, config.intermediate_size
        assert self.H // self.nh == 64, "HIP path: head_dim 64"
        self.nl = config.num_hidden_layers
        self.F = int(config.visual_embedding_dim)
        self.eps = float(config.layer_norm_eps)
        self.p_hidden = float(config.hidden_dropout_prob)
        self.p_attn = float(config.attention_probs_dropout_prob)
        self.grad_ready: Optional[Callable[[int], None]] = None
        self.grad_ready_async: Optional[Callable] = None
        self.taps: Optional[dict] = None
        # forward products on fp16 operands (engine.UnimoEngine.text_f16: LayerNorm outputs, contexts, GELU outputs and N(0, 0.02)-scale weights
        # rounded 8x finer than bf16 at the same MFMA rate; the backward pass multiplies bf16) and the head transform / scoring GEMM on two-term
        # operand splits (engine.UnimoEngine.head_split).  The region features join the fp16 side: pooled post-ReLU detector features are
        # O(1..100), far inside fp16's range
        self.f16 = os.environ.get("MART_TEXT_F16", "1") == "1" and getattr(store, "f16_weight", None) is vbert_f16_weight
        self.head_split = os.environ.get("MART_HEAD_SPLIT", "1") == "1"
        self.visual_mask: Optional[torch.Tensor] = None    # [B, V] (1 = attended) or None = all regions: set by the model before each forward

    # ------------------------------------------------------------------ forward
    def forward(self, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, train: bool, seed: int,
                image_table=None, image_index=None):
        st, H, I, nh, dev = self.st, self.H, self.I, self.nh, input_ids.device
        if image_index is not None or image_table is not None:
            raise NotImplementedError("VisualBERT: region features travel in pixel_values; the device image table holds pixels only")
        if sep_idx is None:
            raise TypeError("VisualBERT needs sep_idx (modeling_visual_bert.py:866 shifts it in place; the reference cannot run without it)")
        B, L = input_ids.shape
        assert pixel_values.dim() == 3 and pixel_values.shape[0] == B and pixel_values.shape[2] == self.F and pixel_values.dtype == F32, \
            f"pixel_values must be f32 [B, V, {self.F}] region features"
        V = int(pixel_values.shape[1])
        assert L <= st.slots[EMB + "position_embeddings.weight"].shape[0], "text longer than max_position_embeddings"
        S = L + V
        M = B * S
        keep = bool(getattr(self, "save_for_backward", True))      # False under torch.no_grad(): backward-only outputs are skipped
        f16 = self.f16
        kb = keep or not f16                                        # bf16 twins needed
        p_h = self.p_hidden if train else 0.0
        p_a = self.p_attn if train else 0.0
        sv: Dict[str, object] = dict(B=B, L=L, V=V, S=S, ids=input_ids, tt=token_type_ids, train=train, seed=seed)
        W = (lambda *n: st.h(*n)) if f16 else (lambda *n: st.fused(list(n)))
        # ---- visual projection: features cast once to the GEMM operand type, K = 2048, bias, f32 result
        feat = pixel_values.contiguous().view(B * V, self.F)
        fb = None
        if kb:
            fb = _e((B * V, self.F), BF, dev)                      # the weight gradient's operand
            ops.cast_f32_bf16(feat, fb)
        fa = fb
        if f16:
            fa = _e((B * V, self.F), HF, dev)
            ops.cast_f32_f16(feat, fa)
        pe = _e((B * V, H), F32, dev)
        ops.gemm_nt(fa, W(VPROJ), pe, bias=st.m(EMB + "visual_projection.bias"))
        sv["feat"] = fb
        # ---- joint embedding: LayerNorm + dropout over [text | regions], with the 16-bit copy layer 0's Q/K/V product reads
        x = _e((M, H), F32, dev)
        xb = _e((M, H), BF, dev) if kb else None
        xh = _e((M, H), HF, dev) if f16 else None
        s_e, emean, erstd = _e((M, H), F32, dev), _e((M,), F32, dev), _e((M,), F32, dev)
        ops.vbert_embed_fwd(ids=input_ids, tt=token_type_ids, word=st.m(WORD), pos=st.m(EMB + "position_embeddings.weight"),
                            type_=st.m(EMB + "token_type_embeddings.weight"), vpos=st.m(EMB + "visual_position_embeddings.weight")[0],
                            vtype=st.m(EMB + "visual_token_type_embeddings.weight")[1], proj=pe, gamma=st.m(EMB + "LayerNorm.weight"),
                            beta=st.m(EMB + "LayerNorm.bias"), eps=self.eps, p_drop=p_h, seed=seed + 1, B=B, L=L, V=V, H=H,
                            x=x, x_bf16=xb, x_f16=xh, s=s_e, mean=emean, rstd=erstd)
        sv["emb"] = (s_e, emean, erstd)
        if self.taps is not None:
            self.taps["emb"] = x.view(B, S, H).clone()
        mask, sep = vbert_mask_and_sep(attention_mask, self.visual_mask, sep_idx, V)
        for l in range(self.nl):
            p = f"visual_bert.encoder.layer.{l}."
            qkv = _e((M, 3 * H), BF, dev)
            ops.gemm_nt(xh if f16 else xb, W(*_qkv(p, "weight")), qkv, bias=st.fused(_qkv(p, "bias"), st.master))
            ctx, lse = _e((M, H), BF, dev), _e((B, nh, S), F32, dev)
            ctxh = _e((M, H), HF, dev) if f16 else None
            akw = dict(q=qkv[:, :H], k=qkv[:, H:2 * H], v=qkv[:, 2 * H:], ctx=ctx, lse=lse, B=B, nh=nh, Sq=S, Sk=S, scale=0.125, attn_mask=mask,
                       sep=sep, sep_stride=1, w0=st.m(p + "attention.self.adaptive_weight.0"), w1=st.m(p + "attention.self.adaptive_weight.1"),
                       rw_row_lo=V + 1, p_drop=p_a, seed=seed + 10 + 4 * l)
            ops.attn_fwd(ctx_f16=ctxh, **akw)
            # attention.output: dense + dropout + residual + LayerNorm (the dense output reaches the LayerNorm in f32)
            so = _e((M, H), F32, dev)
            ops.gemm_nt(ctxh if f16 else ctx, W(p + "attention.output.dense.weight"), so, bias=st.m(p + "attention.output.dense.bias"))
            s1, m1, r1 = _e((M, H), F32, dev), _e((M,), F32, dev), _e((M,), F32, dev)
            a, ab, ah = _e((M, H), F32, dev), (_e((M, H), BF, dev) if kb else None), (_e((M, H), HF, dev) if f16 else None)
            ops.ln_fwd(x_f32=x, y_f32=so, gamma=st.m(p + "attention.output.LayerNorm.weight"), beta=st.m(p + "attention.output.LayerNorm.bias"), eps=self.eps,
                       M=M, H=H, mean=m1, rstd=r1, s_out=s1, out_f32=a, out_bf16=ab, out_f16=ah, p_drop=p_h, seed=seed + 11 + 4 * l)
            del so
            # feed-forward: intermediate.dense + GELU, output.dense + dropout + residual + LayerNorm
            zt = _e((M, I), BF, dev) if keep else None               # gelu'(intermediate.dense output): all the backward pass needs of it
            ht = _e((M, I), BF, dev) if kb else None
            hth = _e((M, I), HF, dev) if f16 else None
            ops.gemm_nt(ah if f16 else ab, W(p + "intermediate.dense.weight"), hth if f16 else ht, bias=st.m(p + "intermediate.dense.bias"),
                        act=ops.ACT_GELU, preact=zt, preact_grad=keep, C2=ht if f16 else None)
            oo = _e((M, H), F32, dev)
            ops.gemm_nt(hth if f16 else ht, W(p + "output.dense.weight"), oo, bias=st.m(p + "output.dense.bias"))
            del hth
            s2, m2, r2 = _e((M, H), F32, dev), _e((M,), F32, dev), _e((M,), F32, dev)
            last = l == self.nl - 1
            xo = _e((M, H), F32, dev)
            xob = _e((M, H), BF, dev) if (kb or (last and not self.head_split)) else None
            xoh = _e((M, H), HF, dev) if f16 and not last else None   # (the head transform reads the f32 stream)
            ops.ln_fwd(x_f32=a, y_f32=oo, gamma=st.m(p + "output.LayerNorm.weight"), beta=st.m(p + "output.LayerNorm.bias"), eps=self.eps,
                       M=M, H=H, mean=m2, rstd=r2, s_out=s2, out_f32=xo, out_bf16=xob, out_f16=xoh, p_drop=p_h, seed=seed + 12 + 4 * l)
            del oo
            sv[f"l{l}"] = dict(xb=xb, qkv=qkv, akw=akw, s1=s1, m1=m1, r1=r1, ab=ab, zt=zt, ht=ht, s2=s2, m2=m2, r2=r2) if keep else None
            x, xb, xh = xo, xob, xoh
            if self.taps is not None:
                self.taps[f"l{l}"] = x.view(B, S, H).clone()
        # ---- MLM head transform on all S rows (:517-521)
        y, zh = _e((M, H), F32, dev), _e((M, H), BF, dev)
        if self.head_split:
            ver, w3 = getattr(self, "_head_w3", (-1, None))
            if ver != st.version:
                w3 = ops.split_bf16x3(st.m(HEAD + "dense.weight"), 1)
                self._head_w3 = (st.version, w3)
            ops.gemm_nt(ops.split_bf16x3(x, 0), w3, y, bias=st.m(HEAD + "dense.bias"), act=ops.ACT_GELU, preact=zh)
        else:
            ops.gemm_nt(xb, st.w(HEAD + "dense.weight"), y, bias=st.m(HEAD + "dense.bias"), act=ops.ACT_GELU, preact=zh)
        trans, transb = _e((M, H), F32, dev), _e((M, H), BF, dev)
        hm, hr = _e((M,), F32, dev), _e((M,), F32, dev)
        ops.ln_fwd(x_f32=y, gamma=st.m(HEAD + "LayerNorm.weight"), beta=st.m(HEAD + "LayerNorm.bias"), eps=self.eps, M=M, H=H, mean=hm, rstd=hr,
                   out_f32=trans, out_bf16=transb)
        sv["head"] = (xb, y, zh, hm, hr)
        return trans.view(B, S, H), transb, sv

    # ------------------------------------------------------------------ backward
    def backward(self, sv, dtrans: torch.Tensor) -> None:
        """Accumulates d(loss)/d(param) into FlatStore.grad given d(loss)/d(trans_hidden_states) (f32 [B, S, H])."""
        st, H, I, nh, dev = self.st, self.H, self.I, self.nh, dtrans.device
        B, L, V, S = sv["B"], sv["L"], sv["V"], sv["S"]
        M = B * S
        seed = sv["seed"]
        p_h = self.p_hidden if sv["train"] else 0.0
        st.join_pending()

        def notify(off):
            if self.grad_ready is not None:
                self.grad_ready(off)
            if self.grad_ready_async is not None:
                self.grad_ready_async(off, [])

        def wgrad(X, Y, wn, bn):
            g = st.g(wn)
            ops.gemm_tn(X, Y, g.view(g.shape[0], -1), colsum=st.g(bn))
        # ---- head transform
        xb, y, zh, hm, hr = sv["head"]
        dyb = _e((M, H), BF, dev)
        ops.ln_bwd(dy_f32=dtrans.contiguous().view(M, H), s=y, mean=hm, rstd=hr, gamma=st.m(HEAD + "LayerNorm.weight"), M=M, H=H, ds_bf16=dyb,
                   dgamma=st.g(HEAD + "LayerNorm.weight"), dbeta=st.g(HEAD + "LayerNorm.bias"))
        dzh = _e((M, H), BF, dev)
        ops.act_bwd(dyb, zh, ops.ACT_GELU, dzh)
        wgrad(dzh, xb, HEAD + "dense.weight", HEAD + "dense.bias")
        d_f32, d_b16 = _e((M, H), F32, dev), None                 # gradient w.r.t. the residual stream: an f32 part plus an optional bf16 part
        ops.gemm_nt(dzh, st.wt("head"), d_f32)
        del dyb, dzh
        notify(st.slots[_qkv(f"visual_bert.encoder.layer.{self.nl - 1}.", "weight")[0]].offset)
        for l in reversed(range(self.nl)):
            p = f"visual_bert.encoder.layer.{l}."
            s = sv[f"l{l}"]
            # output LayerNorm: ds2 = the residual path (f32), doo = the dropped-out dense branch (bf16)
            ds2, doo = _e((M, H), F32, dev), _e((M, H), BF, dev)
            ops.ln_bwd(dy_f32=d_f32, dy_bf16=d_b16, s=s["s2"], mean=s["m2"], rstd=s["r2"], gamma=st.m(p + "output.LayerNorm.weight"), M=M, H=H,
                       ds_f32=ds2, ds_bf16=doo, p_drop=p_h, seed=seed + 12 + 4 * l,
                       dgamma=st.g(p + "output.LayerNorm.weight"), dbeta=st.g(p + "output.LayerNorm.bias"))
            wgrad(doo, s["ht"], p + "output.dense.weight", p + "output.dense.bias")
            dzt = _e((M, I), BF, dev)
            ops.gemm_nt(doo, st.wt(f"l{l}.out"), dzt, mulz=s["zt"], mul_act=ops.ACT_STORED)
            wgrad(dzt, s["ab"], p + "intermediate.dense.weight", p + "intermediate.dense.bias")
            da2 = doo                                              # reuse
            ops.gemm_nt(dzt, st.wt(f"l{l}.int"), da2)
            del dzt
            # attention-output LayerNorm
            ds1, dso = d_f32, _e((M, H), BF, dev)                   # (d_f32 has been consumed: its buffer takes the new residual-path gradient)
            ops.ln_bwd(dy_f32=ds2, dy_bf16=da2, s=s["s1"], mean=s["m1"], rstd=s["r1"], gamma=st.m(p + "attention.output.LayerNorm.weight"), M=M, H=H,
                       ds_f32=ds1, ds_bf16=dso, p_drop=p_h, seed=seed + 11 + 4 * l,
                       dgamma=st.g(p + "attention.output.LayerNorm.weight"), dbeta=st.g(p + "attention.output.LayerNorm.bias"))
            akw = s["akw"]
            wgrad(dso, akw["ctx"], p + "attention.output.dense.weight", p + "attention.output.dense.bias")
            dctx = da2                                             # reuse
            ops.gemm_nt(dso, st.wt(f"l{l}.ao"), dctx)
            dqkv, delta = _e((M, 3 * H), BF, dev), _e((B, nh, S), F32, dev)
            ops.attn_bwd(dctx=dctx, delta=delta, dq=dqkv[:, :H], dk=dqkv[:, H:2 * H], dv=dqkv[:, 2 * H:],
                         dw=st.g(p + "attention.self.adaptive_weight.0"), **akw)
            ops.gemm_tn(dqkv, s["xb"], st.fused(_qkv(p, "weight"), st.grad), colsum=st.fused(_qkv(p, "bias"), st.grad))
            dtb = dso                                              # reuse
            ops.gemm_nt(dqkv, st.wt(f"l{l}.qkv"), dtb)
            d_f32, d_b16 = ds1, dtb
            sv[f"l{l}"] = None
            nxt = _qkv(f"visual_bert.encoder.layer.{l - 1}.", "weight")[0] if l > 0 else EMB + "LayerNorm.weight"
            notify(st.slots[nxt].offset)
        # ---- embeddings: dropout + LayerNorm backward, small tables, then the word scatter and the projection's weight gradient
        s_e, emean, erstd = sv["emb"]
        dx = d_f32
        ops.add_f32_bf16(d_f32, d_b16, dx, None)                   # f32 + bf16 parts of the stream gradient, in place (elementwise)
        ds_t, dproj = _e((B * L, H), F32, dev), _e((B * V, H), BF, dev)
        ws = _e(((B * V + 4 * S) * H,), F32, dev)
        ops.vbert_embed_bwd(ids=sv["ids"], tt=sv["tt"], gamma=st.m(EMB + "LayerNorm.weight"), p_drop=p_h, seed=seed + 1, B=B, L=L, V=V, H=H,
                            s=s_e, mean=emean, rstd=erstd, dx=dx, ds_text=ds_t, dproj=dproj,
                            dgamma=st.g(EMB + "LayerNorm.weight"), dbeta=st.g(EMB + "LayerNorm.bias"), dpos=st.g(EMB + "position_embeddings.weight"),
                            dtype=st.g(EMB + "token_type_embeddings.weight"), dvpos=st.g(EMB + "visual_position_embeddings.weight")[0],
                            dvtype=st.g(EMB + "visual_token_type_embeddings.weight")[1], ws=ws)
        # word rows: the text-embedding scatter (its position / type sums go to a scratch buffer; vbert_embed_bwd owns those tables)
        scratch_pos, scratch_type = torch.zeros((L, H), device=dev, dtype=F32), torch.zeros((2, H), device=dev, dtype=F32)
        ops.text_embed_scatter(ds_t, sv["ids"], sv["tt"], st.g(WORD), scratch_pos, scratch_type, B, L, H)
        ops.gemm_tn(dproj, sv["feat"], st.g(VPROJ), colsum=st.g(EMB + "visual_projection.bias"))
        notify(st.total)
