"""Manual forward/backward schedule of the ViLT path MarT runs (reference: MarT/models/modeling_vilt.py:760-869 ViltModel.forward,
:914-968 ViltForMaskedLM.forward) on the HIP kernels.

One stack of 12 pre-LN blocks (the ViT block of FlavaEngine._layer_fwd / _layer_bwd, reused as is) over the joint sequence
[text (L) | image 0 (1 + P) | image 1 (1 + P)], S = L + 290 at 384 px / patch 32:
  embeddings  csrc/vilt.hip (text: BERT embeddings with positions only below max_position_embeddings, LN, modality row 0;
              image: cls / patch projection in a per-example random patch order, positions, modality row 1),
  attention   additive padding mask over [attention_mask | ones(290)], ViLT's adaptive-analogy reweight shifted into image territory:
              s' = sep_idx[:, 2] + 290, rows [291, s') x keys [s', S) scaled by clamp(w0, 0, .5), rows [s', S) x keys [s', S) by
              clamp(w1, .5, 1) (:370-375; the attention kernels' rw_row_lo),
  final LayerNorm (vilt.layernorm), MLM head transform (dense, erf GELU, LN) on the text rows, decoder tied to the word embedding.
Dropouts are 0 (ViltConfig defaults).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import os

import torch

from . import ops
from .flava_engine import FlavaEngine, _layer_names
from .params import FlatStore

BF, F32, HF = torch.bfloat16, torch.float32, torch.float16
WORD = "vilt.embeddings.text_embeddings.word_embeddings.weight"


def _e(shape, dtype, dev):
    return torch.empty(shape, device=dev, dtype=dtype)


def vilt_layout_order(n: int) -> List[str]:
    """Backward-completion order: head, encoder (top down), embeddings, never-used tensors, tied word embedding last."""
    o = ["mlm_score.transform.dense.weight", "mlm_score.transform.dense.bias", "mlm_score.transform.LayerNorm.weight",
         "mlm_score.transform.LayerNorm.bias", "vilt.layernorm.weight", "vilt.layernorm.bias"]
    for l in reversed(range(n)):
        o += _layer_names(f"vilt.encoder.layer.{l}.")
    e, t = "vilt.embeddings.", "vilt.embeddings.text_embeddings."
    o += [t + "LayerNorm.weight", t + "LayerNorm.bias", t + "position_embeddings.weight", t + "token_type_embeddings.weight",
          e + "cls_token", e + "position_embeddings", e + "patch_embeddings.projection.weight", e + "patch_embeddings.projection.bias",
          e + "token_type_embeddings.weight", "vilt.pooler.dense.weight", "vilt.pooler.dense.bias", "mlm_score.bias", WORD]
    return o


def VILT_DEAD() -> tuple:
    """Tensors whose gradient is None in the reference's MarT usage: the pooler is computed but never reaches the loss."""
    return ("vilt.pooler.",)


def vilt_f16_weight(name: str) -> bool:
    """GEMM weights that get an fp16 forward shadow: the patch projection and the encoder's four products per layer (as flava_f16_weight)."""
    if name == "vilt.embeddings.patch_embeddings.projection.weight":
        return True
    return name.startswith("vilt.encoder.layer.") and name.endswith(".weight") and "layernorm" not in name


def vilt_gemm_groups(n: int):
    g = [("head", ("mlm_score.transform.dense.weight",))]
    for l in range(n):
        p = f"vilt.encoder.layer.{l}."
        g += [(f"l{l}.qkv", tuple(p + f"attention.attention.{x}.weight" for x in ("query", "key", "value"))),
              (f"l{l}.o", (p + "attention.output.dense.weight",)), (f"l{l}.fc1", (p + "intermediate.dense.weight",)),
              (f"l{l}.fc2", (p + "output.dense.weight",))]
    return g


def vilt_mask_and_sep(attention_mask: torch.Tensor, sep_idx: torch.Tensor, n_image: int):
    """The joint key mask [attention_mask | ones(n_image)] and the reweight split s' = sep_idx[:, 2] + n_image (modeling_vilt.py:241, :843-844),
    both NEW tensors: the reference shifts the caller's sep_idx in place, this path leaves it as it was."""
    B = attention_mask.shape[0]
    mask = torch.cat([attention_mask, torch.ones((B, n_image), device=attention_mask.device, dtype=attention_mask.dtype)], 1).contiguous()
    return mask, (sep_idx[:, 2] + n_image).contiguous()


class ViltEngine:
    # the pre-LN block of the FLAVA engine, shared (same parameter names under a layer prefix, same arithmetic)
    _layer_fwd = FlavaEngine._layer_fwd
    _layer_bwd = FlavaEngine._layer_bwd

    def __init__(self, store: FlatStore, config):
        self.st, self.cfg = store, config
        self.H, self.nh, self.I = config.hidden_size, config.num_attention_heads, config.intermediate_size
        assert self.H // self.nh == 64, "HIP path: head_dim 64"
        self.nl = config.num_hidden_layers
        self.eps = float(config.layer_norm_eps)
        self.n_tpos = int(config.max_position_embeddings)
        self.grad_ready: Optional[Callable[[int], None]] = None
        self.grad_ready_async: Optional[Callable] = None
        self.taps: Optional[dict] = None
        self.grad_stream_bf16 = True
        # forward products on fp16 operands (FlavaEngine.f16: LayerNorm outputs, contexts and GELU outputs rounded 8x finer than bf16 at the
        # same MFMA rate) and the head transform on two-term operand splits (FlavaEngine.head_split): with bf16 operands the trans_hidden
        # rows sat at 4.7e-3 rel-L2 from the reference (G10), above the FLAVA gate of 4e-3
        self.f16 = os.environ.get("MART_TEXT_F16", "1") == "1" and getattr(store, "f16_weight", None) is vilt_f16_weight
        self.head_split = os.environ.get("MART_HEAD_SPLIT", "1") == "1"
        self.patch_order: Optional[torch.Tensor] = None    # [2, B, P] int64 (host): set by the model before each forward

    def forward(self, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, train: bool, seed: int,
                image_table=None, image_index=None):
        st, H, dev = self.st, self.H, input_ids.device
        B, L = input_ids.shape
        S_img, p = self.cfg.image_size, self.cfg.patch_size
        P = (S_img // p) ** 2
        ni = 2 * (1 + P)
        S = L + ni
        M = B * S
        if sep_idx is None:
            raise TypeError("ViLT needs sep_idx (modeling_vilt.py:844 shifts it in place; the reference cannot run without it)")
        perm = self.patch_order
        assert perm is not None and tuple(perm.shape) == (2, B, P), "patch order [2, B, P] must be drawn first (ViltForMaskedLM.draw_patch_order)"
        sv: Dict[str, object] = dict(B=B, L=L, P=P, S=S, ids=input_ids, tt=token_type_ids)
        # ---- patch projection (conv 32x32 stride 32 + bias as a GEMM), f32 result
        e = "vilt.embeddings."
        Kp = 3 * p * p
        pe = _e((B * 2 * P, H), F32, dev)
        if self.f16:
            pf = _e((B * 2 * P, Kp), F32, dev)
            if image_index is not None:
                ops.patchify_f32(image_table, image_index.contiguous(), pf, B, S_img, p)
            else:
                pix = pixel_values.contiguous()
                assert pix.dtype == F32 and tuple(pix.shape) == (B, 2, 3, S_img, S_img)
                ops.patchify_f32(pix, None, pf, B, S_img, p)
            ph = _e((B * 2 * P, Kp), HF, dev)
            ops.cast_f32_f16(pf, ph)
            patches = None
            if bool(getattr(self, "save_for_backward", True)):
                patches = _e((B * 2 * P, Kp), BF, dev)                 # the weight gradient's operand
                ops.cast_f32_bf16(pf, patches)
            del pf
            ops.gemm_nt(ph, st.h(e + "patch_embeddings.projection.weight").view(H, Kp), pe, bias=st.m(e + "patch_embeddings.projection.bias"))
        else:
            patches = _e((B * 2 * P, Kp), BF, dev)
            if image_index is not None:
                ops.patchify_gather(image_table, image_index.contiguous(), patches, B, S_img, p)
            else:
                pix = pixel_values.contiguous()
                assert pix.dtype == F32 and tuple(pix.shape) == (B, 2, 3, S_img, S_img)
                ops.patchify(pix, patches, B, S_img, p)
            ops.gemm_nt(patches, st.w(e + "patch_embeddings.projection.weight").view(H, Kp), pe, bias=st.m(e + "patch_embeddings.projection.bias"))
        sv["patches"] = patches
        perm_d = perm.to(device=dev, dtype=torch.int32).contiguous()
        inv_d = torch.argsort(perm_d.long(), dim=-1).to(torch.int32).contiguous()
        sv["perm"], sv["inv"] = perm_d, inv_d
        # ---- joint embedding
        t = e + "text_embeddings."
        x = _e((M, H), F32, dev)
        s_t, tmean, trstd = _e((B * L, H), F32, dev), _e((B * L,), F32, dev), _e((B * L,), F32, dev)
        ops.vilt_embed_fwd(ids=input_ids, tt=token_type_ids, word=st.m(t + "word_embeddings.weight"), tpos=st.m(t + "position_embeddings.weight"),
                           ttype=st.m(t + "token_type_embeddings.weight"), gamma=st.m(t + "LayerNorm.weight"), beta=st.m(t + "LayerNorm.bias"),
                           eps=self.eps, n_tpos=self.n_tpos, patch_f32=pe, cls=st.m(e + "cls_token"), ipos=st.m(e + "position_embeddings"),
                           modality=st.m(e + "token_type_embeddings.weight"), perm=perm_d, B=B, L=L, P=P, H=H, x=x, s_text=s_t, mean=tmean, rstd=trstd)
        sv["temb"] = (s_t, tmean, trstd)
        if self.taps is not None:
            self.taps["emb"] = x.view(B, S, H).clone()
        # ---- encoder: mask [attention_mask | ones(2 (1 + P))], reweight rows from ni + 1 on (modeling_vilt.py:370-375, :843-844)
        mask, sep = vilt_mask_and_sep(attention_mask, sep_idx, ni)
        sv["mask"], sv["sep"] = mask, sep
        for l in range(self.nl):
            a = f"vilt.encoder.layer.{l}.attention.attention."
            kw = dict(B=B, Sq=S, Sk=S, attn_mask=mask, sep=sep, sep_stride=1, w0=st.m(a + "adaptive_weight.0"), w1=st.m(a + "adaptive_weight.1"),
                      rw_row_lo=ni + 1)
            x, _, sv[f"l{l}"] = self._layer_fwd(f"vilt.encoder.layer.{l}.", x, M, kw, False, self.f16)
            if self.taps is not None:
                self.taps[f"l{l}"] = x.view(B, S, H).clone()
        # ---- final layernorm, text rows, MLM head transform (:861, :961-962, :981-985)
        split = self.head_split
        xb, xmean, xrstd = _e((M, H), BF, dev), _e((M,), F32, dev), _e((M,), F32, dev)
        xf = _e((M, H), F32, dev) if split else None
        ops.ln_fwd(x_f32=x, gamma=st.m("vilt.layernorm.weight"), beta=st.m("vilt.layernorm.bias"), eps=self.eps, M=M, H=H,
                   mean=xmean, rstd=xrstd, out_bf16=xb, out_f32=xf)
        Mt = B * L
        rows = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] * S + torch.arange(L, device=dev, dtype=torch.int32)[None]).reshape(-1).contiguous()
        y, zh = _e((Mt, H), F32, dev), _e((Mt, H), BF, dev)
        if split:
            ver, w3 = getattr(self, "_head_w3", (-1, None))
            if ver != st.version:
                w3 = ops.split_bf16x3(st.m("mlm_score.transform.dense.weight"), 1)
                self._head_w3 = (st.version, w3)
            ops.gemm_nt(ops.split_bf16x3_rows(xf, rows, 0), w3, y, bias=st.m("mlm_score.transform.dense.bias"), act=ops.ACT_GELU, preact=zh)
            del xf
        else:
            ops.gemm_nt(xb, st.w("mlm_score.transform.dense.weight"), y, a_rows=rows, bias=st.m("mlm_score.transform.dense.bias"), act=ops.ACT_GELU, preact=zh)
        trans, transb = _e((Mt, H), F32, dev), _e((Mt, H), BF, dev)
        hm, hr = _e((Mt,), F32, dev), _e((Mt,), F32, dev)
        ops.ln_fwd(x_f32=y, gamma=st.m("mlm_score.transform.LayerNorm.weight"), beta=st.m("mlm_score.transform.LayerNorm.bias"), eps=self.eps, M=Mt, H=H,
                   mean=hm, rstd=hr, out_f32=trans, out_bf16=transb)
        sv["head"] = (x, xmean, xrstd, xb, rows, y, zh, hm, hr)
        return trans.view(B, L, H), transb, sv

    def backward(self, sv, dtrans: torch.Tensor) -> None:
        st, H, dev = self.st, self.H, dtrans.device
        B, L, P, S = sv["B"], sv["L"], sv["P"], sv["S"]
        M, Mt = B * S, B * L

        def notify(off):
            if self.grad_ready is not None:
                self.grad_ready(off)
            if self.grad_ready_async is not None:
                self.grad_ready_async(off, [])
        x, xmean, xrstd, xb, rows, y, zh, hm, hr = sv["head"]
        # head transform
        dyb = _e((Mt, H), BF, dev)
        ops.ln_bwd(dy_f32=dtrans.contiguous().view(Mt, H), s=y, mean=hm, rstd=hr, gamma=st.m("mlm_score.transform.LayerNorm.weight"), M=Mt, H=H, ds_bf16=dyb,
                   dgamma=st.g("mlm_score.transform.LayerNorm.weight"), dbeta=st.g("mlm_score.transform.LayerNorm.bias"))
        dzh = _e((Mt, H), BF, dev)
        ops.act_bwd(dyb, zh, ops.ACT_GELU, dzh)
        seq_b = _e((Mt, H), BF, dev)
        ops.gather_rows_bf16(xb, rows, seq_b)
        ops.gemm_tn(dzh, seq_b, st.g("mlm_score.transform.dense.weight"), colsum=st.g("mlm_score.transform.dense.bias"))
        dseq = _e((Mt, H), F32, dev)
        ops.gemm_nt(dzh, st.wt("head"), dseq)
        dln = torch.zeros((M, H), device=dev, dtype=F32)
        ops.scatter_add_rows_f32(dseq, rows, dln)
        # final layernorm (image rows get a zero gradient: only the text rows reach the loss)
        dx, dxb = _e((M, H), F32, dev), _e((M, H), BF, dev)
        ops.ln_bwd(dy_f32=dln, s=x, mean=xmean, rstd=xrstd, gamma=st.m("vilt.layernorm.weight"), M=M, H=H, ds_f32=dx, ds_bf16=dxb, bf16_total=True,
                   dgamma=st.g("vilt.layernorm.weight"), dbeta=st.g("vilt.layernorm.bias"))
        del dln
        for l in reversed(range(self.nl)):
            pfx = f"vilt.encoder.layer.{l}."
            dw = st.g(pfx + "attention.attention.adaptive_weight.0")
            self._layer_bwd(pfx, f"l{l}", sv[f"l{l}"], M, dx, dxb, dw=dw, want_f32=(l == 0))
            sv[f"l{l}"] = None
        notify(st.slots["vilt.embeddings.text_embeddings.LayerNorm.weight"].offset)
        # embeddings
        e, t = "vilt.embeddings.", "vilt.embeddings.text_embeddings."
        s_t, tmean, trstd = sv["temb"]
        ds_t = _e((Mt, H), F32, dev)
        dpatch = _e((B * 2 * P, H), BF, dev)
        ws = _e(((1 + P + 4 * L) * H,), F32, dev)
        ops.vilt_embed_bwd(ids=sv["ids"], tt=sv["tt"], gamma=st.m(t + "LayerNorm.weight"), n_tpos=self.n_tpos, modality=st.m(e + "token_type_embeddings.weight"),
                           perm=sv["perm"], inv=sv["inv"], B=B, L=L, P=P, H=H, s_text=s_t, mean=tmean, rstd=trstd, dx=dx, ds_text=ds_t, dpatch=dpatch,
                           dgamma=st.g(t + "LayerNorm.weight"), dbeta=st.g(t + "LayerNorm.bias"), dtpos=st.g(t + "position_embeddings.weight"),
                           dttype=st.g(t + "token_type_embeddings.weight"), dcls=st.g(e + "cls_token"), dipos=st.g(e + "position_embeddings"),
                           dmodality=st.g(e + "token_type_embeddings.weight"), ws=ws)
        # word rows: the text-embedding scatter (position / type rows of the full-length text table go to a scratch buffer; vilt_embed_bwd owns them)
        scratch_pos, scratch_type = torch.zeros((L, H), device=dev, dtype=F32), torch.zeros((2, H), device=dev, dtype=F32)
        ops.text_embed_scatter(ds_t, sv["ids"], sv["tt"], st.g(t + "word_embeddings.weight"), scratch_pos, scratch_type, B, L, H)
        gw = st.g(e + "patch_embeddings.projection.weight")
        ops.gemm_tn(dpatch, sv["patches"], gw.view(H, -1), colsum=st.g(e + "patch_embeddings.projection.bias"))
        notify(st.total)
