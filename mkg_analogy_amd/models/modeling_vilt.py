"""ViLT backbone under the MarT framework (reference: MarT/models/modeling_vilt.py:896-968 ViltForMaskedLM, MarT/models/model.py ViltKGC)
on the gfx950 HIP kernels.

Only the path MarT runs is implemented: the joint text + two-image embedding (random patch order, drawn on the host exactly as the
reference draws it), 12 pre-LN layers with the ViLT variant of the adaptive analogy reweight, the final layernorm and the MLM head on the
text positions.  The pooler exists as parameters (checkpoint compatibility) but is never evaluated, as in the reference's MarT usage.
Sub-modules are parameter containers; compute is in ``mkg_analogy_amd.vilt_engine``.  All dropout probabilities must be 0 (ViltConfig
defaults), images are 384 x 384 with no pixel mask.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional

import torch
from torch import nn

from .. import functional as Fn
from ..engine_precise import PreciseViltForward
from ..params import FlatStore
from ..vilt_engine import VILT_DEAD, WORD as VILT_WORD, ViltEngine, vilt_f16_weight, vilt_gemm_groups, vilt_layout_order
from ._backbone import HipMaskedLM
from .modeling_flava import FlavaLayer
from .modeling_unimo import _Container


def draw_patch_order(B: int, n_patches: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """[2, B, n_patches] int64: the patch order of every image, drawn with the reference's calls (modeling_vilt.py:150-184 with
    max_image_length = -1 and every patch valid): image 0 for b = 0..B-1, then image 1, each ``torch.multinomial(ones(n).float(), n)`` on
    the default CPU generator (or ``generator``).  Token j + 1 of image i of example b is patch ``order[i, b, j]``."""
    out = torch.empty((2, B, n_patches), dtype=torch.int64)
    w = torch.ones(n_patches).float()
    for i in range(2):
        for b in range(B):
            out[i, b] = torch.multinomial(w, n_patches, generator=generator)
    return out


class TextEmbeddings(_Container):
    def __init__(self, c):
        super().__init__()
        self.word_embeddings = nn.Embedding(c.vocab_size, c.hidden_size)
        self.position_embeddings = nn.Embedding(c.max_position_embeddings, c.hidden_size)
        self.token_type_embeddings = nn.Embedding(c.type_vocab_size, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.register_buffer("position_ids", torch.arange(c.max_position_embeddings).expand((1, -1)))


class PatchEmbeddings(_Container):
    def __init__(self, c):
        super().__init__()
        self.projection = nn.Conv2d(c.num_channels, c.hidden_size, kernel_size=c.patch_size, stride=c.patch_size)


class ViltEmbeddings(_Container):
    def __init__(self, c):
        super().__init__()
        self.text_embeddings = TextEmbeddings(c)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, c.hidden_size))
        self.patch_embeddings = PatchEmbeddings(c)
        n = (c.image_size // c.patch_size) ** 2
        self.position_embeddings = nn.Parameter(torch.zeros(1, n + 1, c.hidden_size))
        self.token_type_embeddings = nn.Embedding(c.modality_type_vocab_size, c.hidden_size)


class ViltEncoder(_Container):
    def __init__(self, c):
        super().__init__()
        self.layer = nn.ModuleList([FlavaLayer(c.hidden_size, c.intermediate_size, c.layer_norm_eps) for _ in range(c.num_hidden_layers)])


class _Dense(_Container):
    def __init__(self, i, o):
        super().__init__()
        self.dense = nn.Linear(i, o)


class ViltModel(_Container):
    def __init__(self, c):
        super().__init__()
        self.embeddings = ViltEmbeddings(c)
        self.encoder = ViltEncoder(c)
        self.layernorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.pooler = _Dense(c.hidden_size, c.hidden_size)


class ViltPredictionHeadTransform(_Container):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)


class ViltMLMHead(_Container):
    def __init__(self, c):
        super().__init__()
        self.transform = ViltPredictionHeadTransform(c)
        self.decoder = nn.Linear(c.hidden_size, c.vocab_size, bias=False)
        self.bias = nn.Parameter(torch.zeros(c.vocab_size))
        self.decoder.bias = self.bias


def vilt_config(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                max_position_embeddings=40, image_size=384, patch_size=32, layer_norm_eps=1e-12):
    """Plain-object stand-in for transformers.ViltConfig (attribute access only; the real config object works too)."""
    return SimpleNamespace(vocab_size=vocab_size, hidden_size=hidden_size, num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                           intermediate_size=intermediate_size, hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                           initializer_range=0.02, layer_norm_eps=layer_norm_eps, max_position_embeddings=max_position_embeddings, type_vocab_size=2,
                           modality_type_vocab_size=2, image_size=image_size, patch_size=patch_size, num_channels=3, qkv_bias=True,
                           max_image_length=-1, pad_token_id=0)


class ViltForMaskedLM(HipMaskedLM):
    WORD, BIAS = VILT_WORD, "mlm_score.bias"
    ENGINE, PRECISE = ViltEngine, PreciseViltForward              # fp32 training (verification mode) is not built for ViLT

    def __init__(self, config):
        super().__init__(config)
        if getattr(config, "hidden_dropout_prob", 0.0) or getattr(config, "attention_probs_dropout_prob", 0.0):
            raise NotImplementedError("the HIP ViLT path implements the ViltConfig defaults (all dropouts 0)")
        if getattr(config, "max_image_length", -1) not in (-1, None):
            raise NotImplementedError("the HIP ViLT path keeps every patch (max_image_length = -1, the ViltConfig default)")
        if getattr(config, "hidden_act", "gelu") != "gelu" or not getattr(config, "qkv_bias", True):
            raise NotImplementedError("the HIP ViLT path implements erf GELU and biased q / k / v projections")
        self.vilt = ViltModel(config)
        self.mlm_score = ViltMLMHead(config)
        self._tie_and_hook()

    def _make_store(self, named, device):
        n = self.config.num_hidden_layers
        return FlatStore(named, 0, device, order=vilt_layout_order(n), gemm_groups=vilt_gemm_groups(n), dead=VILT_DEAD(), f16_weight=vilt_f16_weight)

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, pixel_values=None, pixel_mask=None, head_mask=None,
                inputs_embeds=None, image_embeds=None, labels=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                sep_idx=None, image_index=None):
        if pixel_mask is not None or image_embeds is not None or inputs_embeds is not None or head_mask is not None or output_attentions:
            raise NotImplementedError("MarT never passes pixel_mask / image_embeds / inputs_embeds / head_mask / output_attentions; "
                                      "unsupported on the HIP ViLT path")
        if sep_idx is None:
            # the reference shifts sep_idx in place (modeling_vilt.py:844): None fails there with this TypeError, so ViLT has no pre-train step
            raise TypeError("unsupported operand type(s) for +=: 'NoneType' and 'int' (ViLT needs sep_idx: no MarKG pre-train step)")
        fp32 = self.precision == "fp32"
        if fp32 and (torch.is_grad_enabled() or self.training):
            raise NotImplementedError("precision='fp32' is the ViLT evaluation path (model.eval() under torch.no_grad()); "
                                      "fp32 training (verification mode) is not built for ViLT")
        if fp32 and labels is not None:
            raise NotImplementedError("precision='fp32': no full-vocabulary labels path; score slices of .logits instead")
        st = self.finalize()
        self._check_trainable()
        dev = st.device
        input_ids, attention_mask, token_type_ids, sep_idx = self._text_inputs(dev, input_ids, attention_mask, token_type_ids, sep_idx)
        pixel_values, image_table, image_index = self._image_inputs(dev, pixel_values, image_index)
        P = (self.config.image_size // self.config.patch_size) ** 2
        order = draw_patch_order(input_ids.shape[0], P)         # the reference's draws, on the default CPU generator (always a permutation)
        if fp32:
            st.join_pending()
            pr = self._fp32_engine()
            trans = pr.forward(input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, order, image_table=image_table, image_index=image_index)
            return self._pack(trans, self._logits(trans, None, precise=pr), return_dict)
        self._engine.patch_order = order
        holder: Dict[str, torch.Tensor] = {}
        self._engine.save_for_backward = torch.is_grad_enabled()
        trans = Fn._MKGformerFn.apply(self._anchor, self._engine, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx,
                                      bool(self.training), self._next_seed(), holder, image_table, image_index)
        st.join_pending()
        logits = self._logits(trans, holder["trans_bf16"], head_split=self._engine.head_split)
        loss = None
        if labels is not None:
            full = logits.materialize()
            loss = torch.nn.functional.cross_entropy(full.view(-1, full.shape[-1]), labels.to(dev).view(-1))
        return self._pack(trans, logits, return_dict, loss=loss)
