"""VisualBERT backbone under the MarT framework (reference: MarT/models/modeling_visual_bert.py:1632-1723 VisualBertForMaskedLM,
MarT/models/model.py VisualBertKGC) on the gfx950 HIP kernels.

Only the path MarT runs is implemented: the joint text + region embedding (no image_text_alignment, no visual_token_type_ids: visual position 0,
visual type 1), 12 post-LN layers with the VisualBERT variant of the adaptive analogy reweight, and the MLM head on all S = L + V rows
(``trans_hidden_states`` is [B, S, H]; the lit model reads rows shifted by V).  No pooler (add_pooling_layer=False).  Sub-modules are parameter
containers; compute is in ``mkg_analogy_amd.visual_bert_engine``.  ``pixel_values`` are Faster R-CNN region features [B, V, visual_embedding_dim]
(MarT: V = 72, two entities x 36 regions); running the detector is outside this package.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict

import torch
from torch import nn

from .. import functional as Fn
from ..engine_precise import PreciseVisualBertForward
from ..params import FlatStore
from ..visual_bert_engine import BIAS as VBERT_BIAS, WORD as VBERT_WORD, VisualBertEngine, vbert_f16_weight, vbert_gemm_groups, vbert_layout_order
from ._backbone import HipMaskedLM
from .modeling_unimo import BertOutput, BertSelfOutput, UnimoOnlyMLMHead, _Container


class VisualBertEmbeddings(_Container):
    def __init__(self, c):
        super().__init__()
        self.word_embeddings = nn.Embedding(c.vocab_size, c.hidden_size, padding_idx=getattr(c, "pad_token_id", None))
        self.position_embeddings = nn.Embedding(c.max_position_embeddings, c.hidden_size)
        self.token_type_embeddings = nn.Embedding(c.type_vocab_size, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.register_buffer("position_ids", torch.arange(c.max_position_embeddings).expand((1, -1)))
        self.visual_token_type_embeddings = nn.Embedding(c.type_vocab_size, c.hidden_size)
        self.visual_position_embeddings = nn.Embedding(c.max_position_embeddings, c.hidden_size)
        if getattr(c, "special_visual_initialize", True):            # :95-101
            self.visual_token_type_embeddings.weight.data = self.token_type_embeddings.weight.data.clone()
            self.visual_position_embeddings.weight.data = self.position_embeddings.weight.data.clone()
        self.visual_projection = nn.Linear(c.visual_embedding_dim, c.hidden_size)


class VisualBertSelfAttention(_Container):
    def __init__(self, c):
        super().__init__()
        self.query = nn.Linear(c.hidden_size, c.hidden_size)
        self.key = nn.Linear(c.hidden_size, c.hidden_size)
        self.value = nn.Linear(c.hidden_size, c.hidden_size)
        # per-layer adaptive analogy weights, init U(0, .5) and 0.5 (:223-226)
        self.adaptive_weight = nn.ParameterList([nn.Parameter(torch.empty(1).uniform_(0.0, 0.5)), nn.Parameter(torch.full((1,), 0.5))])


class VisualBertAttention(_Container):
    def __init__(self, c):
        super().__init__()
        self.self = VisualBertSelfAttention(c)
        self.output = BertSelfOutput(c)


class VisualBertIntermediate(_Container):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.intermediate_size)


class VisualBertLayer(_Container):
    def __init__(self, c):
        super().__init__()
        self.attention = VisualBertAttention(c)
        self.intermediate = VisualBertIntermediate(c)
        self.output = BertOutput(c)


class VisualBertEncoder(_Container):
    def __init__(self, c):
        super().__init__()
        self.layer = nn.ModuleList([VisualBertLayer(c) for _ in range(c.num_hidden_layers)])


class VisualBertModel(_Container):
    def __init__(self, c):
        super().__init__()
        self.embeddings = VisualBertEmbeddings(c)
        self.encoder = VisualBertEncoder(c)


def visual_bert_config(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                       max_position_embeddings=512, visual_embedding_dim=2048, layer_norm_eps=1e-12, hidden_dropout_prob=0.1,
                       attention_probs_dropout_prob=0.1):
    """Plain-object stand-in for transformers.VisualBertConfig (attribute access only; the real config object works too).  The defaults are
    VisualBertConfig's, with the visual_embedding_dim of uclanlp/visualbert-vqa-coco-pre (scripts/run_finetune_visualbert.sh)."""
    return SimpleNamespace(vocab_size=vocab_size, hidden_size=hidden_size, num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                           intermediate_size=intermediate_size, hidden_act="gelu", hidden_dropout_prob=hidden_dropout_prob,
                           attention_probs_dropout_prob=attention_probs_dropout_prob, initializer_range=0.02, layer_norm_eps=layer_norm_eps,
                           max_position_embeddings=max_position_embeddings, type_vocab_size=2, visual_embedding_dim=visual_embedding_dim,
                           bypass_transformer=False, special_visual_initialize=True, pad_token_id=1)


class VisualBertForMaskedLM(HipMaskedLM):
    WORD, BIAS = VBERT_WORD, VBERT_BIAS
    ENGINE, PRECISE = VisualBertEngine, PreciseVisualBertForward  # fp32 training (verification mode) is not built for VisualBERT
    no_image_table = "VisualBERT reads region features from pixel_values [B, 72, 2048]; the device image table (image_index) holds pixels only"

    def __init__(self, config):
        super().__init__(config)
        if getattr(config, "bypass_transformer", False):
            raise NotImplementedError("the HIP VisualBERT path implements bypass_transformer=False (the VisualBertConfig default)")
        if getattr(config, "hidden_act", "gelu") != "gelu":
            raise NotImplementedError("the HIP VisualBERT path implements erf GELU")
        self.visual_bert = VisualBertModel(config)
        self.cls = UnimoOnlyMLMHead(config)
        self._tie_and_hook()

    def _make_store(self, named, device):
        n = self.config.num_hidden_layers
        return FlatStore(named, 0, device, order=vbert_layout_order(n), gemm_groups=vbert_gemm_groups(n), dead=(), f16_weight=vbert_f16_weight)

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, head_mask=None, inputs_embeds=None,
                pixel_values=None, visual_attention_mask=None, visual_token_type_ids=None, labels=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, sep_idx=None):
        if position_ids is not None or head_mask is not None or inputs_embeds is not None or visual_token_type_ids is not None or output_attentions:
            raise NotImplementedError("MarT never passes position_ids / head_mask / inputs_embeds / visual_token_type_ids / output_attentions; "
                                      "unsupported on the HIP VisualBERT path")
        if sep_idx is None:
            # the reference shifts sep_idx in place (modeling_visual_bert.py:866): None fails there with this TypeError
            raise TypeError("unsupported operand type(s) for +=: 'NoneType' and 'int' (VisualBERT needs sep_idx: no MarKG pre-train step)")
        if pixel_values is None:
            raise ValueError("VisualBERT needs pixel_values: region features [B, V, visual_embedding_dim]")
        fp32 = self.precision == "fp32"
        if fp32 and (torch.is_grad_enabled() or self.training):
            raise NotImplementedError("precision='fp32' is the VisualBERT evaluation path (model.eval() under torch.no_grad()); "
                                      "fp32 training (verification mode) is not built for VisualBERT")
        if fp32 and labels is not None:
            raise NotImplementedError("precision='fp32': no full-vocabulary labels path; score slices of .logits instead")
        st = self.finalize()
        self._check_trainable()
        dev = st.device
        input_ids, attention_mask, token_type_ids, sep_idx = self._text_inputs(dev, input_ids, attention_mask, token_type_ids, sep_idx)
        pixel_values = pixel_values.to(dev, torch.float32).contiguous()
        if visual_attention_mask is not None:
            visual_attention_mask = visual_attention_mask.to(dev)
        if fp32:
            st.join_pending()
            pr = self._fp32_engine()
            trans = pr.forward(input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, visual_attention_mask)
            return self._pack(trans, self._logits(trans, None, precise=pr), return_dict)
        self._engine.visual_mask = visual_attention_mask
        holder: Dict[str, torch.Tensor] = {}
        self._engine.save_for_backward = torch.is_grad_enabled()
        trans = Fn._MKGformerFn.apply(self._anchor, self._engine, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx,
                                      bool(self.training), self._next_seed(), holder, None, None)
        st.join_pending()
        if labels is not None:
            raise NotImplementedError("labels are [B, L] while the logits cover L + V rows (the reference's CrossEntropyLoss fails on the shapes too); "
                                      "score slices of .logits instead")
        return self._pack(trans, self._logits(trans, holder["trans_bf16"], head_split=self._engine.head_split), return_dict)
