"""FLAVA backbone under the MarT framework (reference: MarT/models/modeling_flava.py:2127-2204 FlavaForMaskedLM,
MarT/models/model.py:31 FlavaKGC) on the gfx950 HIP kernels -- SURVEY 8(a) row 19 / BASELINE config 4.

Only the path MarT runs is implemented: image encoder (12 pre-LN layers over 1+196+196 tokens, FlavaImageEmbeddings quirk
included), text encoder (12 pre-LN layers, FLAVA variant of the adaptive analogy reweight), the two multimodal projections
of the PRE-final-layernorm states, the 6-layer multimodal encoder, final layernorm, MLM head on the text positions.
Poolers, contrastive projections, logit_scale, codebook, ITM/MIM heads exist as parameters (checkpoint compatibility) but are
never evaluated, exactly as in the reference's MarT usage.  Sub-modules are parameter containers; compute is in
``mkg_analogy_amd.flava_engine``.  All dropout probabilities must be 0 (the facebook/flava-full config).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict

import torch
from torch import nn

from .. import functional as Fn
from ..engine_precise import PreciseFlavaForward, PreciseFlavaTrain
from ..flava_engine import FLAVA_DEAD, WORD as FLAVA_WORD, FlavaEngine, flava_f16_weight, flava_gemm_groups, flava_layout_order
from ..params import FlatStore
from ._backbone import HipMaskedLM
from .modeling_unimo import _Container


class FlavaSelfAttention(_Container):
    def __init__(self, H):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H)
        self.adaptive_weight = nn.ParameterList([nn.Parameter(torch.empty(1).uniform_(0.0, 0.5)), nn.Parameter(torch.full((1,), 0.5))])


class FlavaSelfOutput(_Container):
    def __init__(self, H):
        super().__init__()
        self.dense = nn.Linear(H, H)


class FlavaAttention(_Container):
    def __init__(self, H):
        super().__init__()
        self.attention = FlavaSelfAttention(H)
        self.output = FlavaSelfOutput(H)


class _Dense(_Container):
    def __init__(self, i, o):
        super().__init__()
        self.dense = nn.Linear(i, o)


class FlavaLayer(_Container):
    def __init__(self, H, I, eps):
        super().__init__()
        self.attention = FlavaAttention(H)
        self.intermediate = _Dense(H, I)
        self.output = _Dense(I, H)
        self.layernorm_before = nn.LayerNorm(H, eps=eps)
        self.layernorm_after = nn.LayerNorm(H, eps=eps)


class FlavaEncoder(_Container):
    def __init__(self, n, H, I, eps):
        super().__init__()
        self.layer = nn.ModuleList([FlavaLayer(H, I, eps) for _ in range(n)])


class FlavaTextEmbeddings(_Container):
    def __init__(self, c):
        super().__init__()
        self.word_embeddings = nn.Embedding(c.vocab_size, c.hidden_size)
        self.position_embeddings = nn.Embedding(c.max_position_embeddings, c.hidden_size)
        self.token_type_embeddings = nn.Embedding(c.type_vocab_size, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.register_buffer("position_ids", torch.arange(c.max_position_embeddings).expand((1, -1)))


class FlavaTextModel(_Container):
    def __init__(self, c):
        super().__init__()
        self.embeddings = FlavaTextEmbeddings(c)
        self.encoder = FlavaEncoder(c.num_hidden_layers, c.hidden_size, c.intermediate_size, c.layer_norm_eps)
        self.layernorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.pooler = _Dense(c.hidden_size, c.hidden_size)


class PatchEmbeddings(_Container):
    def __init__(self, c):
        super().__init__()
        self.projection = nn.Conv2d(3, c.hidden_size, kernel_size=c.patch_size, stride=c.patch_size)


class FlavaImageEmbeddings(_Container):
    def __init__(self, c):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, c.hidden_size))
        self.mask_token = nn.Parameter(torch.zeros(1, 1, c.hidden_size))
        self.patch_embeddings = PatchEmbeddings(c)
        n = (c.image_size // c.patch_size) ** 2
        self.position_embeddings = nn.Parameter(torch.zeros(1, n + 1, c.hidden_size))


class FlavaImageModel(_Container):
    def __init__(self, c):
        super().__init__()
        self.embeddings = FlavaImageEmbeddings(c)
        self.encoder = FlavaEncoder(c.num_hidden_layers, c.hidden_size, c.intermediate_size, c.layer_norm_eps)
        self.layernorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.pooler = _Dense(c.hidden_size, c.hidden_size)


class FlavaMultimodalModel(_Container):
    def __init__(self, c):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, c.hidden_size))
        self.encoder = FlavaEncoder(c.num_hidden_layers, c.hidden_size, c.intermediate_size, c.layer_norm_eps)
        self.layernorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.pooler = _Dense(c.hidden_size, c.hidden_size)


class FlavaModel(_Container):
    def __init__(self, cfg):
        super().__init__()
        self.logit_scale = nn.Parameter(torch.ones([]) * 2.6592)
        self.text_model = FlavaTextModel(cfg.text_config)
        self.image_model = FlavaImageModel(cfg.image_config)
        self.multimodal_model = FlavaMultimodalModel(cfg.multimodal_config)
        H = cfg.text_config.hidden_size
        self.image_projection = nn.Linear(H, H)
        self.text_projection = nn.Linear(H, H)
        self.image_to_mm_projection = nn.Linear(H, H)
        self.text_to_mm_projection = nn.Linear(H, H)


class FlavaPredictionHeadTransform(_Container):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)


class FlavaMaskedPredictionHead(_Container):
    def __init__(self, c):
        super().__init__()
        self.transform = FlavaPredictionHeadTransform(c)
        self.decoder = nn.Linear(c.hidden_size, c.vocab_size, bias=False)
        self.bias = nn.Parameter(torch.zeros(c.vocab_size))
        self.decoder.bias = self.bias


def flava_config(vocab_size=30522, hidden_size=768, text_layers=12, image_layers=12, mm_layers=6, num_attention_heads=12,
                 intermediate_size=3072, max_position_embeddings=512, image_size=224, patch_size=16, layer_norm_eps=1e-12):
    """Plain-object stand-in for transformers.FlavaConfig (attribute access only; the real config object works too)."""
    common = dict(hidden_size=hidden_size, num_attention_heads=num_attention_heads, intermediate_size=intermediate_size,
                  layer_norm_eps=layer_norm_eps, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    return SimpleNamespace(
        text_config=SimpleNamespace(vocab_size=vocab_size, num_hidden_layers=text_layers, max_position_embeddings=max_position_embeddings,
                                    type_vocab_size=2, initializer_range=0.02, **common),
        image_config=SimpleNamespace(num_hidden_layers=image_layers, image_size=image_size, patch_size=patch_size, **common),
        multimodal_config=SimpleNamespace(num_hidden_layers=mm_layers, **common), initializer_range=0.02)


class FlavaForMaskedLM(HipMaskedLM):
    WORD, BIAS = FLAVA_WORD, "cls.bias"
    ENGINE, PRECISE, PRECISE_TRAIN = FlavaEngine, PreciseFlavaForward, PreciseFlavaTrain
    no_image_table = "FLAVA reads pixels from pixel_values; the device image table (image_index) is not built for this backbone"

    def __init__(self, config):
        super().__init__(config)
        for sub in (config.text_config, config.image_config, config.multimodal_config):
            if getattr(sub, "hidden_dropout_prob", 0.0) or getattr(sub, "attention_probs_dropout_prob", 0.0):
                raise NotImplementedError("the HIP FLAVA path implements the facebook/flava-full configuration (all dropouts 0)")
        self.flava = FlavaModel(config)
        self.cls = FlavaMaskedPredictionHead(config.text_config)
        self._tie_and_hook()

    @property
    def initializer_range(self):
        return self.config.text_config.initializer_range

    def _make_store(self, named, device):
        c = self.config
        nl = (c.text_config.num_hidden_layers, c.image_config.num_hidden_layers, c.multimodal_config.num_hidden_layers)
        return FlatStore(named, 0, device, order=flava_layout_order(*nl), gemm_groups=flava_gemm_groups(*nl), dead=FLAVA_DEAD(nl),
                         f16_weight=flava_f16_weight)

    def forward(self, input_ids=None, pixel_values=None, attention_mask=None, token_type_ids=None, bool_masked_pos=None, position_ids=None,
                image_attention_mask=None, skip_multimodal_encoder=None, output_attentions=None, output_hidden_states=True, return_dict=None,
                labels=None, sep_idx=None):
        if bool_masked_pos is not None or position_ids is not None or image_attention_mask is not None or skip_multimodal_encoder or output_attentions:
            raise NotImplementedError("MarT never passes these FlavaForMaskedLM arguments; unsupported on the HIP path")
        st = self.finalize()
        self._check_trainable()
        dev = st.device
        input_ids, attention_mask, token_type_ids, sep_idx = self._text_inputs(dev, input_ids, attention_mask, token_type_ids, sep_idx)
        pixel_values = pixel_values.to(dev, torch.float32)
        if self.precision == "fp32":
            st.join_pending()
            if labels is not None:
                raise NotImplementedError("precision='fp32': no full-vocabulary labels path; score slices of .logits instead")
            if torch.is_grad_enabled():
                # verification mode: fp32-accurate forward AND backward (engine_precise.PreciseFlavaTrain); eval-mode gradients
                pr = self._fp32_engine(train=True)
                trans = Fn._MKGformerFn.apply(self._anchor, pr, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, False, 0, {})
                return self._pack(trans, self._logits(trans, None, precise=pr), return_dict)
            if self.training:
                raise NotImplementedError("precision='fp32' under no_grad is the evaluation path: call model.eval() (or set_precision('bf16'))")
            pr = self._fp32_engine()
            trans = pr.forward(input_ids, attention_mask, token_type_ids, pixel_values, sep_idx)
            return self._pack(trans, self._logits(trans, None, precise=pr), return_dict)
        holder: Dict[str, torch.Tensor] = {}
        self._engine.save_for_backward = torch.is_grad_enabled()
        trans = Fn._MKGformerFn.apply(self._anchor, self._engine, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx,
                                      bool(self.training), self._next_seed(), holder)
        st.join_pending()                           # gradient zero-fill / W^T refresh issued next to this forward pass (optim.FusedAdamW)
        logits = self._logits(trans, holder["trans_bf16"], head_split=self._engine.head_split)
        loss = None
        if labels is not None:
            full = logits.materialize()
            loss = torch.nn.functional.cross_entropy(full.view(-1, full.shape[-1]), labels.to(dev).view(-1))
        return self._pack(trans, logits, return_dict, loss=loss)
