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
from .. import ops
from ..params import FlatStore, refresh_shadows_on_load
from ..vilt_engine import VILT_DEAD, WORD, ViltEngine, vilt_f16_weight, vilt_gemm_groups, vilt_layout_order
from .modeling_flava import FlavaLayer
from .modeling_unimo import MaskedLMOutput, _Container


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


class ViltForMaskedLM(nn.Module):
    def __init__(self, config):
        super().__init__()
        if getattr(config, "hidden_dropout_prob", 0.0) or getattr(config, "attention_probs_dropout_prob", 0.0):
            raise NotImplementedError("the HIP ViLT path implements the ViltConfig defaults (all dropouts 0)")
        if getattr(config, "max_image_length", -1) not in (-1, None):
            raise NotImplementedError("the HIP ViLT path keeps every patch (max_image_length = -1, the ViltConfig default)")
        if getattr(config, "hidden_act", "gelu") != "gelu" or not getattr(config, "qkv_bias", True):
            raise NotImplementedError("the HIP ViLT path implements erf GELU and biased q / k / v projections")
        self.config = config
        self.vilt = ViltModel(config)
        self.mlm_score = ViltMLMHead(config)
        self._store: Optional[FlatStore] = None
        self._engine: Optional[ViltEngine] = None
        self.image_table = None
        self.tie_weights()
        refresh_shadows_on_load(self)

    # embedding surgery (same contract as the MKGformer / FLAVA classes)
    def get_input_embeddings(self):
        return self.vilt.embeddings.text_embeddings.word_embeddings

    def get_output_embeddings(self):
        return self.mlm_score.decoder

    def set_output_embeddings(self, new_embeddings):
        self.mlm_score.decoder = new_embeddings
        self.tie_weights()

    def tie_weights(self):
        dec, emb = self.mlm_score.decoder, self.get_input_embeddings()
        dec.weight = emb.weight
        if self.mlm_score.bias.shape[0] != emb.weight.shape[0]:
            nb = torch.zeros(emb.weight.shape[0], dtype=self.mlm_score.bias.dtype, device=self.mlm_score.bias.device)
            n = min(nb.shape[0], self.mlm_score.bias.shape[0])
            nb[:n] = self.mlm_score.bias.data[:n]
            self.mlm_score.bias = nn.Parameter(nb)
        dec.bias = self.mlm_score.bias
        dec.out_features = emb.num_embeddings

    def resize_token_embeddings(self, new_num_tokens):
        old = self.get_input_embeddings()
        if new_num_tokens is None or new_num_tokens == old.weight.shape[0]:
            return
        w = old.weight.data
        new = nn.Embedding(new_num_tokens, w.shape[1]).to(device=w.device, dtype=w.dtype)
        new.weight.data.normal_(mean=0.0, std=self.config.initializer_range)
        n = min(w.shape[0], new_num_tokens)
        new.weight.data[:n] = w[:n]
        self.vilt.embeddings.text_embeddings.word_embeddings = new
        self._store = self._engine = None
        self.tie_weights()

    def finalize(self, device=None) -> FlatStore:
        if self._store is not None and self._store.still_bound():
            return self._store
        named = dict(self.named_parameters())
        if self._store is not None and self._store.owns(named):
            self._store.bind(self)
            return self._store
        ops.require_gpu()
        if device is None:
            p0 = next(iter(named.values()))
            device = p0.device if p0.is_cuda else torch.device("cuda", torch.cuda.current_device())
        n = self.config.num_hidden_layers
        self._store = FlatStore(named, 0, torch.device(device), order=vilt_layout_order(n), gemm_groups=vilt_gemm_groups(n), dead=VILT_DEAD(),
                                f16_weight=vilt_f16_weight)
        self.tie_weights()
        self._engine = ViltEngine(self._store, self.config)
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        if not hasattr(self, "base_seed"):
            self._step = 0
            self.base_seed = 0x5EED
        if not hasattr(self, "precision"):
            self.precision = "bf16"
        self._store.bind(self)
        return self._store

    @property
    def store(self) -> FlatStore:
        return self.finalize()

    @property
    def engine(self) -> ViltEngine:
        self.finalize()
        return self._engine

    def sync_shadows(self):
        self.finalize().refresh_shadows()

    def set_image_table(self, table: torch.Tensor):
        """Keep the per-entity pixel tensor [N, 3, 384, 384] resident in HBM; batches then carry ``image_index`` [B, 2] (-1 = zero image)."""
        st = self.finalize()
        self.image_table = table.to(st.device, torch.float32).contiguous()

    def set_precision(self, precision: str):
        """"bf16" (training + eval) or "fp32" (evaluation only: fp32 activations, split-bf16 MFMA contractions, fp32 attention;
        engine_precise.PreciseViltForward).  fp32 training (verification mode) is not built for ViLT."""
        if precision not in ("bf16", "fp32"):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        self.precision = precision
        return self

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, pixel_values=None, pixel_mask=None, head_mask=None,
                inputs_embeds=None, image_embeds=None, labels=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                sep_idx=None, image_index=None):
        if pixel_mask is not None or image_embeds is not None or inputs_embeds is not None or head_mask is not None or output_attentions:
            raise NotImplementedError("MarT never passes pixel_mask / image_embeds / inputs_embeds / head_mask / output_attentions; "
                                      "unsupported on the HIP ViLT path")
        if sep_idx is None:
            # the reference shifts sep_idx in place (modeling_vilt.py:844): None fails there with this TypeError, so ViLT has no pre-train step
            raise TypeError("unsupported operand type(s) for +=: 'NoneType' and 'int' (ViLT needs sep_idx: no MarKG pre-train step)")
        fp32 = getattr(self, "precision", "bf16") == "fp32"
        if fp32 and (torch.is_grad_enabled() or self.training):
            raise NotImplementedError("precision='fp32' is the ViLT evaluation path (model.eval() under torch.no_grad()); "
                                      "fp32 training (verification mode) is not built for ViLT")
        if fp32 and labels is not None:
            raise NotImplementedError("precision='fp32': no full-vocabulary labels path; score slices of .logits instead")
        st = self.finalize()
        dev = st.device
        input_ids = input_ids.to(dev, torch.int64).contiguous()
        B, L = input_ids.shape
        attention_mask = torch.ones((B, L), device=dev, dtype=torch.int64) if attention_mask is None else attention_mask.to(dev, torch.int64).contiguous()
        token_type_ids = torch.zeros((B, L), device=dev, dtype=torch.int64) if token_type_ids is None else token_type_ids.to(dev, torch.int64).contiguous()
        sep_idx = sep_idx.to(dev, torch.int64).contiguous()              # (a copy when it lives elsewhere; the engine never writes to it)
        image_table = None
        if image_index is not None:
            if self.image_table is None:
                raise ValueError("image_index given but no image table attached: call model.set_image_table(table) first")
            image_table = self.image_table
            image_index = image_index.to(dev, torch.int32).contiguous()
        else:
            pixel_values = pixel_values.to(dev, torch.float32)
        P = (self.config.image_size // self.config.patch_size) ** 2
        order = draw_patch_order(B, P)                  # the reference's draws, on the default CPU generator (always a permutation)
        if fp32:
            st.join_pending()
            pr = getattr(self, "_precise", None)
            if pr is None or pr.st is not st:
                from ..engine_precise import PreciseViltForward
                pr = self._precise = PreciseViltForward(st, self.config)
            trans = pr.forward(input_ids, attention_mask, token_type_ids, pixel_values, sep_idx, order, image_table=image_table, image_index=image_index)
            out = MaskedLMOutput(loss=None, logits=Fn.LazyLogits(trans, None, st, word_name=WORD, bias_name="mlm_score.bias", precise=pr),
                                 hidden_states=None, attentions=None)
            return (out, trans) if return_dict else ((out.logits,), trans)
        self._engine.patch_order = order
        self._step += 1
        holder: Dict[str, torch.Tensor] = {}
        self._engine.save_for_backward = torch.is_grad_enabled()
        trans = Fn._MKGformerFn.apply(self._anchor, self._engine, input_ids, attention_mask, token_type_ids, pixel_values, sep_idx,
                                      bool(self.training), (self.base_seed * 1000003 + self._step * 7919) & 0x7FFFFFFFFFFF, holder,
                                      image_table, image_index)
        st.join_pending()
        logits = Fn.LazyLogits(trans, holder["trans_bf16"], st, word_name=WORD, bias_name="mlm_score.bias", head_split=self._engine.head_split)
        loss = None
        if labels is not None:
            full = logits.materialize()
            loss = torch.nn.functional.cross_entropy(full.view(-1, full.shape[-1]), labels.to(dev).view(-1))
        out = MaskedLMOutput(loss=loss, logits=logits, hidden_states=None, attentions=None)
        if not return_dict:
            return ((loss, logits) if loss is not None else (logits,)), trans
        return out, trans
