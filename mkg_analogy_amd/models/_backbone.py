"""The host-side shell every backbone class shares: weight tying and embedding resize, the flat parameter store and the engines behind it, the
dropout-seed and precision state, and the parts of a forward pass that run before the first kernel and after the last.

A backbone class derives from ``HipMaskedLM``, builds its parameter-container tree in its constructor (after ``super().__init__(config)``,
ending with ``self._tie_and_hook()``) and supplies

* ``WORD`` / ``BIAS``: the parameter names of the word embedding and of the decoder bias.  They say where the embedding lives and which module
  holds ``.decoder`` and ``.bias``, and they are the names ``functional.LazyLogits`` scores with;
* ``ENGINE``, ``PRECISE`` and (where fp32 training is built) ``PRECISE_TRAIN``: the engine classes, all constructed as ``cls(store, *self._cfgs)``
  (``_cfgs`` is ``(config,)`` unless the constructor sets it);
* ``_make_store(named, device)``: its ``FlatStore`` layout;
* ``no_image_table``: the refusal message of ``set_image_table`` when the backbone takes no device image table;
* ``forward``: its own keyword set and refusals (all of them before ``finalize()`` is reached), built on the ``_text_inputs`` / ``_image_inputs`` /
  ``_next_seed`` / ``_fp32_engine`` / ``_logits`` / ``_pack`` helpers below.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional

import torch
from torch import nn

from .. import functional as Fn
from .. import ops
from ..params import FlatStore, refresh_shadows_on_load


class MaskedLMOutput(SimpleNamespace):
    """Duck-type of transformers.modeling_outputs.MaskedLMOutput: ``out.logits`` and ``out[0]`` style access."""

    def __getitem__(self, i):
        return [v for v in (self.loss, self.logits, self.hidden_states, self.attentions) if v is not None][i]


class HipMaskedLM(nn.Module):
    WORD: str
    BIAS: str
    ENGINE: type
    PRECISE: type
    PRECISE_TRAIN: Optional[type] = None
    no_image_table: Optional[str] = None

    def __init__(self, config):
        super().__init__()
        self.config = config
        self._cfgs: tuple = (config,)               # what every engine constructor takes after the store
        self._store: Optional[FlatStore] = None
        self._engine = None
        self._precise = None                        # fp32-accurate engines (engine_precise), built on first use: see _fp32_engine
        self._precise_train = None
        self._step = 0
        self.base_seed = 0x5EED                     # dropout stream; distributed.GradSync hashes the rank into it
        self.precision = "bf16"
        self.image_table = None                     # optional resident [N_img, 3, S, S] f32 table for device-side batch assembly
        self._flags = None                          # requires_grad of every parameter as sync_trainable() last read it (name, flag) -- the plan in use
        self._extra_dead: tuple = ()

    def _tie_and_hook(self):
        """Last line of a subclass constructor, once the parameter containers exist."""
        self.tie_weights()
        refresh_shadows_on_load(self)

    @staticmethod
    def add_to_argparse(parser):
        parser.add_argument("--pretrain", type=int, default=0, help="")
        return parser

    # ------------------------------------------------------------------ embedding surgery (modeling_unimo.py:895-930)
    def _head(self) -> nn.Module:
        return self.get_submodule(self.BIAS.rpartition(".")[0])

    @property
    def initializer_range(self) -> float:
        return self.config.initializer_range

    def get_input_embeddings(self) -> nn.Embedding:
        return self.get_submodule(self.WORD.rpartition(".")[0])

    def get_output_embeddings(self) -> nn.Linear:
        return self._head().decoder

    def set_output_embeddings(self, new_embeddings):
        """The decoder is always tied: scoring reads the word embedding by name from the store."""
        self._head().decoder = new_embeddings
        self.tie_weights()

    def tie_weights(self):
        head, emb = self._head(), self.get_input_embeddings()
        dec = head.decoder
        dec.weight = emb.weight
        if head.bias.shape[0] != emb.weight.shape[0]:                   # zero-pad / truncate the decoder bias on resize
            nb = torch.zeros(emb.weight.shape[0], dtype=head.bias.dtype, device=head.bias.device)
            n = min(nb.shape[0], head.bias.shape[0])
            nb[:n] = head.bias.data[:n]
            head.bias = nn.Parameter(nb)
        dec.bias = head.bias
        dec.out_features = emb.num_embeddings

    def resize_token_embeddings(self, new_num_tokens):
        old = self.get_input_embeddings()
        if new_num_tokens is None or new_num_tokens == old.weight.shape[0]:
            return
        w = old.weight.data
        new = nn.Embedding(new_num_tokens, w.shape[1]).to(device=w.device, dtype=w.dtype)
        new.weight.data.normal_(mean=0.0, std=self.initializer_range)   # _init_text_weights, :768-771
        n = min(w.shape[0], new_num_tokens)
        new.weight.data[:n] = w[:n]
        parent, _, leaf = self.WORD.rpartition(".")[0].rpartition(".")
        setattr(self.get_submodule(parent), leaf, new)
        self._store = self._engine = None
        self.tie_weights()

    # ------------------------------------------------------------------ flat storage / engines
    def _make_store(self, named: Dict[str, nn.Parameter], device: torch.device) -> FlatStore:
        raise NotImplementedError

    def _make_engine(self, store: FlatStore):
        return self.ENGINE(store, *self._cfgs)

    def finalize(self, device=None) -> FlatStore:
        """Move the parameters into the flat fp32/bf16 buffers the kernels use (idempotent).  Leaves the seed, the step counter and the precision
        alone, so a re-finalize (after resize_token_embeddings, .cpu() / .cuda(), a re-assigned Parameter) keeps them."""
        if self._store is not None and self._store.still_bound():
            return self._store
        named = dict(self.named_parameters())         # tied decoder weight/bias are deduplicated by torch
        if self._store is not None and self._store.owns(named):
            self._store.bind(self)
            return self._store
        ops.require_gpu()
        if device is None:
            p0 = next(iter(named.values()))
            device = p0.device if p0.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self._store = self._make_store(named, torch.device(device))
        self.tie_weights()
        self._engine = self._make_engine(self._store)
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        self._store.bind(self)
        self._flags = None
        self.sync_trainable(self._extra_dead)         # a new store starts from the flags as they are now
        return self._store

    # ------------------------------------------------------------------ frozen parameters
    # ONE rule for "what is trainable": requires_grad = True minus the store's dead tensors, read at ONE moment -- sync_trainable(), which
    # lit_models' configure_optimizers() calls before it builds the optimizer.  The store (AdamW chunk table) and the engine (backward schedule) are
    # told together; a flag that moves afterwards is refused at the next training forward pass instead of being half honoured.
    def _select(self, prefixes):
        named = list(self.named_parameters())
        if not prefixes:
            return [p for _, p in named]
        hit = [p for n, p in named if n.startswith(tuple(prefixes))]
        if not hit:
            raise ValueError(f"no parameter name starts with any of {list(prefixes)}")
        return hit

    def freeze(self, *name_prefixes: str):
        """``requires_grad_(False)`` on every parameter whose name starts with one of the prefixes (none given: all).  Flags only: call
        ``sync_trainable()`` (or the lit model's ``configure_optimizers()``) afterwards."""
        for p in self._select(name_prefixes):
            p.requires_grad_(False)
        return self

    def unfreeze(self, *name_prefixes: str):
        for p in self._select(name_prefixes):
            p.requires_grad_(True)
        return self

    def _read_flags(self):
        return tuple((n, bool(p.requires_grad)) for n, p in self.named_parameters())

    def sync_trainable(self, extra_dead=()):
        """Read ``requires_grad`` of every parameter NOW and hand the trainable set to the store and the engine: frozen tensors get no AdamW update
        (no weight decay, untouched m / v / master / shadows), the MKGformer bf16 engine drops the backward launches nobody consumes
        (mkg_analogy_amd/freeze.py), and whatever an engine still writes for a frozen tensor is cleared with the step.  ``extra_dead``: run-mode
        specific tensors that never receive a gradient (FlatStore.rebuild_chunks).  When the set changes the gradient buffer is zero-filled once.
        Returns the trainable names."""
        st = self.finalize()
        flags = self._read_flags()
        changed = self._flags is not None and (flags != self._flags or tuple(extra_dead) != self._extra_dead)    # (None: a new store, all-zero already)
        self._flags, self._extra_dead = flags, tuple(extra_dead)
        self._plist = [p for _, p in self.named_parameters()]
        self._fingerprint = tuple(f for _, f in flags)
        self._apply_trainable()
        if changed:
            st.zero_grad()
        return st.trainable_names()

    def _apply_trainable(self):
        """Store + engine follow ``self._flags`` (the engine that the current precision runs decides which frozen tensors are still written)."""
        st = self._store
        frozen = frozenset(n for n, f in self._flags if not f)
        st.rebuild_chunks(self._extra_dead, frozen=frozen)
        written = None
        if hasattr(self._engine, "set_trainable"):
            written = self._engine.set_trainable(st.trainable_names())
            if self.precision != "bf16":
                written = None                         # the fp32 engines run every launch (tier 2: the optimizer alone honours the flags)
        st.rebuild_chunks(self._extra_dead, written=written)
        # nothing trainable at all: the output needs no gradient, and loss.backward() fails as torch does for such an output
        self._anchor.requires_grad_(bool(st.trainable_names()))

    def _check_trainable(self):
        """First thing in a training forward pass under grad: the flags must be the ones the plan in use was made from."""
        if not (self.training and torch.is_grad_enabled()) or self._flags is None:
            return
        if tuple(p.requires_grad for p in self._plist) == self._fingerprint:      # ~450 attribute reads; no walk of the module tree
            return
        n = next(n for (n, f), p in zip(self._flags, self._plist) if f != bool(p.requires_grad))
        raise RuntimeError(f"requires_grad of '{n}' changed after the trainable set was read: call configure_optimizers() / "
                           f"model.sync_trainable() again (the optimizer and the backward schedule still follow the old set)")

    @property
    def store(self) -> FlatStore:
        return self.finalize()

    @property
    def engine(self):
        self.finalize()
        return self._engine

    def _fp32_engine(self, train: bool = False):
        """The fp32-accurate engine over the CURRENT store (call after finalize()); rebuilt when the store was replaced."""
        eng = self._precise_train if train else self._precise
        if eng is None or eng.st is not self._store:
            eng = (self.PRECISE_TRAIN if train else self.PRECISE)(self._store, *self._cfgs)
            if train:
                self._precise_train = eng
            else:
                self._precise = eng
        return eng

    def sync_shadows(self):
        """Call after editing parameters in place (e.g. _init_relation_word) so the bf16 GEMM operands follow."""
        self.finalize().refresh_shadows()

    def set_precision(self, precision: str):
        """"bf16" (default: bf16 MFMA operands, fp32 accumulation / residual streams; training + eval) or "fp32" (fp32 activations, split-bf16 MFMA
        contractions, fp32 attention -- meets the reference's fp32 results to ~1e-4 on logits; see engine_precise.py).  "fp32" is the evaluation
        path under no_grad; MKGformer and FLAVA also run a verification-mode training step in it (eval-mode gradients, no dropout replay) when
        gradients are enabled, ViLT and VisualBERT refuse that."""
        if precision not in ("bf16", "fp32"):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        changed, self.precision = precision != self.precision, precision
        if changed and self._store is not None and self._flags is not None and not all(f for _, f in self._flags):
            self._apply_trainable()                    # which frozen tensors are still written depends on the engine that runs
        return self

    def set_image_table(self, table: torch.Tensor):
        """Keep the per-entity pixel tensor (MarT/tools/encode_images_data.py output, data_module.py:209) resident in HBM so that batches carry
        ``image_index`` [B, 2] row indices (-1 = zero image) instead of 1.2 MB of pixels per example."""
        if self.no_image_table:
            raise NotImplementedError(self.no_image_table)
        st = self.finalize()
        self.image_table = table.to(st.device, torch.float32).contiguous()

    # ------------------------------------------------------------------ the ends of a forward pass
    @staticmethod
    def _text_inputs(dev, input_ids, attention_mask, token_type_ids, sep_idx):
        """int64, contiguous, on the store's device; all-ones mask and all-zero types by default.  (``sep_idx`` is copied when it lives elsewhere;
        no engine writes to it.)"""
        input_ids = input_ids.to(dev, torch.int64).contiguous()
        B, L = input_ids.shape
        attention_mask = torch.ones((B, L), device=dev, dtype=torch.int64) if attention_mask is None else attention_mask.to(dev, torch.int64).contiguous()
        token_type_ids = torch.zeros((B, L), device=dev, dtype=torch.int64) if token_type_ids is None else token_type_ids.to(dev, torch.int64).contiguous()
        if sep_idx is not None:
            sep_idx = sep_idx.to(dev, torch.int64).contiguous()
        return input_ids, attention_mask, token_type_ids, sep_idx

    def _image_inputs(self, dev, pixel_values, image_index):
        """(pixel_values, image_table, image_index): pixels on the device, or -- device-side batch assembly, mkg_analogy_amd.batching.DeviceImageTable --
        the attached table and int32 row indices."""
        if image_index is None:
            return pixel_values.to(dev, torch.float32), None, None
        if self.image_table is None:
            raise ValueError("image_index given but no image table attached: call model.set_image_table(table) first")
        return pixel_values, self.image_table, image_index.to(dev, torch.int32).contiguous()

    def _next_seed(self) -> int:
        """Counts one bf16 pass and returns its dropout seed (distributed.rank_seed keeps this injective across ranks)."""
        self._step += 1
        return (self.base_seed * 1000003 + self._step * 7919) & 0x7FFFFFFFFFFF

    def _logits(self, trans, trans_bf16, **kw) -> Fn.LazyLogits:
        return Fn.LazyLogits(trans, trans_bf16, self._store, word_name=self.WORD, bias_name=self.BIAS, **kw)

    @staticmethod
    def _pack(trans, logits, return_dict, loss=None, hidden_states=None):
        if not return_dict:
            return tuple(v for v in (loss, logits, hidden_states) if v is not None), trans
        return MaskedLMOutput(loss=loss, logits=logits, hidden_states=hidden_states, attentions=None), trans
