"""TransformerLitModel: loss, ranking eval, metrics and optimizer config of the MarT trainer surface
(reference: MarT/lit_models/transformer.py:18-262), with every tensor op on the HIP kernels.

Same constructor, hooks and return types; differences that do not change results:
  * ``logits`` is a lazy object -- only the [MASK] row x the scored vocabulary slice is ever computed,
  * the [MASK] position is found on the device (no ``nonzero`` host sync),
  * ranks are computed as 1 + #(logit > logit[label]) instead of two full sorts (identical without ties),
  * AdamW is the fused multi-tensor kernel over the flat parameter buffer.
"""
from functools import partial

import numpy as np
import torch

from .. import functional as Fn
from ..optim import FusedAdamW, LinearWarmupSchedule, TorchOptimizerOnStore
from .base import BaseLitModel
from .utils import LabelSmoothSoftmaxCEV1


def decode(output_ids, tokenizer):
    return [s.strip() for s in tokenizer.batch_decode(output_ids, skip_special_tokens=False, clean_up_tokenization_spaces=True)]


class TransformerLitModel(BaseLitModel):
    def __init__(self, model, args, tokenizer=None, data_config={}):
        super().__init__(model, args)
        self.save_hyperparameters(args)
        if args.label_smoothing != 0.0:
            self.loss_fn = LabelSmoothSoftmaxCEV1(lb_smooth=args.label_smoothing)
        else:
            self.loss_fn = LabelSmoothSoftmaxCEV1(lb_smooth=0.0)        # plain CE == label smoothing with eps 0
        self.best_acc = 0
        self.first = True
        self.tokenizer = tokenizer
        self.__dict__.update(data_config)
        self.model.resize_token_embeddings(len(self.tokenizer))
        self.alpha = args.alpha
        self._ids_cache = {}
        # tell the model which rows of trans_hidden_states this step reads ([MASK] + the four relaxation-loss rows): the last text layer and the
        # head transform then run on those rows only (UnimoForMaskedLM.forward: needed_rows).  MART_LAST_ROWS=0: every row, as the reference.
        import os
        self.last_layer_rows = os.environ.get("MART_LAST_ROWS", "1") == "1"

    # -- lit_models/transformer.py:41-54
    def _init_relation_word(self):
        self.tokenizer.add_special_tokens({"additional_special_tokens": ["[R]"]})
        self.model.resize_token_embeddings(len(self.tokenizer))
        self.decode = partial(decode, tokenizer=self.tokenizer)
        with torch.no_grad():
            emb = self.model.get_input_embeddings()
            rel_word = [a[0] for a in self.tokenizer(["[R]"], add_special_tokens=False)["input_ids"]]
            src = torch.as_tensor(list(self.analogy_relation_ids), dtype=torch.long, device=emb.weight.device)
            for idx in rel_word:
                emb.weight[idx] = torch.mean(emb.weight[src], dim=0)
            assert self.model.get_input_embeddings().weight is self.model.get_output_embeddings().weight
        if getattr(self.model, "_store", None) is not None:
            self.model.sync_shadows()

    def _ids(self, key):
        v = getattr(self, key)
        dev = self.model.store.device
        c = self._ids_cache.get(key)
        if c is None or c.device != dev:
            c = torch.as_tensor(list(v) if not torch.is_tensor(v) else v, dtype=torch.int32, device=dev).contiguous()
            self._ids_cache[key] = c
        return c

    def _needed(self, input_ids, extra):
        """kwargs for the model call: the token positions whose trans_hidden_states rows this step reads."""
        if not self.last_layer_rows or not getattr(self.model, "accepts_needed_rows", False) or getattr(self.model, "precision", "bf16") != "bf16":
            return {}
        dev = self.model.store.device
        # one device launch: [MASK] position (an example without [MASK]: its row 0, flagged for Fn.check_status -- the row mask_rows() falls back to as well)
        # + the four relaxation-loss positions, as flat int32 row ids
        return dict(needed_rows=Fn.needed_rows(input_ids.to(dev, torch.int64), int(self.tokenizer.mask_token_id), extra))

    def _mask_rows(self, logits, input_ids):
        return logits.mask_rows(input_ids, int(self.tokenizer.mask_token_id))

    # -- lit_models/transformer.py:59-113
    def training_step(self, batch, batch_idx):
        label = batch.pop("label")
        batch.pop("rel_label", None)
        pre_type = batch.pop("pre_type", None)
        rel_idx = batch.pop("rel_idx", None)
        q_head_idx = batch.pop("q_head_idx", None)
        a_head_idx = batch.pop("a_head_idx", None)
        input_ids = batch["input_ids"]
        if "VisualBertKGC" in str(type(self.model)):
            if self.args.pretrain:
                raise NotImplementedError("VisualBertKGC has no MarKG pre-train step on the HIP path: the model needs sep_idx, which pre-train batches "
                                          "do not carry (fine-tune only, scripts/run_finetune_visualbert.sh)")
            # lit_models/transformer.py:98-102: trans_hidden_states covers [text | regions] and the relaxation-loss rows are read V rows further down
            # (partly in region territory -- the reference's behaviour, reproduced); the [MASK] row is read unshifted.  New tensors: the batch keeps its own
            img_len = int(batch["pixel_values"].shape[1])
            rel_idx, q_head_idx, a_head_idx = rel_idx + img_len, q_head_idx + img_len, a_head_idx + img_len
        model_output = self.model(**batch, return_dict=True, **self._needed(input_ids, None if self.args.pretrain else (rel_idx, q_head_idx, a_head_idx)))
        logits = model_output[0].logits
        dev = logits.trans.device
        label = label.to(dev)
        rows = self._mask_rows(logits, input_ids.to(dev))
        if self.args.pretrain:
            pre_type = pre_type.to(dev)
            loss = 0
            entity_mask = (pre_type != 2).nonzero(as_tuple=True)[0]
            if len(entity_mask) > 0:
                loss = loss + self.loss_fn(rows[entity_mask, self.entity_id_st:self.entity_id_ed], label[entity_mask])
            relation_mask = (pre_type == 2).nonzero(as_tuple=True)[0]
            if len(relation_mask) > 0:
                loss = loss + self.loss_fn(rows[relation_mask, self.relation_id_st:self.relation_id_ed], label[relation_mask])
        else:
            mask_logits = rows[:, self._ids("analogy_entity_ids")]
            trans_hidden_states = model_output[1]
            sim_loss = Fn.relaxation_loss(trans_hidden_states, rel_idx.to(dev), q_head_idx.to(dev), a_head_idx.to(dev))
            loss = self.loss_fn(mask_logits, label) + self.alpha * sim_loss
        if batch_idx == 0 and getattr(self, "decode", None) is not None and getattr(self.args, "print_first_batch", False):
            print("\n".join(self.decode(batch["input_ids"][:4])))
        return loss

    # -- lit_models/transformer.py:115-166
    @torch.no_grad()
    def _eval(self, batch, batch_idx):
        label = batch.pop("label")
        pre_type = batch.pop("pre_type", None)
        for k in ("rel_idx", "rel_label", "q_head_idx", "a_head_idx"):
            batch.pop(k, None)
        input_ids = batch["input_ids"]
        model_output = self.model(**batch, return_dict=True, **self._needed(input_ids, None))
        logits = model_output[0].logits
        dev = logits.trans.device
        label = label.to(dev)
        rows = self._mask_rows(logits, input_ids.to(dev))
        if self.args.pretrain:
            pre_type = pre_type.to(dev)
            out = {}
            entity_mask = (pre_type != 2).nonzero(as_tuple=True)[0]
            if len(entity_mask) > 0:
                lg = rows[entity_mask, self.entity_id_st:self.entity_id_ed]
                out["entity_ranks"] = Fn.entity_ranks(lg, label[entity_mask]).cpu().numpy()
            relation_mask = (pre_type == 2).nonzero(as_tuple=True)[0]
            if len(relation_mask) > 0:
                lg = rows[relation_mask, self.relation_id_st:self.relation_id_ed]
                out["relation_ranks"] = Fn.entity_ranks(lg, label[relation_mask]).cpu().numpy()
            if not out:
                raise ValueError("entity and relation cannot be None at the same time.")
            return out
        mask_logits = rows[:, self._ids("analogy_entity_ids")]
        return dict(entity_ranks=Fn.entity_ranks(mask_logits, label).cpu().numpy())

    def _eval_at(self, batch, batch_idx, step=None, **kw):
        """Validation / test / predict batches are scored on the fp32-accurate path (engine_precise) by default: the reference evaluates in fp32 and the
        acceptance criterion for this step is bit-exact ranked entity indices (lit_models/transformer.py:162-164), which a bf16 forward can only
        meet where the margin exceeds its logit error.  3.3 x the time of a bf16 evaluation pass (2.4 k against 8 k examples/s on one MI355X).
        ``args.eval_precision = "bf16"`` (or MART_EVAL_PRECISION=bf16) evaluates in the training configuration.  ``step``: the hook body run under the
        switch (default ``_eval``; ``predict_step`` passes ``_predict``)."""
        import os
        step = self._eval if step is None else step
        prec = getattr(self.args, "eval_precision", None) or os.environ.get("MART_EVAL_PRECISION", "fp32")
        if not hasattr(self.model, "set_precision"):
            prec = None
        cur = getattr(self.model, "precision", "bf16")
        if not prec or prec == cur:
            return step(batch, batch_idx, **kw)
        old = cur
        self.model.set_precision(prec)
        try:
            return step(batch, batch_idx, **kw)
        finally:
            self.model.set_precision(old)

    def validation_step(self, batch, batch_idx):
        return self._eval_at(batch, batch_idx)

    def test_step(self, batch, batch_idx):
        return self._eval_at(batch, batch_idx)

    # -- answering a query: the k best entities of (head, relation, ?).  No counterpart in the reference's lit model (pl.Trainer.predict would need
    # one); the selection is mart_topk, in the order of the reference's descending stable sort (lit_models/transformer.py:162).
    @torch.no_grad()
    def _predict(self, batch, batch_idx, k=None):
        k = int(getattr(self.args, "predict_topk", None) or 10) if k is None else int(k)
        if k < 1:
            raise ValueError(f"predict_step: k must be positive, got {k}")
        label = batch.pop("label", None)
        pre_type = batch.pop("pre_type", None)
        for key in ("rel_idx", "rel_label", "q_head_idx", "a_head_idx"):
            batch.pop(key, None)
        if self.args.pretrain and "VisualBertKGC" in str(type(self.model)):
            raise NotImplementedError("VisualBertKGC has no MarKG pre-train step on the HIP path (fine-tune only)")
        input_ids = batch["input_ids"]
        model_output = self.model(**batch, return_dict=True, **self._needed(input_ids, None))
        logits = model_output[0].logits
        dev = logits.trans.device
        rows = self._mask_rows(logits, input_ids.to(dev))
        if label is not None:
            label = label.to(dev)

        def best(lg, lab, name, out):
            kk = min(k, Fn.TOPK_MAX, int(lg.shape[1]))           # clamped to the scored slice (and to the kernel's list length)
            values, indices = Fn._topk_i32(lg, kk)
            ranks = Fn.entity_ranks(lg, lab) if lab is not None else None     # the same logits: the model ran once, the [MASK] rows were scored once
            out[f"{name}_topk"] = indices.cpu().numpy().astype(np.int64)
            out[f"{name}_topk_logits"] = values.cpu().numpy()
            if ranks is not None:
                out[f"{name}_ranks"] = ranks.cpu().numpy()

        out = {}
        if self.args.pretrain:
            if pre_type is None:
                raise ValueError("predict_step in pre-train mode needs pre_type (which examples ask for an entity, which for a relation)")
            pre_type = pre_type.to(dev)
            for name, sel, st, ed in (("entity", pre_type != 2, self.entity_id_st, self.entity_id_ed),
                                      ("relation", pre_type == 2, self.relation_id_st, self.relation_id_ed)):
                idx = sel.nonzero(as_tuple=True)[0]
                if len(idx) > 0:
                    out[f"{name}_rows"] = idx.cpu().numpy()
                    best(rows[idx, st:ed], None if label is None else label[idx], name, out)
            if not out:
                raise ValueError("entity and relation cannot be None at the same time.")
            return out
        best(rows[:, self._ids("analogy_entity_ids")], label, "entity", out)
        return out

    def predict_step(self, batch, batch_idx, k=None):
        """The ``k`` best answers of every example, as host numpy arrays (``k``: ``args.predict_topk`` if present, else 10; clamped to the scored
        slice).  ``label`` is optional: with it the ranks of ``validation_step`` ride along, from the same logits.
        Fine-tune: ``entity_topk`` int64 [B, k] in the label's index space (positions in ``analogy_entity_ids``; ``KGC.describe_entities`` names
        them), ``entity_topk_logits`` float32 [B, k], ``entity_ranks`` [B] with labels.  Pre-train: ``entity_rows`` / ``relation_rows`` (batch
        positions by ``pre_type``), ``entity_topk`` / ``relation_topk`` (indices inside the entity / relation slice), ``*_topk_logits`` and, with
        labels, ``*_ranks``.  Lists come in the order of a descending stable sort: equal logits by ascending index, a NaN logit first.
        Same precision switch as ``validation_step``; ``Fn.check_status()`` reports an example without [MASK] as there."""
        return self._eval_at(batch, batch_idx, step=self._predict, k=k)

    # -- lit_models/transformer.py:173-222
    def _epoch_end(self, outputs):
        entity_ranks = [o["entity_ranks"] for o in outputs if "entity_ranks" in o]
        if len(entity_ranks) > 0:
            r = np.concatenate(entity_ranks)
            for k in (1, 3, 5, 10, 20):
                self.log(f"Eval_entity/hits{k}", (r <= k).mean())
            self.log("Eval_entity/mean_rank", r.mean())
            self.log("Eval_entity/mrr", (1.0 / r).mean())
            self.log("entity_hits10", (r <= 10).mean(), prog_bar=True)
            self.log("entity_hits1", (r <= 1).mean(), prog_bar=True)

    def validation_epoch_end(self, outputs) -> None:
        self._epoch_end(outputs)

    def test_epoch_end(self, outputs) -> None:
        self._epoch_end(outputs)

    # -- lit_models/transformer.py:224-241
    def configure_optimizers(self):
        dead = [n for n in self.model.store.slots if "adaptive_weight" in n] if self.args.pretrain else []
        # the trainable set is read HERE, once: requires_grad (the reference filters on it, transformer.py:228-229) minus the tensors that never get a
        # gradient (pretrain: no sep_idx => the adaptive weights get grad None in the reference => torch never touches them)
        if hasattr(self.model, "sync_trainable"):
            self.model.sync_trainable(extra_dead=dead)
        if self.optimizer_name == "AdamW":
            optimizer = FusedAdamW(self.model, lr=self.lr, eps=1e-8, weight_decay=self.args.weight_decay)
        else:                           # base.py:31: any torch.optim class by name (torch's own update on the fp32 master views; not the fused path)
            optimizer = TorchOptimizerOnStore(self.model, self.optimizer_name, lr=self.lr, eps=1e-8, weight_decay=self.args.weight_decay, extra_dead=dead)
        steps = self.num_training_steps
        scheduler = LinearWarmupSchedule(optimizer, num_warmup_steps=steps * self.args.warm_up_radio, num_training_steps=steps)
        return {"optimizer": optimizer, "lr_scheduler": {"scheduler": scheduler, "interval": "step", "frequency": 1}}

    # -- the reference's two freezing hooks (lit_models/transformer.py:243-254), by their substring rule.  Flags only: call them before
    # configure_optimizers(), which reads the flags (HipMaskedLM.sync_trainable); a later change is refused at the next training forward pass.
    def _set_word_rule(self, keep_word: bool):
        for name, p in self.model.named_parameters():
            if ("word" in name) != keep_word:
                p.requires_grad_(False)

    def _freeze_attention(self):
        """Only the parameters whose name contains "word" (the tied word embedding) stay trainable."""
        self._set_word_rule(keep_word=True)

    def _freeze_word_embedding(self):
        """The parameters whose name contains "word" are frozen; everything else keeps its flag."""
        self._set_word_rule(keep_word=False)

    @staticmethod
    def add_to_argparse(parser):
        parser = BaseLitModel.add_to_argparse(parser)
        parser.add_argument("--label_smoothing", type=float, default=0.1, help="")
        parser.add_argument("--bce", type=int, default=0, help="")
        return parser
