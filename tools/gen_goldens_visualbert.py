"""G11 / G11b: golden vectors of the UNMODIFIED reference VisualBertForMaskedLM (MarT/models/modeling_visual_bert.py) at real dimensions.

Run where the reference tree is available (it is not needed by any test):

    python tools/gen_goldens_visualbert.py --ref <path to the MarT checkout>      # writes tests/golden/g11_visualbert_real.npz, g11b_visualbert_odd.npz

TEST INFRASTRUCTURE ONLY: the reference module is imported in place (nothing of it is copied), only inputs and outputs are stored.
Shims for transformers 5.x, with the transformers==4.19.0 semantics the reference was written against: ``apply_chunking_to_forward``,
``find_pruneable_heads_and_indices`` and ``prune_linear_layer`` made visible in ``transformers.modeling_utils`` (the module imports them from
there), ``config.is_decoder = False``, ``init_weights`` a no-op (the weights come from ``data_synth.seeded_weights``), ``get_head_mask`` ->
[None] * n, the extended mask (1 - m) * -10000, the decoder tied by hand.

G11   B = 2, L = 64, V = 72, vocabulary 42007, VisualBertConfig(visual_embedding_dim=2048) (768 wide, 12 post-LN layers: S = 136), eval mode,
      fine-tune loss (alpha 0.43, scripts/run_finetune_visualbert.sh) with the lit model's + V shift of rel_idx / q_head_idx / a_head_idx
      (lit_models/transformer.py:98-102); all regions present.
G11b  B = 3, L = 37 (padded text rows, S = 109); example 1 has the second entity's 36 regions zero and masked, example 2 all 72.
      Region features are NOT stored: ``region_features(B, seed, mask)`` below regenerates them (|N(0, 1)|, zero where masked -- the collate's
      zero blocks).  Stored: the visual attention mask, mask logits over the 2063 analogy entities, the trans_hidden rows the loss reads
      (already shifted) and the [MASK] row, the loss, ranks, every gradient norm, strided gradient samples, the parameter names, and the
      bf16-weight control (the same forward with every weight rounded to bf16).
"""
from __future__ import annotations

import argparse as ap
import importlib.util
import os
import sys
import time

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mkg_analogy_amd import data_synth as D  # noqa: E402
from oracle import mkgformer_oracle as O  # noqa: E402

ALPHA = 0.43
V, FEAT = 72, 2048
WORD, BIAS = "visual_bert.embeddings.word_embeddings.weight", "cls.predictions.bias"


def region_features(B: int, seed: int, mask: torch.Tensor) -> torch.Tensor:
    """[B, 72, 2048] f32 stand-in for Faster R-CNN region features (non-negative, as post-ReLU pooled features are); masked regions are the
    collate's zero blocks."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn((B, V, FEAT), generator=g).abs() * mask[:, :, None].to(torch.float32)


def visual_mask(B: int, odd: bool) -> torch.Tensor:
    m = torch.ones((B, V), dtype=torch.float32)
    if odd:
        m[1, V // 2:] = 0.0                        # single-entity example: (entity, zeros)
        m[2] = 0.0                                 # no entity at all
    return m


def load_reference_visualbert(ref: str):
    import transformers.modeling_utils as mu
    import transformers.pytorch_utils as pu
    for n in ("apply_chunking_to_forward", "prune_linear_layer"):
        if not hasattr(mu, n):
            setattr(mu, n, getattr(pu, n))
    if not hasattr(mu, "find_pruneable_heads_and_indices"):
        mu.find_pruneable_heads_and_indices = getattr(pu, "find_pruneable_heads_and_indices",
                                                      lambda *a, **k: (_ for _ in ()).throw(NotImplementedError()))
    spec = importlib.util.spec_from_file_location("ref_visual_bert", os.path.join(ref, "models/modeling_visual_bert.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.VisualBertPreTrainedModel.init_weights = lambda self: None
    m.VisualBertPreTrainedModel.get_head_mask = lambda self, head_mask, n, *a, **k: [None] * n
    m.VisualBertPreTrainedModel.get_extended_attention_mask = \
        lambda self, mask, shape=None, device=None, *a, **k: (1.0 - mask[:, None, None, :].to(torch.float32)) * -10000.0
    return m


def grad_sample(g: torch.Tensor, n: int = 1024) -> np.ndarray:
    f = g.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n].numpy().copy()


def weights(named_shapes, relation_ids):
    """seeded_weights (seed 31) over the reference's names; [R] row and its zero decoder bias appended."""
    v0 = D.VOCAB - 1
    shapes = [(n, ((v0,) + tuple(s[1:]) if n in (WORD, BIAS) else tuple(s))) for n, s in named_shapes]
    sd = D.seeded_weights(shapes, seed=31)
    W = sd[WORD]
    sd[WORD] = torch.cat([W, W[torch.tensor(relation_ids)].mean(0, keepdim=True)], 0)
    sd[BIAS] = torch.cat([sd[BIAS], torch.zeros(1)])
    return sd


_E = "visual_bert.embeddings."
SAMPLE = ["cls.predictions.transform.dense.weight", BIAS, WORD, _E + "position_embeddings.weight", _E + "token_type_embeddings.weight",
          _E + "LayerNorm.weight", _E + "LayerNorm.bias", _E + "visual_token_type_embeddings.weight", _E + "visual_position_embeddings.weight",
          _E + "visual_projection.weight", _E + "visual_projection.bias", "cls.predictions.transform.LayerNorm.weight"]
for _l in (0, 6, 11):
    _p = f"visual_bert.encoder.layer.{_l}."
    SAMPLE += [_p + "attention.self.query.weight", _p + "attention.self.key.bias", _p + "attention.self.value.weight",
               _p + "attention.self.adaptive_weight.0", _p + "attention.self.adaptive_weight.1", _p + "attention.output.dense.weight",
               _p + "attention.output.LayerNorm.weight", _p + "intermediate.dense.weight", _p + "output.dense.bias", _p + "output.LayerNorm.bias"]


def run(m, B, L, batch_seed, feat_seed, odd, out_path):
    t0 = time.time()
    from transformers import VisualBertConfig
    cfgd = D.data_config(seed=1234)
    cfg = VisualBertConfig(vocab_size=D.VOCAB, visual_embedding_dim=FEAT)
    cfg.is_decoder = False
    assert cfg.hidden_size == 768 and cfg.num_hidden_layers == 12 and cfg.hidden_dropout_prob == 0.1 and not cfg.bypass_transformer
    torch.manual_seed(0)
    model = m.VisualBertForMaskedLM(cfg)
    model.cls.predictions.decoder.weight = model.visual_bert.embeddings.word_embeddings.weight    # tie by hand (main.py; no resize under 5.x)
    model.visual_bert.embeddings.word_embeddings.padding_idx = None                                # 4.19.0 resize drops padding_idx
    named = dict(model.named_parameters())
    sd = weights([(n, p.shape) for n, p in named.items()], cfgd["analogy_relation_ids"])
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    named = dict(model.named_parameters())
    assert set(named) == set(sd), set(named) ^ set(sd)
    model.eval()
    batch = D.make_batch(B, L, image_size=2, seed=batch_seed)
    batch.pop("pixel_values")
    vmask = visual_mask(B, odd)
    feats = region_features(B, feat_seed, vmask)
    ids = torch.tensor(cfgd["analogy_entity_ids"])
    ar = torch.arange(B)
    _, mask_idx = (batch["input_ids"] == 103).nonzero(as_tuple=True)

    def fwd():
        sep = batch["sep_idx"].clone()               # the reference shifts it in place (:866)
        return model(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], token_type_ids=batch["token_type_ids"],
                     pixel_values=feats, visual_attention_mask=vmask, sep_idx=sep, return_dict=True)
    out, trans = fwd()
    assert tuple(trans.shape) == (B, L + V, 768)
    mask_logits = out.logits[ar, mask_idx][:, ids]
    rel, qh, ah = batch["rel_idx"] + V, batch["q_head_idx"] + V, batch["a_head_idx"] + V             # lit_models/transformer.py:98-102
    loss = O.label_smooth_ce(mask_logits, batch["label"], 0.1) + ALPHA * O.relaxation_loss(trans, rel, qh, ah)
    loss.backward()
    rows = torch.stack([mask_idx, qh, ah, rel[:, 0], rel[:, 1]], 1)
    none_grad = sorted(n for n, p in named.items() if p.grad is None)
    norms = {n: float(p.grad.double().norm()) for n, p in named.items() if p.grad is not None}
    samples = {"gs::" + n: grad_sample(named[n].grad) for n in SAMPLE if named[n].grad is not None}
    ranks = O.ranks_double_sort(mask_logits.detach(), batch["label"])
    with torch.no_grad():                            # bf16-weight control
        for p in model.parameters():
            p.copy_(p.to(torch.bfloat16).float())
        out_c, _ = fwd()
        ctrl = out_c.logits[ar, mask_idx][:, ids]
    ctrl_dev = float((ctrl - mask_logits.detach()).abs().max())
    np.savez_compressed(
        out_path, B=np.int64(B), L=np.int64(L), V=np.int64(V), weight_seed=np.int64(31), batch_seed=np.int64(batch_seed), feat_seed=np.int64(feat_seed),
        alpha=np.float64(ALPHA), param_names=np.array(list(named)), visual_attention_mask=vmask.numpy(),
        **{"in::" + k: v.numpy() for k, v in batch.items()},
        mask_logits=mask_logits.detach().numpy(), bf16_control_logits=ctrl.numpy(), bf16_control_dev=np.float64(ctrl_dev),
        trans_rows=trans.detach()[ar[:, None], rows].numpy(), trans_row_index=rows.numpy(),
        loss=np.float64(float(loss.detach())), ranks=np.asarray(ranks), none_grad=np.array(none_grad),
        grad_norm_names=np.array(sorted(norms)), grad_norm_vals=np.array([norms[k] for k in sorted(norms)]), **samples)
    print(f"{os.path.basename(out_path)}: loss {float(loss):.6f} ranks {np.asarray(ranks).tolist()} none-grad {none_grad} "
          f"bf16 control {ctrl_dev:.3e} ({time.time() - t0:.1f} s)", flush=True)


def main():
    a = ap.ArgumentParser()
    a.add_argument("--ref", required=True, help="MarT checkout (the directory holding models/modeling_visual_bert.py)")
    a.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a.add_argument("--only", default="")
    a = a.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    m = load_reference_visualbert(a.ref)
    if not a.only or a.only == "g11":
        run(m, 2, 64, 41, 43, False, os.path.join(a.out, "g11_visualbert_real.npz"))
    if not a.only or a.only == "g11b":
        run(m, 3, 37, 47, 53, True, os.path.join(a.out, "g11b_visualbert_odd.npz"))


if __name__ == "__main__":
    main()
