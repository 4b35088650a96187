"""Reloading weights into a model whose parameters already live in the flat store.

The reference reloads its best checkpoint through the LIT model (main.py:134,159: ``lit_model.load_state_dict(...)``).
``torch.nn.Module.load_state_dict`` on a parent never calls a child's ``load_state_dict``: it calls ``_load_from_state_dict`` on every
submodule.  The parameters are views of the fp32 master buffer, so the masters change; unless the bf16 / fp16 / W^T copies that every
kernel reads are refreshed too, fit -> reload best -> test evaluates the LAST weights, silently.  Held here for the three model classes:
after a training step and a load through the lit model, every shadow is the cast of its master and the evaluation forward (bf16 and
fp32-accurate) is bit-identical to a fresh model that was given the same weights before its store was built."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("input_ids", "attention_mask", "token_type_ids", "pixel_values", "sep_idx")


def _new(kind):
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.lit_models import TransformerLitModel
    from mkg_analogy_amd import models as M
    torch.manual_seed(0)
    if kind == "MKGformerKGC":
        model, alpha, lr = M.MKGformerKGC(M.VisionConfig(patch_size=32), M.TextConfig()), 0.43, 5e-5
    elif kind == "FlavaKGC":
        model, alpha, lr = M.FlavaKGC(M.flava_config(vocab_size=30522)), 0.45, 5e-5
    else:
        model, alpha, lr = M.ViltKGC(M.vilt_config(vocab_size=30522)), 0.3, 4e-5
    cfg = D.data_config(seed=1234)
    args = argparse.Namespace(label_smoothing=0.1, alpha=alpha, pretrain=0, lr=lr, weight_decay=0.01, optimizer="AdamW", warm_up_radio=0.1)
    lit = TransformerLitModel(model=model, args=args, tokenizer=D.FakeTokenizer(), data_config=cfg)      # resize -> 42006
    lit._init_relation_word()                                                                            # -> 42007 (on the host: no store yet)
    assert model._store is None
    return model, lit, cfg


def _weights(model, seed):
    """A seeded weight set over the model's own names: N(0, 0.02), normalisation scales 1 + 0.05 N(0, 1), adaptive weights (0.25, 0.5)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, p in model.named_parameters():
        x = torch.randn(tuple(p.shape), generator=g)
        if n.endswith("adaptive_weight.0") or n.endswith("adaptive_weight.1"):
            out[n] = torch.full(tuple(p.shape), 0.25 if n.endswith("0") else 0.5)
        elif "norm" in n.lower() and n.endswith(".weight"):
            out[n] = 1.0 + 0.05 * x
        else:
            out[n] = 0.02 * x
    return out


def _fresh(kind, sd):
    """A model that is given ``sd`` BEFORE its store exists: finalize() then builds masters and shadows from it."""
    model, lit, cfg = _new(kind)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert model._store is None and not unexpected and all(("position_ids" in m or "decoder" in m) for m in missing), (missing, unexpected)
    model.cuda()
    return model, lit, cfg


def _shadow_faults(st):
    bad = []
    if not torch.equal(st.shadow, st.master.to(torch.bfloat16)):
        bad += ["bf16:" + n for n in st.slots if not torch.equal(st.w(n), st.m(n).to(torch.bfloat16))] or ["bf16:<padding>"]
    for n in st.slots:
        if st.f16_weight is not None and st.f16_weight(n) and not torch.equal(st.h(n), st.m(n).to(torch.float16)):
            bad.append("fp16:" + n)
    st.join_pending()
    for (key, (toff, rows, cols)), (first, toff2, _, _) in zip(st.tslots.items(), st.ttable.cpu().tolist()):
        assert toff == toff2
        if not torch.equal(st.shadow_t[toff:toff + rows * cols].view(cols, rows), st.shadow[first:first + rows * cols].view(rows, cols).t()):
            bad.append("wt:" + key)
    return bad


def _eval(model, gb, ids):
    """Mask-row logits over the analogy entities and the full trans_hidden, bf16 path and fp32-accurate path."""
    model.eval()
    out = {}
    B = gb["input_ids"].shape[0]
    _, mi = (gb["input_ids"] == 103).nonzero(as_tuple=True)
    for prec in ("bf16", "fp32"):
        model.set_precision(prec)
        torch.manual_seed(5)
        with torch.no_grad():
            o, trans = model(**{k: gb[k] for k in KEYS}, return_dict=True)
            out[prec] = (o.logits[torch.arange(B, device="cuda"), mi][:, ids].float().clone(), trans.float().clone())
    model.set_precision("bf16")
    return out


@pytest.mark.parametrize("kind", ["MKGformerKGC", "FlavaKGC", "ViltKGC"])
def test_load_through_the_lit_model_refreshes_every_shadow(kind, tmp_path):
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.trainer import Trainer
    model, lit, cfg = _new(kind)
    sd_a, sd_b = _weights(model, 41), _weights(model, 42)
    model.load_state_dict(sd_a, strict=False)
    model.cuda()
    b = D.make_batch(2, 64, image_size=384 if kind == "ViltKGC" else 224, seed=17)
    gb = {k: v.cuda() for k, v in b.items()}
    ids = torch.tensor(cfg["analogy_entity_ids"], device="cuda")
    tr = Trainer(max_epochs=1, max_steps=4)
    tr._setup(lit, [gb] * 4)
    for i in range(2):                                                   # lr(0) = 0: the second step moves the weights
        tr.train_step(lit, gb, i)
    st = model.store
    assert _shadow_faults(st) == []
    moved = _eval(model, gb, ids)

    # (1) a different weight set through the LIT model, as main.py reloads its best checkpoint
    r = lit.load_state_dict({"model." + k: v for k, v in sd_b.items()}, strict=False)
    assert not r.unexpected_keys
    assert model.store is st, "the store survives a load"
    name = next(n for n in st.slots if n.endswith("query.weight") or n.endswith("q_proj.weight"))
    assert torch.equal(st.m(name).cpu(), sd_b[name]), "the masters are views of the parameters: they follow any load"
    assert _shadow_faults(st) == []
    got = _eval(model, gb, ids)
    fresh_model, fresh_lit, _ = _fresh(kind, sd_b)
    want = _eval(fresh_model, gb, ids)
    for prec in ("bf16", "fp32"):
        assert not torch.equal(got[prec][0], moved[prec][0])
        assert torch.equal(got[prec][0], want[prec][0]) and torch.equal(got[prec][1], want[prec][1]), prec

    # (2) back to the first set, then a checkpoint FILE written from the fresh product's lit.state_dict()
    path = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": fresh_lit.state_dict()}, path)
    del fresh_model, fresh_lit
    lit.load_state_dict({"model." + k: v for k, v in sd_a.items()}, strict=False)
    back = _eval(model, gb, ids)
    assert _shadow_faults(st) == [] and not torch.equal(back["bf16"][0], want["bf16"][0])
    lit.load_state_dict(torch.load(path)["state_dict"])
    assert _shadow_faults(st) == []
    got = _eval(model, gb, ids)
    for prec in ("bf16", "fp32"):
        assert torch.equal(got[prec][0], want[prec][0]) and torch.equal(got[prec][1], want[prec][1]), prec

    # (3) the model's own load_state_dict keeps doing the same
    model.load_state_dict(sd_a, strict=False)
    assert _shadow_faults(st) == []
    again = _eval(model, gb, ids)
    assert torch.equal(again["bf16"][0], back["bf16"][0]) and torch.equal(again["fp32"][0], back["fp32"][0])


def _hf_names(n_layers=12):
    """State-dict names of transformers' CLIPVisionModel.vision_model and BertModel (the checkpoints main.py:87-88 reads), with the shape of the
    MKGformer tensor each one lands in (looked up in the oracle's name table)."""
    clip = {"embeddings.class_embedding": "unimo.vision_embeddings.class_embedding", "embeddings.position_ids": None,
            "embeddings.patch_embedding.weight": "unimo.vision_embeddings.patch_embedding.weight",
            "embeddings.position_embedding.weight": "unimo.vision_embeddings.position_embedding.weight"}
    for p, q in (("pre_layrnorm", "unimo.vision_pre_layrnorm"), ("post_layernorm", "unimo.vision_post_layernorm")):
        clip.update({f"{p}.{w}": f"{q}.{w}" for w in ("weight", "bias")})
    bert = {"embeddings.position_ids": None}
    for e in ("word_embeddings", "position_embeddings", "token_type_embeddings"):
        bert[f"embeddings.{e}.weight"] = f"unimo.text_embeddings.{e}.weight"
    for w in ("weight", "bias"):
        bert[f"embeddings.LayerNorm.{w}"] = f"unimo.text_embeddings.LayerNorm.{w}"
        bert[f"pooler.dense.{w}"] = f"unimo.text_pooler.dense.{w}"
    for l in range(n_layers):
        for m in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "layer_norm1", "mlp.fc1", "mlp.fc2", "layer_norm2"):
            clip.update({f"encoder.layers.{l}.{m}.{w}": f"unimo.encoder.vision_layers.{l}.{m}.{w}" for w in ("weight", "bias")})
        for m in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense", "attention.output.LayerNorm",
                  "intermediate.dense", "output.dense", "output.LayerNorm"):
            bert.update({f"encoder.layer.{l}.{m}.{w}": f"unimo.encoder.text_layer.{l}.{m}.{w}" for w in ("weight", "bias")})
    return clip, bert


def test_pretrained_rename_loop_consumes_every_key_and_refreshes_the_shadows():
    """main.py:90-109 restated: every name of the CLIP vision / BERT checkpoints is found under a renamed MKGformer key, the merged dict loads
    strictly -- into a model whose store already exists -- and the kernels' operand copies follow."""
    from mkg_analogy_amd.models import MKGformerKGC, TextConfig, VisionConfig
    from oracle import mkgformer_oracle as O
    torch.manual_seed(0)
    model = MKGformerKGC(VisionConfig(patch_size=32), TextConfig())
    model.cuda()
    st = model.finalize()
    table = O.init_params(O.VisionCfg(patch_size=32), O.TextCfg(vocab_size=30522), seed=3)
    g = torch.Generator().manual_seed(9)
    clip_names, bert_names = _hf_names()
    fake = lambda names, n_pos: {k: (torch.randn(table[v].shape, generator=g) * 0.02 if v is not None else torch.arange(n_pos).expand((1, -1)))
                                 for k, v in names.items()}
    sources = {"vision": fake(clip_names, 50), "text": fake(bert_names, 512)}

    # the rule of main.py:90-109: a model tensor whose name mentions a tower takes the checkpoint tensor found under its name without the tower
    # prefix ("vision_" / "text_"), "model." and "unimo."; every checkpoint tensor must have been taken; the merged dict loads strictly
    merged, used = model.state_dict(), {"vision": set(), "text": set()}
    for name in list(merged):
        side = "vision" if "vision" in name else "text" if "text" in name else None
        if side is None:
            continue
        key = name
        for cut in (side + "_", "model.", "unimo."):
            key = key.replace(cut, "")
        if key in sources[side]:
            merged[name] = sources[side][key]
            used[side].add(key)
    assert used["vision"] == set(sources["vision"]) and used["text"] == set(sources["text"]), \
        (sorted(set(sources["vision"]) - used["vision"])[:5], sorted(set(sources["text"]) - used["text"])[:5])
    model.load_state_dict(merged)
    assert model.store is st and _shadow_faults(st) == []
    for hf, mine in list(clip_names.items()) + list(bert_names.items()):
        if mine is not None:
            src = sources["vision" if "vision" in mine else "text"][hf]
            assert torch.equal(st.m(mine).cpu(), src), mine
