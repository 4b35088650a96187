"""VisualBERT backbone (VisualBertKGC), host side: parameter names, the region-feature collate against a restatement of the reference's
(MarT/data/data_module.py:121-173), argument refusals, the lit model's + V row shift, and the caller's sep_idx left alone.
Goldens: tests/golden/g11_visualbert_real.npz / g11b_visualbert_odd.npz (tools/gen_goldens_visualbert.py, the unmodified reference)."""
import argparse
import os
import pickle

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = os.path.join(GOLD, "mars")


def _g(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def test_parameter_names_match_reference():
    from mkg_analogy_amd.models import VisualBertKGC, visual_bert_config
    from mkg_analogy_amd.visual_bert_engine import vbert_f16_weight, vbert_gemm_groups, vbert_layout_order
    g = _g("g11_visualbert_real.npz")
    model = VisualBertKGC(visual_bert_config(vocab_size=42007))
    names = [n for n, _ in model.named_parameters()]
    assert names == [str(x) for x in g["param_names"]] == [str(x) for x in _g("g11b_visualbert_odd.npz")["param_names"]]
    assert len(names) == 230                              # the untied reference has 231: cls.predictions.decoder.weight is the word embedding here
    assert model.get_output_embeddings().weight is model.get_input_embeddings().weight
    sd = set(model.state_dict())
    assert sd - set(names) == {"visual_bert.embeddings.position_ids", "cls.predictions.decoder.weight", "cls.predictions.decoder.bias"}
    order = vbert_layout_order(12)
    assert sorted(order) == sorted(names) and order[-1] == "visual_bert.embeddings.word_embeddings.weight"
    for _, members in vbert_gemm_groups(12):             # members of a fused GEMM weight are adjacent in the layout
        i = order.index(members[0])
        assert tuple(order[i:i + len(members)]) == members
    f16 = [n for n in names if vbert_f16_weight(n)]
    assert len(f16) == 1 + 12 * 6 and all(model.get_parameter(n).dim() == 2 for n in f16)
    model.resize_token_embeddings(42010)
    assert model.get_output_embeddings().weight.shape[0] == 42010 and model.cls.predictions.bias.shape[0] == 42010
    assert model.get_output_embeddings().weight is model.get_input_embeddings().weight


def test_refusals():
    from mkg_analogy_amd.models import VisualBertKGC, visual_bert_config
    model = VisualBertKGC(visual_bert_config(vocab_size=64, num_hidden_layers=1, hidden_size=64, num_attention_heads=1, intermediate_size=128))
    ids = torch.zeros((1, 8), dtype=torch.int64)
    feats = torch.zeros(1, 72, 2048)
    with pytest.raises(TypeError, match="NoneType"):
        model(input_ids=ids, pixel_values=feats, sep_idx=None)
    kw = dict(input_ids=ids, pixel_values=feats, sep_idx=torch.zeros((1, 6), dtype=torch.int64))
    for bad in (dict(position_ids=ids), dict(inputs_embeds=torch.zeros(1, 8, 64)), dict(head_mask=torch.ones(1)), dict(output_attentions=True),
                dict(visual_token_type_ids=torch.ones(1, 72, dtype=torch.int64))):
        with pytest.raises(NotImplementedError):
            model(**kw, **bad)
    with pytest.raises(ValueError, match="pixel_values"):
        model(input_ids=ids, sep_idx=kw["sep_idx"])
    model.set_precision("fp32")                              # fp32 is the evaluation path: training / gradients in fp32 are refused
    with pytest.raises(NotImplementedError, match="verification mode"):
        model(**kw)
    model.eval()
    with pytest.raises(NotImplementedError, match="verification mode"):
        model(**kw)                                          # grad enabled
    with pytest.raises(ValueError):
        model.set_precision("fp16")
    with pytest.raises(NotImplementedError):
        model.set_image_table(torch.zeros(1, 3, 224, 224))
    with pytest.raises(NotImplementedError):
        c = visual_bert_config(vocab_size=64)
        c.bypass_transformer = True
        VisualBertKGC(c)
    p = argparse.ArgumentParser()
    VisualBertKGC.add_to_argparse(p)
    assert p.parse_args([]).pretrain == 0


def test_mask_and_sep_leave_the_callers_tensors():
    """The reference adds img_length to sep_idx in place (modeling_visual_bert.py:866); both VisualBERT engines build the joint mask and the
    shifted split through vbert_mask_and_sep, which returns new tensors.  The joint mask is not a prefix."""
    from mkg_analogy_amd.visual_bert_engine import vbert_mask_and_sep
    sep = torch.tensor([[0, 5, 12, 20, 22, 25], [0, 3, 9, 15, 16, 18]])
    am = torch.tensor([[1] * 26 + [0] * 4, [1] * 19 + [0] * 11])
    vm = torch.ones(2, 72)
    vm[1, 36:] = 0.0
    sep0, am0, vm0 = sep.clone(), am.clone(), vm.clone()
    mask, s = vbert_mask_and_sep(am, vm, sep, 72)
    assert torch.equal(sep, sep0) and torch.equal(am, am0) and torch.equal(vm, vm0)
    assert s.tolist() == [84, 81] and s.data_ptr() != sep.data_ptr()
    assert mask.dtype == torch.int64 and mask.shape == (2, 102) and torch.equal(mask[:, :30], am) and torch.equal(mask[:, 30:], vm.long())
    assert mask[1].tolist() == [1] * 19 + [0] * 11 + [1] * 36 + [0] * 36
    mask2, _ = vbert_mask_and_sep(am, None, sep, 72)         # no visual mask: all regions attended (:831-832)
    assert bool((mask2[:, 30:] == 1).all())


class _StubModel(torch.nn.Module):
    """What the lit model needs of a backbone, on the CPU: outputs of the right shapes, no compute."""

    @property
    def store(self):
        from types import SimpleNamespace
        return SimpleNamespace(device=torch.device("cpu"))

    def resize_token_embeddings(self, n):
        pass

    def forward(self, **kw):
        from types import SimpleNamespace

        class _Rows:
            def __getitem__(self, k):
                return torch.zeros(2, 2063)

        class _Logits:
            trans = torch.zeros(2, 136, 8)

            def mask_rows(self, ids, tok):
                return _Rows()
        return SimpleNamespace(logits=_Logits()), _Logits.trans


class _ZeroLoss(torch.nn.Module):
    def forward(self, logits, label):
        return torch.zeros(())


@pytest.mark.parametrize("cls_name,shift", [("VisualBertKGC", 72), ("ViltKGC", 0), ("MKGformerKGC", 0)])
def test_lit_model_shifts_rows_for_visualbert_only(cls_name, shift, monkeypatch):
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd import functional as Fn
    from mkg_analogy_amd.lit_models import TransformerLitModel
    args = argparse.Namespace(label_smoothing=0.1, alpha=0.43, pretrain=0, lr=4e-5, weight_decay=0.01, optimizer="AdamW", warm_up_radio=0.1)
    model = type(cls_name, (_StubModel,), {})()                 # the lit model tells the backbones apart by class name, as the reference does
    lit = TransformerLitModel(model=model, args=args, tokenizer=D.FakeTokenizer(), data_config=D.data_config(seed=1234))
    batch = D.make_batch(2, 64, image_size=2, seed=3)
    batch["pixel_values"] = torch.zeros(2, 72, 2048)
    rel0, q0, a0 = batch["rel_idx"].clone(), batch["q_head_idx"].clone(), batch["a_head_idx"].clone()
    seen = {}
    monkeypatch.setattr(Fn, "relaxation_loss", lambda t, rel, q, a: seen.update(rel=rel.clone(), q=q.clone(), a=a.clone()) or torch.zeros(()))
    lit.loss_fn = _ZeroLoss()
    monkeypatch.setattr(lit, "_needed", lambda ids, extra: seen.update(extra=extra) or {})
    b = dict(batch)
    lit.training_step(b, 1)
    assert torch.equal(seen["rel"], rel0 + shift) and torch.equal(seen["q"], q0 + shift) and torch.equal(seen["a"], a0 + shift)
    # the row-subset hint sees the same (shifted) rows as the loss
    assert torch.equal(seen["extra"][0], rel0 + shift) and torch.equal(seen["extra"][1], q0 + shift) and torch.equal(seen["extra"][2], a0 + shift)
    assert torch.equal(batch["rel_idx"], rel0) and torch.equal(batch["q_head_idx"], q0) and torch.equal(batch["a_head_idx"], a0)   # caller's tensors untouched
    if shift:
        lit.args.pretrain = 1
        with pytest.raises(NotImplementedError, match="pre-train"):
            lit.training_step(dict(batch, pre_type=torch.ones(2, dtype=torch.int64)), 1)


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    import shutil
    tmp = tmp_path_factory.mktemp("mars_vbert")
    data_dir, pre = tmp / "MARS", tmp / "MarKG"
    data_dir.mkdir(); pre.mkdir()
    for fn in ("dev.json", "train.json", "test.json", "analogy_entities.txt", "analogy_relations.txt"):
        shutil.copy(os.path.join(FIX, fn), data_dir)
    for fn in ("entity2text.txt", "relation2text.txt", "wiki_tuple_ids.txt"):
        shutil.copy(os.path.join(FIX, fn), pre)
    return str(data_dir), str(pre)


def _args(dirs, model_class="VisualBertKGC"):
    return argparse.Namespace(model_name_or_path="bert-base-uncased", data_dir=dirs[0], pretrain_path=dirs[1], pretrain=0,
                              max_seq_length=128, overwrite_cache=True, precision=32, model_class=model_class,
                              batch_size=4, eval_batch_size=4, num_workers=0)


def _reference_collate(table, head_ent, tail_ent):
    """Restatement of MarT/data/data_module.py:121-159, dict branch."""
    pixel_images, masks = [], []
    for head, tail in zip(head_ent, tail_ent):
        pi, vm = [], []
        if head and tail:
            pi += [torch.from_numpy(table[head]).squeeze(), torch.from_numpy(table[tail]).squeeze()]
            vm += [torch.ones(36, dtype=torch.float), torch.ones(36, dtype=torch.float)]
        else:
            entity = head if head is not None else tail
            if entity:
                pi.append(torch.from_numpy(table[entity]).squeeze())
                vm.append(torch.ones(36, dtype=torch.float))
            else:
                pi.append(torch.zeros((36, 2048)))
                vm.append(torch.zeros(36, dtype=torch.float))
            pi.append(torch.zeros((36, 2048)))
            vm.append(torch.zeros(36, dtype=torch.float))
        pixel_images.append(torch.cat(pi))
        masks.append(torch.cat(vm))
    return torch.stack(pixel_images), torch.stack(masks)


def test_data_module_region_batches_and_refusals(dirs, tmp_path):
    from mkg_analogy_amd.data import BertWordPieceTokenizer
    from mkg_analogy_amd.data.data_module import KGC
    g6 = np.load(os.path.join(GOLD, "g6_mars_plumbing.npz"))
    tok = lambda: BertWordPieceTokenizer(g6["vocab"].tolist())
    with pytest.raises(NotImplementedError, match="visual_features="):
        KGC(_args(dirs), None, tokenizer=tok())
    with pytest.raises(NotImplementedError):
        KGC(_args(dirs, "VilBertKGC"), None, tokenizer=tok())
    with pytest.raises(NotImplementedError):                 # ViLBERT stays refused with features too
        KGC(_args(dirs, "VilBertKGC"), None, tokenizer=tok(), visual_features={})
    with pytest.raises(TypeError):
        KGC(_args(dirs), None, tokenizer=tok(), visual_features=torch.zeros(1, 3, 8, 8))
    ents = [l.split("\t")[0] for l in open(os.path.join(FIX, "entity2text.txt"))]
    rng = np.random.default_rng(5)
    table = {e: rng.random((1, 36, 2048) if i % 2 else (36, 2048), dtype=np.float32) for i, e in enumerate(ents)}   # both stored shapes
    dm = KGC(_args(dirs), None, tokenizer=tok(), visual_features=table)
    dm.setup()
    feats = [dict(dm.data_val[i]) for i in range(4)]
    assert all("head_ent" in f and "tail_ent" in f for f in feats)
    feats[0]["head_ent"], feats[0]["tail_ent"] = ents[0], ents[1]      # head + tail
    feats[1]["head_ent"], feats[1]["tail_ent"] = ents[2], None         # single-entity examples: head only, tail only; and no entity at all
    feats[2]["head_ent"], feats[2]["tail_ent"] = None, ents[3]
    feats[3]["head_ent"] = feats[3]["tail_ent"] = None
    b = dm.sampler(feats)
    pv, vm = b["pixel_values"], b["visual_attention_mask"]
    assert tuple(pv.shape) == (4, 72, 2048) and pv.dtype == torch.float32 and tuple(vm.shape) == (4, 72) and vm.dtype == torch.float32
    ref_pv, ref_vm = _reference_collate(table, [f["head_ent"] for f in feats], [f["tail_ent"] for f in feats])
    assert torch.equal(pv, ref_pv) and torch.equal(vm, ref_vm)
    assert vm.sum(1).tolist() == [72.0, 36.0, 36.0, 0.0]
    assert bool((pv[1, 36:] == 0).all()) and bool((pv[2, 36:] == 0).all()) and bool((pv[3] == 0).all())
    assert torch.equal(pv[2, :36], torch.from_numpy(table[feats[2]["tail_ent"]]).reshape(36, 2048))
    assert "image_index" not in b and "sep_idx" in b and b["input_ids"].shape[0] == 4
    with pytest.raises(NotImplementedError):
        dm.attach(None)
    path = tmp_path / "analogy_entity2vec.pickle"
    small = {e: table[e] for e in ents[:3]}
    with open(path, "wb") as f:
        pickle.dump(small, f)
    back = KGC.load_region_features(str(path))
    assert set(back) == set(small) and all(np.array_equal(back[e], small[e]) for e in small)
