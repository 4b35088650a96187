"""ViLT backbone (ViltKGC), host side: parameter names, the reference's patch-order draws, argument refusals, the data module's ViLT
batches.  Goldens: tests/golden/g10_vilt_real.npz / g10b_vilt_odd.npz (tools/gen_goldens_vilt.py, the unmodified reference)."""
import argparse
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def test_parameter_names_match_reference():
    from mkg_analogy_amd.models import ViltKGC, vilt_config
    g = _g("g10_vilt_real.npz")
    model = ViltKGC(vilt_config(vocab_size=42007))
    names = [n for n, _ in model.named_parameters()]
    assert names == [str(x) for x in g["param_names"]]
    assert len(names) == 235                              # the untied reference has 236: mlm_score.decoder.weight is the word embedding here
    assert model.get_output_embeddings().weight is model.get_input_embeddings().weight


@pytest.mark.parametrize("gold", ["g10_vilt_real.npz", "g10b_vilt_odd.npz"])
def test_patch_order_matches_reference_draws(gold):
    from mkg_analogy_amd.models import draw_patch_order
    g = _g(gold)
    torch.manual_seed(int(g["fwd_seed"]))
    order = draw_patch_order(int(g["B"]), 144)
    assert order.shape == (2, int(g["B"]), 144)
    assert np.array_equal(order.numpy(), g["patch_order"])


def test_refusals():
    from mkg_analogy_amd.models import ViltKGC, vilt_config
    model = ViltKGC(vilt_config(vocab_size=64, num_hidden_layers=1, hidden_size=64, num_attention_heads=1, intermediate_size=128))
    ids = torch.zeros((1, 8), dtype=torch.int64)
    with pytest.raises(TypeError, match="NoneType"):
        model(input_ids=ids, pixel_values=torch.zeros(1, 2, 3, 384, 384), sep_idx=None)
    kw = dict(input_ids=ids, pixel_values=torch.zeros(1, 2, 3, 384, 384), sep_idx=torch.zeros((1, 6), dtype=torch.int64))
    for bad in (dict(pixel_mask=torch.ones(1, 384, 384)), dict(image_embeds=torch.zeros(1, 290, 64)), dict(head_mask=torch.ones(1)),
                dict(output_attentions=True)):
        with pytest.raises(NotImplementedError):
            model(**kw, **bad)
    model.set_precision("fp32")                              # fp32 is the evaluation path: training / gradients in fp32 are refused
    with pytest.raises(NotImplementedError, match="verification mode"):
        model(**kw)
    model.eval()
    with pytest.raises(NotImplementedError, match="verification mode"):
        model(**kw)                                          # grad enabled
    with pytest.raises(ValueError):
        model.set_precision("fp16")
    with pytest.raises(NotImplementedError):
        c = vilt_config(vocab_size=64)
        c.hidden_dropout_prob = 0.1
        ViltKGC(c)


def test_mask_and_sep_leave_the_callers_sep_idx():
    """The reference adds img_length to sep_idx in place (modeling_vilt.py:844); both ViLT engines build the joint mask and the shifted split
    through vilt_mask_and_sep, which returns new tensors."""
    from mkg_analogy_amd.vilt_engine import vilt_mask_and_sep
    sep = torch.tensor([[0, 5, 12, 20, 22, 25], [0, 3, 9, 15, 16, 18]])
    am = torch.tensor([[1] * 26 + [0] * 4, [1] * 19 + [0] * 11])
    sep0, am0 = sep.clone(), am.clone()
    mask, s = vilt_mask_and_sep(am, sep, 290)
    assert torch.equal(sep, sep0) and torch.equal(am, am0)
    assert s.tolist() == [302, 299] and s.data_ptr() != sep.data_ptr()
    assert mask.shape == (2, 320) and torch.equal(mask[:, :30], am) and bool((mask[:, 30:] == 1).all())


def test_argparse_and_exports():
    from mkg_analogy_amd.models import ViltKGC
    p = argparse.ArgumentParser()
    ViltKGC.add_to_argparse(p)
    assert p.parse_args([]).pretrain == 0


FIX = os.path.join(GOLD, "mars")


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    import shutil
    tmp = tmp_path_factory.mktemp("mars_vilt")
    data_dir, pre = tmp / "MARS", tmp / "MarKG"
    data_dir.mkdir(); pre.mkdir()
    for fn in ("dev.json", "train.json", "test.json", "analogy_entities.txt", "analogy_relations.txt"):
        shutil.copy(os.path.join(FIX, fn), data_dir)
    for fn in ("entity2text.txt", "relation2text.txt", "wiki_tuple_ids.txt"):
        shutil.copy(os.path.join(FIX, fn), pre)
    return str(data_dir), str(pre)


def _args(dirs, model_class="ViltKGC"):
    return argparse.Namespace(model_name_or_path="bert-base-uncased", data_dir=dirs[0], pretrain_path=dirs[1], pretrain=0,
                              max_seq_length=128, overwrite_cache=True, precision=32, model_class=model_class,
                              batch_size=4, eval_batch_size=4, num_workers=0)


def test_data_module_builds_vilt_batches(dirs):
    """KGC(model_class="ViltKGC") is no longer refused: it looks for the 384-pixel table, or takes an injected one, and emits 384-pixel
    batches on the host and as device-table indices; VisualBERT / ViLBERT stay refused."""
    from mkg_analogy_amd.data import BertWordPieceTokenizer
    from mkg_analogy_amd.data.data_module import KGC
    g6 = np.load(os.path.join(GOLD, "g6_mars_plumbing.npz"))
    tok = BertWordPieceTokenizer(g6["vocab"].tolist())
    with pytest.raises(FileNotFoundError, match="entity_image_features_vilt.pth"):
        KGC(_args(dirs), None, tokenizer=BertWordPieceTokenizer(g6["vocab"].tolist()))
    for mc in ("VisualBertKGC", "VilBertKGC"):
        with pytest.raises(NotImplementedError):
            KGC(_args(dirs, mc), None, tokenizer=BertWordPieceTokenizer(g6["vocab"].tolist()))
    n = sum(1 for _ in open(os.path.join(FIX, "entity2text.txt")))
    base = torch.randn(1, 3, 384, 384, generator=torch.Generator().manual_seed(3))
    table = base.expand(n, 3, 384, 384)                   # a tiny fake table: every entity has the same image (no 20 GB tensor)
    dm = KGC(_args(dirs), None, tokenizer=tok, visual_features=table)
    dm.setup()
    rows = list(range(4))
    dm.use_host_pixels(True)
    b = dm.sampler([dm.data_val[i] for i in rows])
    assert tuple(b["pixel_values"].shape) == (4, 2, 3, 384, 384)
    assert "sep_idx" in b and b["input_ids"].shape[0] == 4
    dm.use_host_pixels(False)
    b2 = dm.sampler([dm.data_val[i] for i in rows])
    assert "pixel_values" not in b2 and b2["image_index"].dtype == torch.int32 and tuple(b2["image_index"].shape) == (4, 2)
    rebuilt = torch.stack([torch.stack([table[i] if i >= 0 else torch.zeros(3, 384, 384) for i in r]) for r in b2["image_index"].tolist()])
    assert torch.equal(rebuilt, b["pixel_values"])
