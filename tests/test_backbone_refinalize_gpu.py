"""A second FlatStore behind a model that is already in use (resize_token_embeddings after forward passes), for each backbone: the seed, the
step counter and the precision survive, both engines follow the new store, and the scores of existing ids do not move by a bit.
ViLT / VisualBERT at their *_odd golden configurations (12 layers, L = 37); MKGformer / FLAVA with two layers per stream at H = 768 (head_dim 64
and the fusion kernel's width are what the engines require).  B = 2, eval mode, no gradients."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEXT = ("input_ids", "attention_mask", "token_type_ids", "sep_idx")


def _mkgformer():
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.models import MKGformerKGC, TextConfig, VisionConfig
    batch = D.make_batch(2, 64, seed=17)
    return MKGformerKGC(VisionConfig(patch_size=32, num_hidden_layers=2), TextConfig(vocab_size=D.VOCAB, num_hidden_layers=2)), batch, TEXT + ("pixel_values",)


def _flava():
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.models import FlavaKGC, flava_config
    batch = D.make_batch(2, 64, seed=17)
    return FlavaKGC(flava_config(vocab_size=D.VOCAB, text_layers=2, image_layers=2, mm_layers=2)), batch, TEXT + ("pixel_values",)


def _vilt():
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.models import ViltKGC, vilt_config
    g = np.load(os.path.join(GOLD, "g10b_vilt_odd.npz"))
    batch = D.make_batch(2, int(g["L"]), image_size=384, seed=int(g["batch_seed"]))
    return ViltKGC(vilt_config(vocab_size=D.VOCAB)), batch, TEXT + ("pixel_values",)


def _visualbert():
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.models import VisualBertKGC, visual_bert_config
    from tools.gen_goldens_visualbert import region_features
    g = np.load(os.path.join(GOLD, "g11b_visualbert_odd.npz"))
    batch = D.make_batch(2, int(g["L"]), image_size=2, seed=int(g["batch_seed"]))
    batch["visual_attention_mask"] = torch.from_numpy(g["visual_attention_mask"])[:2]         # example 1: a single entity, 36 regions masked
    batch["pixel_values"] = region_features(2, int(g["feat_seed"]), batch["visual_attention_mask"])
    return VisualBertKGC(visual_bert_config(vocab_size=D.VOCAB)), batch, TEXT + ("pixel_values", "visual_attention_mask")


@pytest.mark.parametrize("build", [_mkgformer, _flava, _vilt, _visualbert], ids=["MKGformerKGC", "FlavaKGC", "ViltKGC", "VisualBertKGC"])
def test_resize_behind_a_model_in_use(build):
    from mkg_analogy_amd import data_synth as D
    model, batch, keys = build()
    # N(0, 0.02) weights (FLAVA's scalar logit_scale, which MarT never evaluates, keeps its default)
    model.load_state_dict(D.seeded_weights([(n, p.shape) for n, p in model.named_parameters() if p.dim()], seed=31), strict=False)
    model.cuda().eval()
    kw = {k: batch[k].cuda() for k in keys}
    ar = torch.arange(2, device="cuda")
    _, mi = (kw["input_ids"] == D.MASK).nonzero(as_tuple=True)
    ids = torch.arange(16, device="cuda") * 2500 + 7                         # 16 ids that exist before and after

    def scores():
        out = {}
        for prec in ("bf16", "fp32"):
            model.set_precision(prec)
            torch.manual_seed(5)                                             # (ViLT draws its patch order from the default generator)
            with torch.no_grad():
                o, _ = model(**kw, return_dict=True)
                out[prec] = o.logits[ar, mi][:, ids].float().cpu()
        model.set_precision("bf16")
        return out

    s0 = scores()
    st0 = model.store
    assert model._step == 1 and model._precise.st is st0
    model.base_seed = 12345
    model.resize_token_embeddings(D.VOCAB + 3)
    s1 = scores()
    assert model.store is not st0
    assert model.base_seed == 12345 and model._step == 2 and model.precision == "bf16"
    assert model.engine.st is model.store and model._precise.st is model.store
    for prec in ("bf16", "fp32"):
        assert bool(torch.isfinite(s0[prec]).all()) and float(s0[prec].abs().max()) > 0.0
        print(f"\n{type(model).__name__} {prec}: max|score after - before| {float((s1[prec] - s0[prec]).abs().max()):.3e}")
        assert torch.equal(s0[prec], s1[prec]), prec
