"""The host-side surface every backbone class shares (models/_backbone.py: HipMaskedLM), on tiny configurations with no GPU: weight tying,
embedding resize, precision / seed state from construction on, and the parameter names in construction order.
Golden: tests/golden/backbone_surface_names.json -- names only, recorded from the four classes before they shared a base class."""
import json
import os

import pytest
import torch
from torch import nn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_surface_names.json")
V, H = 100, 64                                      # vocabulary and width of the tiny configurations


def _mkgformer():
    from mkg_analogy_amd.models import MKGformerKGC, TextConfig, VisionConfig
    small = dict(hidden_size=H, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128)
    return MKGformerKGC(VisionConfig(patch_size=32, **small), TextConfig(vocab_size=V, max_position_embeddings=32, **small))


def _flava():
    from mkg_analogy_amd.models import FlavaKGC, flava_config
    return FlavaKGC(flava_config(vocab_size=V, hidden_size=H, text_layers=2, image_layers=2, mm_layers=1, num_attention_heads=1,
                                 intermediate_size=128, max_position_embeddings=32))


def _vilt():
    from mkg_analogy_amd.models import ViltKGC, vilt_config
    return ViltKGC(vilt_config(vocab_size=V, hidden_size=H, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128))


def _visualbert():
    from mkg_analogy_amd.models import VisualBertKGC, visual_bert_config
    return VisualBertKGC(visual_bert_config(vocab_size=V, hidden_size=H, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128,
                                            max_position_embeddings=32, visual_embedding_dim=32))


# class name -> (constructor, the object that holds .decoder and .bias, initializer_range, takes a device image table)
CASES = {"MKGformerKGC": (_mkgformer, lambda m: m.cls.predictions, 0.02, True),
         "FlavaKGC": (_flava, lambda m: m.cls, 0.02, False),
         "ViltKGC": (_vilt, lambda m: m.mlm_score, 0.02, True),
         "VisualBertKGC": (_visualbert, lambda m: m.cls.predictions, 0.02, False)}


@pytest.fixture(params=list(CASES))
def case(request):
    build, head, std, table = CASES[request.param]
    torch.manual_seed(11)
    return request.param, build(), head, std, table


def _assert_tied(m, head, n):
    emb, dec = m.get_input_embeddings(), m.get_output_embeddings()
    assert dec is head(m).decoder
    assert dec.weight is emb.weight and tuple(emb.weight.shape) == (n, H)
    assert dec.bias is head(m).bias and tuple(head(m).bias.shape) == (n,)
    assert dec.out_features == n


def test_names_equal_the_recorded_lists(case):
    name, m, _, _, _ = case
    with open(GOLD) as f:
        gold = json.load(f)[name]
    assert [n for n, _ in m.named_parameters()] == gold["named_parameters"]
    assert list(m.state_dict()) == gold["state_dict"]


def test_tied_weight_and_resize(case):
    _, m, head, std, _ = case
    _assert_tied(m, head, V)
    emb0 = m.get_input_embeddings()
    for same in (None, V):                          # no-ops: the very same nn.Embedding stays in place
        m.resize_token_embeddings(same)
        assert m.get_input_embeddings() is emb0
    _assert_tied(m, head, V)
    with torch.no_grad():
        head(m).bias.copy_(torch.arange(V, dtype=torch.float32) + 1.0)
    old, b_old = emb0.weight.detach().clone(), head(m).bias.detach().clone()

    m.resize_token_embeddings(V + 7)
    _assert_tied(m, head, V + 7)
    w, b = m.get_input_embeddings().weight.detach(), head(m).bias.detach()
    assert torch.equal(w[:V], old)
    assert torch.equal(b[:V], b_old) and float(b[V:].abs().max()) == 0.0
    # 7 x 64 = 448 draws of N(0, std): the sample standard deviation has standard error std / sqrt(2 n), the mean std / sqrt(n); five of each
    new, n = w[V:], 7 * H
    assert abs(float(new.std()) - std) < 5 * std / (2 * n) ** 0.5 and abs(float(new.mean())) < 5 * std / n ** 0.5

    m.resize_token_embeddings(V - 3)
    _assert_tied(m, head, V - 3)
    assert torch.equal(m.get_input_embeddings().weight, old[:V - 3]) and torch.equal(head(m).bias, b_old[:V - 3])


def test_set_output_embeddings_leaves_the_model_tied(case):
    _, m, head, _, _ = case
    new = nn.Linear(H, V)
    m.set_output_embeddings(new)                    # not at the parent commit: assign-only for MKGformer, absent for FLAVA
    assert m.get_output_embeddings() is new
    _assert_tied(m, head, V)


def test_state_exists_from_construction_on(case):
    _, m, _, _, _ = case
    # not at the parent commit for FLAVA / ViLT / VisualBERT: finalize() used to create these
    assert m.base_seed == 0x5EED and m._step == 0 and m.precision == "bf16"
    assert m._precise is None and m._precise_train is None and m.image_table is None
    assert m.set_precision("fp32") is m and m.precision == "fp32"
    assert m.set_precision("bf16") is m and m.precision == "bf16"
    with pytest.raises(ValueError):
        m.set_precision("fp16")
    assert m.precision == "bf16"


def test_image_table_is_refused_where_the_backbone_takes_none(case):
    _, m, _, _, table = case
    if table:
        return                                      # (attaching one needs the device: tests/test_model_gpu.py, tests/test_vilt_gpu.py)
    with pytest.raises(NotImplementedError, match="image table"):      # not at the parent commit for FLAVA: it had no such method
        m.set_image_table(torch.zeros(1, 3, 8, 8))
    assert m.image_table is None


def test_shared_methods_are_the_base_class_functions(case):
    from mkg_analogy_amd.models._backbone import HipMaskedLM          # not at the parent commit: the base class is what this adds
    _, m, _, _, _ = case
    assert isinstance(m, HipMaskedLM)
    for meth in ("tie_weights", "resize_token_embeddings", "finalize", "set_precision", "sync_shadows", "set_output_embeddings",
                 "set_image_table", "add_to_argparse"):
        assert getattr(type(m), meth) is getattr(HipMaskedLM, meth), meth
    for prop in ("store", "engine"):
        assert getattr(type(m), prop) is getattr(HipMaskedLM, prop), prop
