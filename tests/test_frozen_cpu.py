"""Frozen parameters, host side (no GPU): the backward plan of the MKGformer bf16 engine against the regime table of DESIGN.md ("Frozen parameters"),
the AdamW chunk table of a frozen store, the two freezing hooks of the lit model, and the refusal of a flag that moves after the set was read."""
import types

import pytest
import torch

from mkg_analogy_amd.freeze import BIAS, WORD, backward_plan, launch_groups
from mkg_analogy_amd.params import DEAD, NO_DECAY, ZERO_ONLY, Slot, chunk_table, layout_order, text_f16_weight

N, EXPORT, FUSE = 12, 7, 8
ALL = [n for n in layout_order(N) if not n.startswith(DEAD)]
VISION = ("unimo.vision_", "unimo.encoder.vision_layers.")


def plan(trainable):
    return backward_plan(trainable, N, EXPORT, FUSE)


def regime(name):
    if name == "U":
        return list(ALL)
    if name == "F1":                                   # _freeze_attention(): only names containing "word"
        return [n for n in ALL if "word" in n]
    if name == "F2":                                   # vision tower frozen
        return [n for n in ALL if not n.startswith(VISION)]
    if name == "F3":                                   # _freeze_word_embedding()
        return [n for n in ALL if "word" not in n]
    if name == "F4":
        return [n for n in ALL if n.startswith(("unimo.encoder.text_layer.10.", "unimo.encoder.text_layer.11.", "cls."))]
    raise KeyError(name)


def on(p, prefix=""):
    return sorted(k for k, v in p.groups.items() if v and k.startswith(prefix))


def test_launch_groups_cover_every_live_parameter_once_per_block():
    g = launch_groups(N, FUSE)
    named = [n for names in g.values() for n in names]
    assert set(named) == set(ALL)
    assert sorted(named) == sorted(ALL + [WORD])       # the tied word embedding sits in two groups (T_emb scatter and the decoder's rows), nothing else repeats
    assert len(g["t3.qkv"]) == 6 and len(g["v3.qkv"]) == 6     # the fused q/k/v weight + bias launch is ONE group


def test_plan_U_runs_everything():
    p = plan(regime("U"))
    assert p.full and all(p.groups.values())
    assert p.text == [6] * N and p.vision == [7] * N
    assert p.dvis == [False] * FUSE + [True] * (N - FUSE) and p.dprefix == [False] * FUSE + [True] * (N - FUSE)
    assert p.head_ln and p.head_act and p.head_din and p.temb and p.vemb
    assert p.written == set(ALL)


def test_plan_F1_word_embedding_only():
    p = plan(regime("F1"))
    assert on(p) == ["head.word", "temb.word"]                          # head: the tied decoder's row gradients; no cls.predictions.bias, no transform gradients
    assert p.head_ln and p.head_act and p.head_din                      # d(rows) flows through the head transform into the text chain
    assert p.text == [6] * N                                            # T_11 .. T_0: the full data-gradient chain, no parameter launch (checked by on(p) above)
    assert p.temb                                                       # dropout + LN data gradient, scatter into the word table only
    assert not p.g("temb.pos") and not p.g("temb.type") and not p.g("temb.ln")
    # vision: as F2
    assert p.vision == [-1] * 8 + [5, 7, 7, 7] and not p.vemb
    assert p.dvis == [False] * 8 + [True] * 4 and p.dprefix == [False] * 8 + [True] * 4
    assert p.written == {WORD}


def test_plan_F2_vision_tower_frozen():
    p = plan(regime("F2"))
    assert not on(p, "v") and all(v for k, v in p.groups.items() if not k.startswith("v"))     # text + head: everything; vision: no parameter gradient
    assert p.text == [6] * N and p.dvis == [False] * 8 + [True] * 4     # including the fusion's d(vis) for l = 8 .. 11
    assert p.vision[9:] == [7, 7, 7]                                    # V_11, V_10, V_9: the whole data-gradient chain
    assert p.vision[8] == 5 and p.dprefix[8]                            # V_8: through the attention backward (dpk / dpv feed T_7); no q/k/v data-gradient GEMM, no LN1 backward
    assert p.vision[:8] == [-1] * 8 and not p.vemb                      # V_7 .. V_0 and the vision embeddings: nothing
    for l in range(8):                                                  # ... and their forward keeps nothing
        assert not any(p.keeps("v", l, k) for k in ("x", "m1", "r1", "h1", "qkv", "ctx", "lse", "x1", "m2", "r2", "h2", "z", "f", "pre"))
    assert not p.keeps("v", 8, "x") and not p.keeps("v", 8, "h1") and not p.keeps("v", 8, "f") and p.keeps("v", 8, "z") and p.keeps("v", 8, "lse")
    assert not p.keeps("v", 11, "f") and not p.keeps("v", 11, "h2") and p.keeps("v", 11, "x")
    # launches that disappear against U (what tests/test_frozen_gpu.py counts): 4 weight-gradient GEMMs per vision layer + the patch embedding's,
    # attention backward of V_0 .. V_7, both LayerNorms of V_0 .. V_7 + LN1 of V_8 + the pre-LayerNorm, 4 data-gradient GEMMs of V_0 .. V_7 + V_8's q/k/v one
    u = plan(regime("U"))
    assert sum(u.g(f"v{l}.{k}") - p.g(f"v{l}.{k}") for l in range(N) for k in ("fc2", "fc1", "o", "qkv")) + 1 == 49
    assert sum(u.vision[l] >= 5 for l in range(N)) - sum(p.vision[l] >= 5 for l in range(N)) == 8
    ln = lambda q: sum((q.vision[l] >= 3) + (q.vision[l] >= 7) for l in range(N)) + q.vemb
    assert ln(u) - ln(p) == 18
    nt = lambda q: sum(sum(q.vision[l] >= d for d in (1, 2, 4, 6)) for l in range(N))
    assert nt(u) - nt(p) == 33


def test_plan_F3_word_embedding_frozen():
    p = plan(regime("F3"))
    assert sorted(k for k, v in p.groups.items() if not v) == ["head.word", "temb.word"]     # everything except the word-table scatter and the decoder's row gradients
    assert p.g("head.bias") and p.head_din                                                   # d(rows) through the scoring GEMM stays
    assert p.text == [6] * N and p.vision == [7] * N and all(p.dvis[8:]) and p.temb and p.vemb
    assert p.written == set(ALL) - {WORD}


def test_plan_F4_top_two_text_layers_and_head():
    p = plan(regime("F4"))
    assert on(p, "head") == ["head.bias", "head.dense", "head.ln"]      # (the tied word table is not under cls.*)
    assert p.text[11] == 6 and len(on(p, "t11.")) == 8                  # head and T_11: full
    assert p.text[10] == 5 and len(on(p, "t10.")) == 8                  # T_10: parameter gradients, no data gradient into its input
    assert p.dvis[11] and not p.dvis[10]                                # T_11's fusion d(vis) runs (V_11's prefix comes from T_10's key / value weights), T_10's does not
    assert p.vision[11] == 5 and p.dprefix[11]                          # V_11: through the attention backward for dpk / dpv only
    assert p.text[:10] == [-1] * 10 and p.vision[:11] == [-1] * 11 and not p.temb and not p.vemb      # every other block: nothing
    assert not any(p.keeps("t", 3, k) for k in ("s2", "ht", "zt", "ab", "ctx", "qkv", "xb", "s1"))    # ... forward keeps nothing
    assert not any(p.keeps("v", 10, k) for k in ("x", "qkv", "z", "f"))


def test_plan_partly_frozen_group_runs_as_a_whole():
    q = "unimo.encoder.text_layer.9.attention.self.query.weight"
    p = plan([n for n in ALL if n != q])
    assert all(p.groups.values()) and p.text == [6] * N and p.vision == [7] * N
    assert q in p.written                                               # still written by the fused q/k/v launch: cleared by its zero-only chunk
    # only the query frozen in an otherwise frozen model: T_9's key / value feed V_10's prefix, the query does not
    p = plan(["unimo.encoder.text_layer.9.attention.self.key.weight"])
    assert p.dprefix[10] and p.vision[10] == 5 and p.text[9] == 5 and p.text[10] == 6 and p.text[11] == 6 and not p.dvis[9]
    p = plan(["unimo.encoder.text_layer.9.attention.self.query.weight"])
    assert not p.dprefix[10] and p.vision == [-1] * 11 + [5] and p.dprefix[11] and p.text[9] == 5     # (V_11's prefix is the K / V of T_10, whose INPUT depends on that query)


def test_plan_nothing_trainable_upstream_of_the_head():
    p = plan([BIAS])
    assert on(p) == ["head.bias"] and not p.head_ln and not p.head_din and p.text == [-1] * N and p.vision == [-1] * N
    p = plan([])
    assert not on(p) and p.written == set()


# ---------------------------------------------------------------------------------------------- chunk table
def _slots():
    slots, off = {}, 0
    for n in layout_order(N):
        numel = 1 if "adaptive_weight" in n else (768 * 768 if n.endswith("weight") and "LayerNorm" not in n and "layer_norm" not in n else 768)
        if n.endswith("adaptive_weight.1"):
            prev = slots[n[:-1] + "0"]
            slots[n] = Slot(n, (1,), prev.offset + prev.numel, 1)
            continue
        slots[n] = Slot(n, (numel,), off, numel)
        off += ((numel + 255) // 256) * 256
    return slots


def _owner(slots, start):
    return next(n for n, s in slots.items() if s.offset <= start < s.offset + max(s.numel, 1) and not n.endswith("adaptive_weight.1"))


def test_chunk_table_of_a_frozen_store():
    slots, order = _slots(), layout_order(N)
    base = chunk_table(order, slots, DEAD, frozenset(), None, text_f16_weight)
    assert {_owner(slots, c[0]) for c in base} == {n for n in ALL if not n.endswith("adaptive_weight.1")}
    assert all(c[2] & ZERO_ONLY == 0 for c in base)
    # F2 under the schedule tier: frozen tensors nobody writes have no chunk at all; the trainable ones keep their chunks unchanged
    frozen = frozenset(n for n in ALL if n.startswith(VISION))
    p = plan(regime("F2"))
    t = chunk_table(order, slots, DEAD, frozen, p.written, text_f16_weight)
    assert t == [c for c in base if _owner(slots, c[0]) not in frozen]
    # the same set under an engine that skips nothing (FLAVA, ViLT, VisualBERT, fp32 training): every frozen tensor carries the zero-only flag, and only it
    t = chunk_table(order, slots, DEAD, frozen, None, text_f16_weight)
    assert [c[:2] for c in t] == [c[:2] for c in base]
    for c in t:
        assert c[2] == (ZERO_ONLY if _owner(slots, c[0]) in frozen else next(b[2] for b in base if b[0] == c[0]))
    # a partly frozen launch group: its frozen member is zero-only, its trainable members update as before
    q = "unimo.encoder.text_layer.9.attention.self.query.weight"
    p = plan([n for n in ALL if n != q])
    t = chunk_table(order, slots, DEAD, frozenset([q]), p.written, text_f16_weight)
    assert [c[:2] for c in t] == [c[:2] for c in base]
    assert {_owner(slots, c[0]) for c in t if c[2] == ZERO_ONLY} == {q} and all(c[2] in (ZERO_ONLY,) or c[2] < ZERO_ONLY for c in t)
    # one adaptive weight of a pair frozen: the packed two-element chunk splits
    a0 = "unimo.encoder.text_layer.3.attention.self.adaptive_weight.0"
    t = chunk_table(order, slots, DEAD, frozenset([a0]), None, text_f16_weight)
    s0 = slots[a0]
    assert [s0.offset, 1, ZERO_ONLY] in t and [s0.offset + 1, 1, 1] in t
    assert [s0.offset, 2, 1] in base


def test_decay_flag_follows_the_substring_rule():
    slots, order = _slots(), layout_order(N)
    for c in chunk_table(order, slots, DEAD, frozenset(), None, None):
        assert c[2] == (0 if any(nd in _owner(slots, c[0]) for nd in NO_DECAY) else 1)


# ---------------------------------------------------------------------------------------------- model surface
def _tiny():
    from mkg_analogy_amd.models import MKGformerKGC, TextConfig, VisionConfig
    small = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128)
    return MKGformerKGC(VisionConfig(patch_size=32, **small), TextConfig(vocab_size=100, max_position_embeddings=32, **small))


def test_freeze_hooks_follow_the_reference_rule():
    from mkg_analogy_amd.lit_models import TransformerLitModel
    for hook, keep in (("_freeze_attention", lambda n: "word" in n), ("_freeze_word_embedding", lambda n: "word" not in n)):
        m = _tiny()
        lit = types.SimpleNamespace(model=m)
        lit._set_word_rule = types.MethodType(TransformerLitModel._set_word_rule, lit)
        getattr(TransformerLitModel, hook)(lit)
        names = [n for n, p in m.named_parameters() if p.requires_grad]
        assert names == [n for n, _ in m.named_parameters() if keep(n)] and names
    assert [n for n, _ in _tiny().named_parameters() if "word" in n] == [WORD]
    # the full-size names: exactly the requires_grad lists of the unmodified reference's own hooks (golden G12, tools/gen_goldens_frozen.py), and --
    # minus the dead tensors, which keep their flag and are simply never updated -- the F1 / F3 sets the plan tests use
    import os
    import numpy as np
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    full = layout_order(N)
    for tag, keep, reg in (("f1", lambda n: "word" in n, "F1"), ("f3", lambda n: "word" not in n, "F3")):
        ref = np.load(os.path.join(gold, f"g12_frozen_{tag}.npz"), allow_pickle=False)["trainable"].tolist()
        assert sorted(ref) == sorted(n for n in full if keep(n))
        assert sorted(n for n in ref if not n.startswith(DEAD)) == sorted(regime(reg))
    ref = np.load(os.path.join(gold, "g12_frozen_f2.npz"), allow_pickle=False)["trainable"].tolist()
    assert sorted(n for n in ref if not n.startswith(DEAD)) == sorted(regime("F2"))


def test_freeze_and_unfreeze_set_flags_only():
    m = _tiny()
    m.freeze("unimo.vision_", "unimo.encoder.vision_layers.")
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert frozen and all(n.startswith(VISION) for n in frozen)
    assert len(frozen) == sum(n.startswith(VISION) for n, _ in m.named_parameters())
    assert m._store is None and m._flags is None                       # nothing else happened
    m.unfreeze("unimo.encoder.vision_layers.1.")
    assert all(p.requires_grad for n, p in m.named_parameters() if n.startswith("unimo.encoder.vision_layers.1."))
    m.unfreeze()
    assert all(p.requires_grad for p in m.parameters())
    with pytest.raises(ValueError):
        m.freeze("no.such.prefix")


class _StubStore:
    """What sync_trainable() needs of a FlatStore, without device memory."""
    dead = ()

    def __init__(self, names):
        self.order, self.frozen, self.written, self.zeroed = list(names), frozenset(), None, 0

    def still_bound(self):
        return True

    def rebuild_chunks(self, extra_dead=(), frozen=None, written=None):
        if frozen is not None:
            self.frozen = frozenset(frozen)
        self.written = written

    def trainable_names(self):
        return [n for n in self.order if n not in self.frozen]

    def zero_grad(self):
        self.zeroed += 1


def test_flag_changed_after_sync_raises_at_the_next_training_forward():
    m = _tiny()
    m._store = st = _StubStore([n for n, _ in m.named_parameters()])
    m._anchor = torch.zeros(1, requires_grad=True)
    m.freeze("unimo.vision_")
    names = m.sync_trainable()
    assert names == [n for n, p in m.named_parameters() if p.requires_grad] and st.zeroed == 0
    assert st.frozen == {n for n, _ in m.named_parameters() if n.startswith("unimo.vision_")}
    ids = torch.zeros((1, 4), dtype=torch.long)
    m.train()
    m._check_trainable()                                                # unchanged flags: fine
    victim = "unimo.encoder.text_layer.1.output.dense.bias"
    m.get_parameter(victim).requires_grad_(False)
    with pytest.raises(RuntimeError, match=victim.replace(".", r"\.")):
        m(input_ids=ids, pixel_values=torch.zeros(1, 2, 3, 32, 32))     # refused before any kernel is reached
    with torch.no_grad():
        m._check_trainable()                                            # no gradient is asked for: nothing to refuse
    m.eval()
    m._check_trainable()
    m.train()
    m.sync_trainable()                                                  # reading the flags again accepts the new set, and zero-fills the gradients once
    assert st.zeroed == 1 and victim in st.frozen
    m._check_trainable()
    m.sync_trainable()
    assert st.zeroed == 1                                               # same set: no second fill
    m.freeze()
    m.sync_trainable()
    assert not m._anchor.requires_grad                                  # nothing trainable: the output needs no gradient, loss.backward() fails as torch does
    m.unfreeze()
    m.sync_trainable()
    assert m._anchor.requires_grad
