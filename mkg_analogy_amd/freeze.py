"""What the backward pass of the MKGformer bf16 engine runs when some parameters are frozen (``requires_grad = False``).

Pure host logic (no torch, no GPU): ``backward_plan`` turns the set of trainable parameter names into the list of launches the engine issues.

The rule
  (a) a parameter-gradient launch runs iff a member of its LAUNCH GROUP is trainable.  A launch group is what one weight-gradient GEMM (weight + bias
      column sums), one LayerNorm dgamma / dbeta reduction, one adaptive-weight reduction or one embedding-table scatter writes; the fused q/k/v weight +
      bias launch is one group.
  (b) the data gradient along an edge into block Y runs iff Y, or any forward ancestor of Y, holds a trainable tensor.  The graph is the model's own
      (modeling_unimo.py:589-658): V_emb -> V_0 .. V_{n-1};  T_emb -> T_0 .. T_{n-1} -> head;  for l >= fuse_from the output of V_l enters T_l (fusion) and
      the K / V of T_{l-1} (its input and its key / value weights) enter V_l's attention as the prefix;  the tied word embedding sits in T_emb and in the head.
  (c) the forward pass keeps, per block, only what the part of its backward that runs reads (``KEEP_TEXT`` / ``KEEP_VISION`` below).

Inside a block the backward is a chain, so "how far it runs" is one number, the block's DEPTH (-1: nothing runs):

  text block    0 output-LayerNorm backward   1 d(GELU input) GEMM   2 fusion backward (when d(visual) is wanted)   3 d(attention-output) GEMM and
                attention-output-LayerNorm backward   4 d(context) GEMM (+ the fusion backward's d(hidden))   5 attention backward   6 q/k/v data-gradient GEMM
  vision block  0 (fc2 weight gradient only)   1 fc2 data gradient   2 fc1 data gradient   3 LayerNorm-2 backward   4 out-proj data gradient
                5 attention backward   6 q/k/v data-gradient GEMM   7 LayerNorm-1 backward
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Set, Tuple

WORD, BIAS = "unimo.text_embeddings.word_embeddings.weight", "cls.predictions.bias"

# depth a launch group needs (its operands exist from that stage on)
TEXT_GROUP_DEPTH = {"out_ln": 0, "out": 0, "int": 1, "fus": 1, "ao_ln": 3, "ao": 3, "adaptive": 5, "qkv": 5}
VISION_GROUP_DEPTH = {"fc2": 0, "fc1": 1, "ln2": 3, "o": 3, "qkv": 5, "ln1": 7}
# saved tensors of a block (engine.forward: sv["t{l}"] / sv["v{l}"]) -> (least depth that reads it, launch group that reads it on its own)
KEEP_TEXT = {"s2": (0, None), "m2": (0, None), "r2": (0, None), "ht": (None, "out"), "zt": (1, None), "ab": (None, "int"), "fus": (None, "fus"),
             "probs": (2, None), "visb": (2, None), "visT": (2, None), "ctx": (2, "ao"), "s1": (3, None), "m1": (3, None), "r1": (3, None),
             "qkv": (5, None), "lse": (5, None), "tkw": (5, None), "xb": (None, "qkv"), "sub": (-1, None)}
KEEP_VISION = {"f": (None, "fc2"), "z": (1, None), "h2": (None, "fc1"), "x1": (3, None), "m2": (3, None), "r2": (3, None), "ctx": (5, "o"),
               "qkv": (5, None), "lse": (5, None), "pre": (5, None), "h1": (None, "qkv"), "x": (7, None), "m1": (7, None), "r1": (7, None)}


def launch_groups(n_layers: int, fuse_from: int) -> Dict[str, Tuple[str, ...]]:
    """key -> parameter names of every launch group, in the engine's naming ("t3.qkv", "v0.ln1", "head.word", ...)."""
    g: Dict[str, Tuple[str, ...]] = {}
    h = "cls.predictions.transform."
    g["head.ln"] = (h + "LayerNorm.weight", h + "LayerNorm.bias")
    g["head.dense"] = (h + "dense.weight", h + "dense.bias")
    g["head.word"] = (WORD,)                                  # the tied decoder's row gradients (functional._ScoreFn)
    g["head.bias"] = (BIAS,)
    u = "unimo.text_embeddings."
    g["temb.ln"] = (u + "LayerNorm.weight", u + "LayerNorm.bias")
    g["temb.word"] = (WORD,)
    g["temb.pos"] = (u + "position_embeddings.weight",)
    g["temb.type"] = (u + "token_type_embeddings.weight",)
    for l in range(n_layers):
        t = f"unimo.encoder.text_layer.{l}."
        g[f"t{l}.out_ln"] = (t + "output.LayerNorm.weight", t + "output.LayerNorm.bias")
        g[f"t{l}.out"] = (t + "output.dense.weight", t + "output.dense.bias")
        g[f"t{l}.int"] = (t + "intermediate.dense.weight", t + "intermediate.dense.bias")
        if l >= fuse_from:                                     # below: dead (never in the trainable set)
            g[f"t{l}.fus"] = (t + "intermediate.fusion_dense.weight", t + "intermediate.fusion_dense.bias")
        g[f"t{l}.ao_ln"] = (t + "attention.output.LayerNorm.weight", t + "attention.output.LayerNorm.bias")
        g[f"t{l}.ao"] = (t + "attention.output.dense.weight", t + "attention.output.dense.bias")
        g[f"t{l}.adaptive"] = (t + "attention.self.adaptive_weight.0", t + "attention.self.adaptive_weight.1")
        g[f"t{l}.qkv"] = tuple(t + f"attention.self.{n}.{k}" for k in ("weight", "bias") for n in ("query", "key", "value"))
        v = f"unimo.encoder.vision_layers.{l}."
        g[f"v{l}.fc2"] = (v + "mlp.fc2.weight", v + "mlp.fc2.bias")
        g[f"v{l}.fc1"] = (v + "mlp.fc1.weight", v + "mlp.fc1.bias")
        g[f"v{l}.ln2"] = (v + "layer_norm2.weight", v + "layer_norm2.bias")
        g[f"v{l}.o"] = (v + "self_attn.out_proj.weight", v + "self_attn.out_proj.bias")
        g[f"v{l}.qkv"] = tuple(v + f"self_attn.{n}.{k}" for k in ("weight", "bias") for n in ("q_proj", "k_proj", "v_proj"))
        g[f"v{l}.ln1"] = (v + "layer_norm1.weight", v + "layer_norm1.bias")
    g["vemb.ln"] = ("unimo.vision_pre_layrnorm.weight", "unimo.vision_pre_layrnorm.bias")
    g["vemb.cls"] = ("unimo.vision_embeddings.class_embedding",)
    g["vemb.pos"] = ("unimo.vision_embeddings.position_embedding.weight",)
    g["vemb.patch"] = ("unimo.vision_embeddings.patch_embedding.weight",)
    return g


@dataclass
class Plan:
    n_layers: int
    groups: Dict[str, bool]                                    # launch group -> runs
    text: List[int]                                            # depth of text block l
    vision: List[int]                                          # depth of vision block l
    dvis: List[bool]                                           # the fusion of text layer l computes d(visual)
    dprefix: List[bool]                                        # vision layer l's attention backward is wanted for dpk / dpv (they feed T_{l-1})
    head_ln: bool = True                                       # head transform: LayerNorm backward (data gradient)
    head_act: bool = True                                      # ... GELU backward (the dense layer's weight gradient or d(input) reads it)
    head_din: bool = True                                      # ... data gradient into the text stream
    temb: bool = True                                          # text embedding backward (dropout + LayerNorm data gradient) runs
    vemb: bool = True                                          # vision pre-LayerNorm backward runs
    written: Set[str] = field(default_factory=set)             # parameters some launch writes a gradient for (whole groups)
    full: bool = True                                          # everything runs (the engine's schedule as it was before freezing existed)

    def g(self, key: str) -> bool:
        return self.groups.get(key, False)

    def keeps(self, stream: str, l: int, what: str) -> bool:
        """Does the backward of text ("t") / vision ("v") block ``l`` read the saved tensor ``what``?"""
        depth = (self.text if stream == "t" else self.vision)[l]
        need, grp = (KEEP_TEXT if stream == "t" else KEEP_VISION)[what]
        return (need is not None and depth >= need) or (grp is not None and self.g(f"{stream}{l}.{grp}"))


def backward_plan(trainable_names: Iterable[str], n_layers: int = 12, export_from: int = 7, fuse_from: int = 8) -> Plan:
    """``trainable_names``: the parameters with ``requires_grad`` minus the store's dead tensors.  ``export_from`` is where the text K / V start to
    be exported (= fuse_from - 1 in the model; only checked here)."""
    assert export_from == fuse_from - 1, "vision layer l reads the K / V of text layer l - 1"
    tr = set(trainable_names)
    names = launch_groups(n_layers, fuse_from)
    groups = {k: any(n in tr for n in v) for k, v in names.items()}
    n = n_layers

    def any_of(prefix: str) -> bool:
        return any(on for k, on in groups.items() if k.startswith(prefix))

    # ---- (b) forward ancestry: is anything trainable at or upstream of ...
    t_block = [any_of(f"t{l}.") for l in range(n)]
    v_block = [any_of(f"v{l}.") for l in range(n)]
    kv_names = lambda l: [f"unimo.encoder.text_layer.{l}.attention.self.{a}.{k}" for a in ("key", "value") for k in ("weight", "bias")]
    t_in, t_out, v_in, v_out, kv_src = [False] * n, [False] * n, [False] * n, [False] * n, [False] * n
    for l in range(n):
        t_in[l] = any_of("temb.") if l == 0 else t_out[l - 1]
        v_in[l] = any_of("vemb.") if l == 0 else v_out[l - 1]
        kv_src[l] = l >= fuse_from and (t_in[l - 1] or any(x in tr for x in kv_names(l - 1)))
        v_out[l] = v_in[l] or v_block[l] or kv_src[l]
        t_out[l] = t_in[l] or t_block[l] or (l >= fuse_from and v_out[l])

    text, vision, dvis = [-1] * n, [-1] * n, [False] * n
    for l in range(n):
        d = max([TEXT_GROUP_DEPTH[k] for k in TEXT_GROUP_DEPTH if groups.get(f"t{l}.{k}", False)], default=-1)
        dvis[l] = l >= fuse_from and v_out[l]
        if dvis[l]:
            d = max(d, 2)
        if t_in[l]:
            d = 6
        text[l] = d
        d = max([VISION_GROUP_DEPTH[k] for k in VISION_GROUP_DEPTH if groups[f"v{l}.{k}"]], default=-1)
        if kv_src[l]:
            d = max(d, 5)
        if v_in[l]:
            d = 7
        vision[l] = d
    head_din = t_out[n - 1]
    head_act = head_din or groups["head.dense"]
    head_ln = head_act or groups["head.ln"]
    written = {nm for k, on in groups.items() if on for nm in names[k]}
    full = all(groups.values()) and all(d == 6 for d in text) and all(d == 7 for d in vision) and all(dvis[fuse_from:]) and head_din
    return Plan(n_layers=n, groups=groups, text=text, vision=vision, dvis=dvis, dprefix=kv_src, head_ln=head_ln, head_act=head_act, head_din=head_din,
                temb=any_of("temb."), vemb=any_of("vemb."), written=written, full=full)
