"""Throughput of the VisualBERT fine-tune step (VisualBertKGC, Trainer.train_step, dropout on) on one GPU: examples/s at B = 64
(scripts/run_finetune_visualbert.sh) and B = 256, L = 64, V = 72 random region features, plus the fraction of the bf16 MFMA peak
(2.5 PFLOP/s dense) the step reaches.  Prints one JSON line; ``--out`` also writes it.

    python tools/bench_visualbert.py [--batches 64 256] [--seq-len 64] [--steps 10] [--warmup 3] [--out profiles/r08_visualbert_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, I, NL, V, FEAT = 768, 3072, 12, 72, 2048


def visualbert_fwd_gflop_per_example(L: int = 64, A: int = 2063) -> float:
    """Multiply-add flops x 2 of one example's forward pass: visual projection, 12 layers over S = L + V tokens (four H x H and two H x I
    products, QK^T and PV), head transform on all S rows and the scored entity columns of the [MASK] row."""
    S = L + V
    f = 2 * V * H * FEAT + NL * S * (8 * H * H + 4 * H * I) + NL * 4 * S * S * H + 2 * S * H * H + 2 * A * H
    return f / 1e9


def run(B: int, L: int, steps: int, warmup: int, dev) -> dict:
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.lit_models import TransformerLitModel
    from mkg_analogy_amd.models import VisualBertKGC, visual_bert_config
    from mkg_analogy_amd.trainer import Trainer
    torch.manual_seed(0)
    model = VisualBertKGC(visual_bert_config(vocab_size=30522))
    cfg = D.data_config(seed=1234)
    args = argparse.Namespace(label_smoothing=0.1, alpha=0.43, pretrain=0, lr=4e-5, weight_decay=0.01, optimizer="AdamW", warm_up_radio=0.1)
    lit = TransformerLitModel(model=model, args=args, tokenizer=D.FakeTokenizer(), data_config=cfg)
    model.to(dev)
    lit._init_relation_word()
    batch = D.make_batch(B, L, image_size=2, seed=1234, device=dev)
    batch["pixel_values"] = torch.randn((B, V, FEAT), generator=torch.Generator().manual_seed(1234)).abs().to(dev)
    vm = torch.ones((B, V))
    vm[torch.rand(B, generator=torch.Generator().manual_seed(5)) < 0.4, V // 2:] = 0.0     # single-entity examples: the second block masked
    batch["pixel_values"] *= vm[:, :, None].to(dev)
    batch["visual_attention_mask"] = vm.to(dev)
    total = steps + warmup + 4
    tr = Trainer(max_epochs=1, max_steps=10 * total, world_size=1)
    tr._setup(lit, [None] * (10 * total))
    for i in range(warmup):
        tr.train_step(lit, batch, i)
    tr.settle_pool()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = None
    for i in range(steps):
        loss = tr.train_step(lit, batch, warmup + i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ex = B * steps / dt
    gf = 3.0 * visualbert_fwd_gflop_per_example(L)
    out = {"B": B, "L": L, "S": L + V, "steps": steps, "warmup": warmup, "value": round(ex, 2), "unit": "examples/s",
           "step_ms": round(dt / steps * 1e3, 3), "train_gflop_per_example": round(gf, 1), "step_frac_of_mfma_peak": round(ex * gf / 2.5e6, 4),
           "last_loss": round(float(loss), 5)}
    del model, lit, tr, batch
    torch.cuda.empty_cache()
    return out


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    a.add_argument("--seq-len", type=int, default=64)
    a.add_argument("--steps", type=int, default=10)
    a.add_argument("--warmup", type=int, default=3)
    a.add_argument("--out", default=None)
    a = a.parse_args()
    from mkg_analogy_amd import ops
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    legs = [run(B, a.seq_len, a.steps, a.warmup, dev) for B in a.batches]
    res = {"metric": "visualbert_finetune_train_examples_per_s", "device": torch.cuda.get_device_name(0), "legs": legs,
           "fwd_gflop_per_example": round(visualbert_fwd_gflop_per_example(a.seq_len), 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
