"""Throughput of the MKGformer fine-tune step with frozen parameters, against the unfrozen step OF THE SAME RUN.

Four products -- U (everything trains), F1 (``_freeze_attention()``: only the tied word embedding), F2 (vision tower frozen), F3
(``_freeze_word_embedding()``) -- are built in one process at bench.py's geometry and weights (B = 256, L = 64, conditioned weights, 11 292-entity
head; 196 and 49 patches per image) and timed INTERLEAVED: after ``--warmup`` steps each, ``--rounds`` rounds of ``--block`` steps per regime, in
rotating order, so that whatever else shares the box hits every regime alike.  The yardstick is U in the same run, never a number from another box.

Per regime: ms per step (host clock around a block that ends in a device synchronise), examples/s, the live device bytes at the end of a forward
pass (what the backward pass keeps; the model's own buffers subtracted), and the ratios to U.  Prints one JSON line; ``--out`` also writes it.

    python tools/bench_frozen.py [--patches 16 32] [--rounds 4] [--block 5] [--warmup 5] [--out profiles/r09_frozen_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VISION = ("unimo.vision_", "unimo.encoder.vision_layers.")
REGIMES = ("U", "F1", "F2", "F3")


def product(regime: str, patch: int, B: int, L: int, dev, planned_steps: int):
    from bench import build
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.trainer import Trainer
    model, lit, cfg = build(patch, seed=0, device=dev, entity_head=D.N_ENT)
    D.load_seeded_weights(model, lit, seed=0, conditioned=True)
    if regime == "F1":
        lit._freeze_attention()
    elif regime == "F2":
        model.freeze(*VISION)
    elif regime == "F3":
        lit._freeze_word_embedding()
    tr = Trainer(max_epochs=1, max_steps=10 * planned_steps, world_size=1)
    tr._setup(lit, [None] * (10 * planned_steps))                      # configure_optimizers() reads the flags here
    batch = D.make_batch(B, L, seed=1234, device=dev, n_labels=D.N_ENT)
    rec = {"live": 0, "trainable": len(model.store.trainable_names())}
    step = lit.training_step

    def training_step(b, i):
        base = torch.cuda.memory_allocated()
        loss = step(b, i)
        rec["live"] = max(rec["live"], torch.cuda.memory_allocated() - base)      # (allocator accounting on the host: no synchronise)
        return loss
    lit.training_step = training_step
    return dict(model=model, lit=lit, tr=tr, batch=batch, rec=rec, i=0, t=0.0, n=0, loss=None)


def advance(p, n):
    for _ in range(n):
        p["loss"] = p["tr"].train_step(p["lit"], p["batch"], p["i"])
        p["i"] += 1


def leg(patch: int, B: int, L: int, rounds: int, block: int, warmup: int, dev) -> dict:
    planned = warmup + rounds * block + 4
    ps = {r: product(r, patch, B, L, dev, planned) for r in REGIMES}
    for r in REGIMES:
        advance(ps[r], warmup)
        ps[r]["tr"].settle_pool()
    torch.cuda.synchronize()
    for k in range(rounds):
        order = REGIMES[k % len(REGIMES):] + REGIMES[:k % len(REGIMES)]
        for r in order:
            p = ps[r]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            advance(p, block)
            torch.cuda.synchronize()
            p["t"] += time.perf_counter() - t0
            p["n"] += block
    out = {}
    for r in REGIMES:
        p = ps[r]
        ms = 1e3 * p["t"] / p["n"]
        out[r] = {"ms_per_step": round(ms, 3), "examples_per_s": round(B * 1e3 / ms, 1), "live_bytes_after_forward": int(p["rec"]["live"]),
                  "trainable_tensors": p["rec"]["trainable"], "last_loss": round(float(p["loss"]), 5)}
    for r in REGIMES:
        out[r]["step_time_ratio_to_U"] = round(out[r]["ms_per_step"] / out["U"]["ms_per_step"], 4)
        out[r]["live_bytes_ratio_to_U"] = round(out[r]["live_bytes_after_forward"] / max(1, out["U"]["live_bytes_after_forward"]), 4)
    del ps
    torch.cuda.empty_cache()
    return {"patches_per_image": (224 // patch) ** 2, "batch": B, "seq_len": L, "warmup": warmup, "timed_steps_per_regime": rounds * block,
            "rounds": rounds, "regimes": out}


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--patches", type=int, nargs="+", default=[16, 32], help="patch size: 16 -> 196 patches per image, 32 -> 49")
    a.add_argument("--batch", type=int, default=256)
    a.add_argument("--seq-len", type=int, default=64)
    a.add_argument("--rounds", type=int, default=4)
    a.add_argument("--block", type=int, default=5)
    a.add_argument("--warmup", type=int, default=5)
    a.add_argument("--out", default=None)
    a = a.parse_args()
    from mkg_analogy_amd import ops
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    legs = [leg(p, a.batch, a.seq_len, a.rounds, a.block, a.warmup, dev) for p in a.patches]
    res = {"metric": "mkgformer_finetune_step_with_frozen_parameters", "device": torch.cuda.get_device_name(0),
           "regimes": {"U": "all trainable", "F1": "_freeze_attention(): only the tied word embedding trains", "F2": "vision tower frozen",
                       "F3": "_freeze_word_embedding()"},
           "yardstick": "U of the same run (interleaved blocks, one process)", "legs": legs}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
