"""G12: six-step AdamW trajectories of the UNMODIFIED reference with FROZEN parameters.

Run where the reference tree is available (it is not needed by any test, and it does not exist on the GPU box):

    python tools/gen_goldens_frozen.py            # writes tests/golden/g12_frozen_{f1,f2,f3}.npz

TEST INFRASTRUCTURE ONLY (the rules of oracle/gen_goldens_traj.py: the reference modules are imported in place, nothing of them is copied,
only inputs and recorded outputs are stored).

The setup is G11's (oracle/gen_goldens_traj.py): the same six batches, conditioned weights (seed 7), B = 4, L = 64, patch 32, both dropout
probabilities 0, ``num_training_steps`` 12, the optimizer and scheduler of the reference's own ``configure_optimizers`` -- which filters on
``requires_grad`` (lit_models/transformer.py:228-229).  Before it is called the flags are set by

  f1   the reference's own ``lm._freeze_attention()``        (only names containing "word" keep training)
  f2   ``requires_grad_(False)`` on the vision tower          (``unimo.vision_*`` and ``unimo.encoder.vision_layers.*``)
  f3   the reference's own ``lm._freeze_word_embedding()``    (names containing "word" are frozen)

Each regime's file holds its three runs: ``main`` and the two controls of G11, ``ctlbf::`` (weight matrices rounded once to bf16) and ``ctl32::``
(initial weights moved by one fp32 ulp).  Per run: per-step ``loss`` and ``lr``; of ``main`` also the tensors whose ``grad is None`` after step 1
(``none_grad``) and the ``requires_grad`` name list (``trainable``).  Delta samples ``d2:: d4:: d6::<name>`` of every tensor of ``sample_names()``: every
``SUB``-th value of G11's 1024-value ``grad_sample`` (three runs share one file below 1 MiB).  For f1 / f3 the word-row quantities of G11
(``wrows::d6``, ``wrows_norm::d6``, ``never::w6``, and ``never0``).

Asserted here, on the CPU: every trainable sampled tensor has a delta norm (and a sample norm) of at least G11's ``DEAD_NORM`` -- nothing trainable may
be left out of a gate --; every frozen sampled tensor has a delta of exactly 0; in f3 the "never" rows equal their initial values bit for bit (no
weight decay on a frozen table); in f1 they obey G11's closed-form shrink within 6 * 2^-23 * |w0|.
"""
from __future__ import annotations

import argparse as ap
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
from oracle.gen_goldens import load_reference  # noqa: E402
from oracle.gen_goldens_full import build_reference, grad_sample, sample_names  # noqa: E402
from oracle.gen_goldens_traj import (B, BASE, BATCH_SEEDS, DEAD_NORM, L, NE, NEVER_COLS, NR, PATCH, SNAP, ULP_SEED, WEIGHT_SEED, WORD, WORD_COLS,  # noqa: E402
                                     bf16_matrices, ulp_perturb, word_rows)

SUB = 4                                             # every SUB-th value of grad_sample's 1024
TOTAL_STEPS = 12
VISION = ("unimo.vision_", "unimo.encoder.vision_layers.")


def set_flags(regime, model, lm):
    if regime == "f1":
        lm._freeze_attention()
    elif regime == "f3":
        lm._freeze_word_embedding()
    else:
        for n, p in model.named_parameters():
            if n.startswith(VISION):
                p.requires_grad_(False)


def run(lit, unimo, regime, sd0, cfg, batches, occ, never):
    model, lm = build_reference(lit, unimo, PATCH, sd0, False, cfg, dropout=0.0)
    model.train()
    type(lm).num_training_steps = property(lambda self: TOTAL_STEPS)
    set_flags(regime, model, lm)
    oc = lm.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    named = dict(model.named_parameters())
    trainable = [n for n, p in named.items() if p.requires_grad]
    names = list(sample_names())
    start = {n: named[n].detach().double().clone() for n in names}
    word0 = named[WORD].detach().clone()
    nv, oc_rows = torch.from_numpy(never), torch.from_numpy(occ)
    out = {"never0": word0[nv].numpy().copy()}
    losses, lrs, none_grad = [], [], None
    opt.zero_grad()
    for i, batch in enumerate(batches):
        loss = lm.training_step({k: v.clone() for k, v in batch.items()}, i)
        loss.backward()
        losses.append(float(loss.detach()))
        if none_grad is None:
            none_grad = sorted(n for n, p in named.items() if p.grad is None)
        lrs.append(float(opt.param_groups[0]["lr"]))
        opt.step()
        sched.step()
        opt.zero_grad()
        k = i + 1
        if k not in SNAP:
            continue
        for n in names:
            d = named[n].detach().double() - start[n]
            s = grad_sample(d.float())[::SUB].copy()
            if n in trainable and n not in none_grad:
                assert float(d.norm()) >= DEAD_NORM and float(np.linalg.norm(s.astype(np.float64))) >= DEAD_NORM, (regime, n, k)
            else:
                assert float(d.abs().max()) == 0.0, (regime, n, k)          # frozen (or dead): not one bit
            out[f"d{k}::{n}"] = s
    if regime in ("f1", "f3"):
        k = SNAP[-1]
        dw = named[WORD].detach().double() - word0.double()
        out[f"wrows::d{k}"] = dw[oc_rows][:, ::WORD_COLS].float().numpy().copy()
        out[f"wrows_norm::d{k}"] = dw[oc_rows].norm(dim=1).numpy().copy()
        last = named[WORD].detach()[nv]
        out[f"never::w{k}"] = last[:, ::NEVER_COLS].numpy().copy()
        w0 = word0[nv].double()
        if regime == "f3":
            assert torch.equal(last, word0[nv]), "a frozen table gets no weight decay"
        else:
            f = float(np.prod([1.0 - lr * 0.01 for lr in lrs]))
            assert f < 1.0 and bool(((last.double() - w0 * f).abs() <= 6 * 2.0 ** -23 * w0.abs()).all()), "closed-form shrink of G11"
    out["loss"], out["lr"] = np.asarray(losses, np.float64), np.asarray(lrs, np.float64)
    return out, none_grad, trainable


def main():
    p = ap.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    p.add_argument("--regimes", default="f1,f2,f3")
    a = p.parse_args()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
    t0 = time.time()
    lit, unimo = load_reference()
    cfg = D.data_config(seed=1234)
    sd0 = O.condition_weights(O.init_params(O.VisionCfg(patch_size=PATCH), O.TextCfg(vocab_size=BASE + NE + NR), seed=WEIGHT_SEED))
    batches = [D.make_batch(B, L, seed=s) for s in BATCH_SEEDS]
    occ, never = word_rows(cfg, batches)
    starts = {"main": sd0, "ctlbf": bf16_matrices(sd0), "ctl32": ulp_perturb(sd0, ULP_SEED)}
    for regime in a.regimes.split(","):
        rec = dict(patch=np.int64(PATCH), B=np.int64(B), L=np.int64(L), weight_seed=np.int64(WEIGHT_SEED), batch_seeds=np.asarray(BATCH_SEEDS, np.int64),
                   snap=np.asarray(SNAP, np.int64), sub=np.int64(SUB), num_training_steps=np.int64(TOTAL_STEPS), word_rows=occ, never_rows=never,
                   word_cols=np.int64(WORD_COLS), never_cols=np.int64(NEVER_COLS))
        for tag, sd in starts.items():
            out, none_grad, trainable = run(lit, unimo, regime, sd, cfg, batches, occ, never)
            pre = "" if tag == "main" else tag + "::"
            if tag == "main":
                rec["none_grad"], rec["trainable"] = np.array(none_grad), np.array(trainable)
            else:
                assert none_grad == rec["none_grad"].tolist() and trainable == rec["trainable"].tolist()
                out.pop("never0")
            rec.update({pre + k: v for k, v in out.items()})
            print(f"{regime} {tag}: lr {out['lr'].tolist()} loss {out['loss'].tolist()} ({time.time() - t0:.0f} s)", flush=True)
        path = os.path.join(a.out, f"g12_frozen_{regime}.npz")
        np.savez_compressed(path, **rec)
        n = os.path.getsize(path)
        print(f"   {path}: {n} bytes, {len(rec['none_grad'])} tensors without a gradient, {len(rec['trainable'])} trainable", flush=True)
        assert n < (1 << 20), (path, n)


if __name__ == "__main__":
    main()
