"""G11: a six-step AdamW TRAJECTORY of the UNMODIFIED reference (fine-tune loss, real dimensions, CLIP-B/32 patches, L = 64, B = 4).

Run in the build container only (the reference does not exist on the GPU box):

    python oracle/gen_goldens_traj.py            # writes tests/golden/g11_traj*.npz

TEST INFRASTRUCTURE ONLY (same rules as gen_goldens_full.py: the reference modules are imported in place, no reference source is
copied, only inputs + recorded outputs are stored).

What runs: ``lm.training_step`` -> ``backward`` -> ``opt.step()`` -> ``sched.step()`` with the optimizer and the scheduler of the
reference's own ``configure_optimizers`` (lit_models/transformer.py:224-241), ``num_training_steps`` patched to a constant as G4
does.  Conditioned weights (seed 7), fp32, BOTH BERT dropout probabilities 0 so that ``model.train()`` is deterministic; a DIFFERENT
batch every step (seeds ``BATCH_SEEDS``), so that ``v`` is a real history.

  main    six optimizer steps, num_training_steps 12 (1.2 warm-up steps: the six steps span warm-up and decay; the product's Trainer
          derives 12 from six batches and max_epochs = 2).  The learning rate BEFORE step 0 is 0: the first step moves only m and v.
  acc2    the same six batches as three optimizer steps of two micro-batches (loss / 2 per micro-batch, as PL accumulates),
          num_training_steps 6 (six batches, accumulate 2, max_epochs 2).
  ctlbf   the same runs from weight matrices rounded ONCE to bf16 (the rule of gen_goldens_full.py:run), and
  ctl32   from initial weights moved by ONE fp32 ulp up or down (seeded).  They say how far rounding alone moves an AdamW trajectory:
          AdamW is sign-like while v is young, so an element whose gradient is smaller than the gradient error gets a full +-lr of the
          wrong sign.  Single weight elements are therefore not comparable between two correct implementations; norms of deltas and
          the loss are, and the GPU tests bound them by multiples of these controls.

Files (each below 1 MiB; a delta is ``w_k - w_0`` of the run's own initial weights, taken in float64 and stored as float32):
  g11_traj.npz        inputs of the six batches (integers + pixel checksums), per-step loss / lr of every run, the tensors whose
                      gradient is None after step 1, ``w0::<name>`` strided samples (``grad_sample`` rule, 1024 values: the WHOLE of
                      every tensor of up to 1024 elements) of ``sample_names()``, the scored slice of cls.predictions.bias, the ids of
                      the word-embedding rows that occur in the batches and of 64 rows that neither occur nor are scored.
  g11_traj_main.npz   ``d2:: d4:: d6::<name>`` delta samples after optimizer steps 2, 4, 6 (steps counted from 1), word-embedding rows.
  g11_traj_ctlbf.npz, g11_traj_ctl32.npz   the same for the two controls.
  g11_traj_acc2.npz   ``d3::<name>`` after the third optimizer step of acc2, and ``ctlbf::d3::`` / ``ctl32::d3::`` of its controls.
"""
from __future__ import annotations

import argparse as ap
import os
import sys
import time

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import mkgformer_oracle as O  # noqa: E402
from oracle.gen_goldens import load_reference  # noqa: E402
from oracle.gen_goldens_full import build_reference, grad_sample, sample_names  # noqa: E402
from mkg_analogy_amd import data_synth as D  # noqa: E402

BASE, NE, NR = D.BASE_VOCAB, D.N_ENT, D.N_REL
PATCH, B, L = 32, 4, 64
WEIGHT_SEED, ULP_SEED = 7, 1107
BATCH_SEEDS = (101, 202, 303, 404, 505, 606)
SNAP = (2, 4, 6)                                    # optimizer steps (counted from 1) after which the weights are sampled
WORD = "unimo.text_embeddings.word_embeddings.weight"
BIAS = "cls.predictions.bias"
WORD_COLS, NEVER_COLS = 48, 8                       # column strides of the stored word-embedding rows
DEAD_NORM = 1e-9                                    # cap of the GPU tests: only tensors whose reference delta norm is below this may be left out


def ulp_perturb(sd, seed):
    """Every value one fp32 ulp up or down (a factor 1 +- 2^-24 would round back to the same float)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in sorted(sd):
        v = sd[k]
        up = torch.from_numpy(rng.integers(0, 2, size=v.numel(), dtype=np.uint8).astype(bool)).view(v.shape)
        out[k] = torch.where(up, torch.nextafter(v, torch.full_like(v, float("inf"))), torch.nextafter(v, torch.full_like(v, -float("inf"))))
    return out


def bf16_matrices(sd):
    return {k: (v.to(torch.bfloat16).float() if v.dim() >= 2 and "embeddings" not in k else v) for k, v in sd.items()}


def word_rows(cfg, batches):
    """(rows that occur as input tokens, 64 rows that neither occur nor are scored: zero gradient, weight decay only)."""
    occ = np.unique(np.concatenate([b["input_ids"].numpy().ravel() for b in batches]))
    scored = set(int(i) for i in cfg["analogy_entity_ids"])
    busy = set(int(i) for i in occ) | scored
    never = [r for r in range(997, D.VOCAB, 331) if r not in busy][:64]
    assert len(never) == 64
    return occ.astype(np.int64), np.asarray(never, np.int64)


def trajectory(lit, unimo, sd0, cfg, batches, accumulate, total_steps, snaps, occ, never):
    model, lm = build_reference(lit, unimo, PATCH, sd0, False, cfg, dropout=0.0)
    model.train()
    type(lm).num_training_steps = property(lambda self: total_steps)
    oc = lm.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    named = dict(model.named_parameters())
    names = [n for n in sample_names()]
    w0 = {n: named[n].detach().double().clone() for n in names}
    word0 = named[WORD].detach().double().clone()
    res = {"w0": {n: grad_sample(named[n]) for n in names}, "bias0": named[BIAS].detach()[torch.tensor(cfg["analogy_entity_ids"])].numpy().copy(),
           "never0": named[WORD].detach()[torch.from_numpy(never)].numpy().copy()}
    losses, lrs, none_grad = [], [], None
    opt.zero_grad()
    for i, batch in enumerate(batches):
        loss = lm.training_step({k: v.clone() for k, v in batch.items()}, i)
        (loss / accumulate).backward()
        losses.append(float(loss.detach()))
        if (i + 1) % accumulate:
            continue
        k = (i + 1) // accumulate
        if none_grad is None:
            none_grad = sorted(n for n, p in named.items() if p.grad is None)
        lrs.append(float(opt.param_groups[0]["lr"]))
        opt.step()
        sched.step()
        opt.zero_grad()
        if k == 1:
            assert lrs[0] == 0.0 and all(torch.equal(named[n].detach().double(), w0[n]) for n in names), "lr(0) = 0: the first step moves nothing"
        if k in snaps:
            for n in names:
                d = named[n].detach().double() - w0[n]
                if n not in none_grad:
                    assert float(d.norm()) >= DEAD_NORM, (n, k, float(d.norm()))     # nothing but the dead tensors is below the cap
                res[f"d{k}::{n}"] = grad_sample(d.float())
                assert n in none_grad or float(np.linalg.norm(res[f"d{k}::{n}"].astype(np.float64))) >= DEAD_NORM, (n, k)   # ... nor is its sample
        if k == snaps[-1]:
            dw = named[WORD].detach().double() - word0
            res[f"wrows::d{k}"] = dw[torch.from_numpy(occ)][:, ::WORD_COLS].float().numpy().copy()
            res[f"wrows_norm::d{k}"] = dw[torch.from_numpy(occ)].norm(dim=1).numpy().copy()
            res[f"never::w{k}"] = named[WORD].detach()[torch.from_numpy(never)][:, ::NEVER_COLS].numpy().copy()
            ids = torch.tensor(cfg["analogy_entity_ids"])
            res[f"bias::d{k}"] = (named[BIAS].detach()[ids].double() - torch.from_numpy(res["bias0"]).double()).float().numpy().copy()
    res["loss"], res["lr"], res["none_grad"] = np.asarray(losses, np.float64), np.asarray(lrs, np.float64), none_grad
    return res


def main():
    p = ap.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = p.parse_args()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
    t0 = time.time()
    lit, unimo = load_reference()
    cfg = D.data_config(seed=1234)
    sd0 = O.condition_weights(O.init_params(O.VisionCfg(patch_size=PATCH), O.TextCfg(vocab_size=BASE + NE + NR), seed=WEIGHT_SEED))
    batches = [D.make_batch(B, L, seed=s) for s in BATCH_SEEDS]
    occ, never = word_rows(cfg, batches)
    starts = {"main": sd0, "ctlbf": bf16_matrices(sd0), "ctl32": ulp_perturb(sd0, ULP_SEED)}
    base = dict(patch=np.int64(PATCH), B=np.int64(B), L=np.int64(L), conditioned=np.int64(1), weight_seed=np.int64(WEIGHT_SEED),
                ulp_seed=np.int64(ULP_SEED), batch_seeds=np.asarray(BATCH_SEEDS, np.int64), snap=np.asarray(SNAP, np.int64),
                num_training_steps=np.int64(12), acc2_num_training_steps=np.int64(6), word_rows=occ, never_rows=never,
                word_cols=np.int64(WORD_COLS), never_cols=np.int64(NEVER_COLS))
    for i, b in enumerate(batches):
        base.update({f"in{i}::" + k: v.numpy() for k, v in b.items() if k != "pixel_values"})
        pix = b["pixel_values"]
        base[f"pixel_sum{i}"] = np.float64(float(pix.double().sum()))
        base[f"pixel_abs_sum{i}"] = np.float64(float(pix.double().abs().sum()))
    acc2 = {}
    for tag, sd in starts.items():
        r = trajectory(lit, unimo, sd, cfg, batches, 1, 12, SNAP, occ, never)
        r2 = trajectory(lit, unimo, sd, cfg, batches, 2, 6, (3,), occ, never)
        pre = "" if tag == "main" else tag + "::"
        base[pre + "loss"], base[pre + "lr"] = r["loss"], r["lr"]
        base[pre + "acc2::loss"], base[pre + "acc2::lr"] = r2["loss"], r2["lr"]
        if tag == "main":
            base["none_grad"] = np.array(r["none_grad"])
            assert r["none_grad"] == r2["none_grad"]
            base.update({"w0::" + n: v for n, v in r["w0"].items()})
            base["bias0"], base["never0"] = r["bias0"], r["never0"]
        else:
            assert r["none_grad"] == base["none_grad"].tolist()
        np.savez_compressed(os.path.join(a.out, f"g11_traj_{tag}.npz"), **{k: v for k, v in r.items() if "::" in k})
        acc2.update({pre + k: v for k, v in r2.items() if "::" in k})
        print(f"{tag}: lr {r['lr'].tolist()} loss {r['loss'].tolist()}\n   acc2: lr {r2['lr'].tolist()} loss {r2['loss'].tolist()} ({time.time() - t0:.0f} s)", flush=True)
    np.savez_compressed(os.path.join(a.out, "g11_traj_acc2.npz"), **acc2)
    np.savez_compressed(os.path.join(a.out, "g11_traj.npz"), **base)
    print(f"none-grad tensors: {len(base['none_grad'])}; word rows {len(occ)} + {len(never)}")
    for f in sorted(os.listdir(a.out)):
        if f.startswith("g11_"):
            n = os.path.getsize(os.path.join(a.out, f))
            assert n < (1 << 20), (f, n)
            print(f"   {f}: {n} bytes")


if __name__ == "__main__":
    main()
