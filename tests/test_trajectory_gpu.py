"""What happens BETWEEN training steps, against a six-step AdamW trajectory of the UNMODIFIED reference (golden G11,
oracle/gen_goldens_traj.py): the fused AdamW launched in ranges under the backward pass, gradients zeroed by the update kernel and the
skipped ``zero_grad()``, the bf16 / fp16 / W^T weight shadows refreshed after every update, the tied word embedding, dead tensors, the
warm-up schedule, gradient accumulation, and a save / resume of the optimizer state.

Everything goes through ``Trainer._setup`` + ``Trainer.train_step`` with the defaults (streamed optimizer, fused zeroing, row-subset
last layer); both dropout probabilities are 0 on both sides so that train mode is deterministic.

Exact conditions need no measurement.  The MEASURED conditions compare sampled weight deltas ``w_k - w_0`` and the per-step loss with
the reference.  AdamW is sign-like while ``v`` is young: an element whose gradient is smaller than the gradient error moves by a full
+-lr in the wrong direction, so single elements are not comparable between two correct implementations; norms of deltas and the loss
are.  Every gate is ``multiple x control + floor``: the control is the displacement of the same quantity in the reference's own run
from perturbed initial weights (``ctl32``: every value moved by one fp32 ulp, for the fp32-accurate path; ``ctlbf``: weight matrices
rounded once to bf16, for the bf16 path), the multiple is 4 for L2-type quantities and 8 for the scalar loss (the convention and the
reasoning of test_parity_full_gpu.py: the control perturbs once, a pipeline rounds at every operation), and the floor is the
tolerance of the existing ONE-step gates (fp32: loss 1e-4, sample rel-L2 1e-3, test_fp32_training_step_vs_reference; bf16: loss 5e-3,
sample rel-L2 0.12, cosine 0.99, the conditioned branch of test_parity_full_gpu.py).  The fp32 one-step gates have no cosine; a rel-L2
error r moves 1 - cos by at most r^2 / 2, so its floor is (1e-3)^2 / 2 = 5e-7.  No sampled tensor is left out of the delta gates.
Set MART_GATES_OUT to a file name to keep the table of measured value / control / gate.
"""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mkgformer_oracle as O  # noqa: E402  (weights regenerated from the golden's seed; the product never imports it)

BASE, NE, NR = 30522, 11292, 192
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORD = "unimo.text_embeddings.word_embeddings.weight"
BIAS = "cls.predictions.bias"
FLOOR = {"fp32": dict(loss=1e-4, rel=1e-3, cos=5e-7), "bf16": dict(loss=5e-3, rel=0.12, cos=1e-2)}
CTL = {"fp32": "ctl32", "bf16": "ctlbf"}
PRECISIONS = ["fp32", "bf16"]


@functools.lru_cache(maxsize=None)
def _gold(tag=""):
    return dict(np.load(os.path.join(GOLD, f"g11_traj{'_' + tag if tag else ''}.npz"), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def _weights(conditioned=True):
    g = _gold()
    sd = O.init_params(O.VisionCfg(patch_size=int(g["patch"])), O.TextCfg(vocab_size=BASE + NE + NR), seed=int(g["weight_seed"]))
    return O.condition_weights(sd) if conditioned else sd


@functools.lru_cache(maxsize=None)
def _batches():
    """The golden's six batches, regenerated from their seeds; integer inputs and pixel checksums are checked against the file."""
    from mkg_analogy_amd import data_synth as D
    g = _gold()
    out = []
    for i, s in enumerate(g["batch_seeds"].tolist()):
        b = D.make_batch(int(g["B"]), int(g["L"]), seed=int(s))
        for k, v in b.items():
            if k != "pixel_values":
                assert np.array_equal(v.numpy(), g[f"in{i}::" + k]), (i, k)
        assert abs(float(b["pixel_values"].double().sum()) - float(g[f"pixel_sum{i}"])) < 1e-6 * float(g[f"pixel_abs_sum{i}"])
        out.append({k: v.cuda() for k, v in b.items()})
    return tuple(out)


def _product(precision, conditioned=True, pretrain=False):
    """tests/test_model_gpu.py:_product with the golden's weights and both dropout probabilities 0."""
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.lit_models import TransformerLitModel
    from mkg_analogy_amd.models import MKGformerKGC, TextConfig, VisionConfig
    torch.manual_seed(0)
    model = MKGformerKGC(VisionConfig(patch_size=int(_gold()["patch"])), TextConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
    cfg = D.data_config(seed=1234)
    args = argparse.Namespace(label_smoothing=0.1, alpha=0.43, pretrain=int(pretrain), lr=5e-5, weight_decay=0.01, optimizer="AdamW", warm_up_radio=0.1)
    lit = TransformerLitModel(model=model, args=args, tokenizer=D.FakeTokenizer(), data_config=cfg)
    missing, unexpected = model.load_state_dict(_weights(conditioned), strict=False)
    assert not unexpected and all(("position_ids" in m or "decoder" in m) for m in missing), (missing, unexpected)
    model.cuda()
    lit._init_relation_word()
    model.finalize()
    model.set_precision(precision)
    return model, lit, cfg


def _sample(t, n=1024):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n].float().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _omc(a, b):
    """1 - cosine."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(1.0 - a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


def _sample_names():
    return [k[4:] for k in _gold() if k.startswith("w0::")]


def _shadow_faults(model):
    """Names of the slots / GEMM groups whose bf16, fp16 or transposed shadow is not the cast of the fp32 master (empty = all fresh)."""
    from mkg_analogy_amd.params import gemm_weight_names
    st = model.store
    bad = []
    if not torch.equal(st.shadow, st.master.to(torch.bfloat16)):
        bad += ["bf16:" + n for n, s in st.slots.items() if not torch.equal(st.w(n), st.m(n).to(torch.bfloat16))] or ["bf16:<padding>"]
    for n in st.slots:
        if st.f16_weight is not None and st.f16_weight(n) and not torch.equal(st.h(n), st.m(n).to(torch.float16)):
            bad.append("fp16:" + n)
    for key, names in gemm_weight_names(model.config.num_hidden_layers):
        if not torch.equal(st.wt(key), st.fused(list(names)).t()):
            bad.append("wt:" + key)
    return bad


def _drive(precision, acc=1, steps=6, poke_after=None, resume_at=None):
    """Six batches through Trainer.train_step; what every test below reads is recorded on the way."""
    from mkg_analogy_amd.trainer import Trainer
    g, batches = _gold(), _batches()
    model, lit, cfg = _product(precision)
    st = model.store
    tr = Trainer(max_epochs=2, accumulate_grad_batches=acc)
    tr._setup(lit, list(batches))
    assert lit.num_training_steps == int(g["num_training_steps" if acc == 1 else "acc2_num_training_steps"])
    assert tr.stream_optimizer and tr.optimizer.fused_zero_grad, "the defaults: MART_STREAM_OPT=1, MART_FUSED_ZERO_GRAD=1"
    names = _sample_names()
    w0 = st.master.detach().clone()
    never = torch.from_numpy(g["never_rows"]).cuda()
    occ = torch.from_numpy(g["word_rows"]).cuda()
    ids = torch.tensor(cfg["analogy_entity_ids"], device="cuda")
    rec = dict(loss=[], lr=[], grad_max=[], shadow_faults=[], same_after_first=None, snaps={}, names=names)

    def delta(n):
        s = st.slots[n]
        sl = slice(s.offset, s.offset + s.numel)
        return (st.master[sl].double() - w0[sl].double()).view(s.shape)

    saved = None
    for i, b in enumerate(batches[:steps]):
        if resume_at is not None and i == resume_at:
            # a fresh product (other initial weights), the model through the LIT model's load_state_dict, the optimizer through its own
            model, lit, cfg = _product(precision, conditioned=False)
            st = model.store
            lit.load_state_dict(saved[0])
            tr = Trainer(max_epochs=2, accumulate_grad_batches=acc)
            tr._setup(lit, list(batches))
            tr.optimizer.load_state_dict(saved[1])
            tr.global_step = saved[2]
            rec["resume_faults"] = _shadow_faults(model)
        if i % acc == 0:
            rec["lr"].append(float(tr.optimizer.param_groups[0]["lr"]))
        loss = tr.train_step(lit, b, i)
        rec["loss"].append(float(loss))
        stepped = (i + 1) % acc == 0
        k = (i + 1) // acc
        if not stepped:
            rec.setdefault("dirty_is_clean", []).append(st.grad_is_clean())
            rec.setdefault("dirty_grad_max", []).append(float(st.grad.abs().max()))
            continue
        rec["grad_max"].append(float(st.grad.abs().max()))              # the WHOLE buffer: dead ranges and padding included
        rec["shadow_faults"].append(_shadow_faults(model))
        if k == 1:
            rec["same_after_first"] = bool(torch.equal(st.master, w0))
        if k in (g["snap"].tolist() if acc == 1 else [3]):
            rec["snaps"][k] = {n: _sample(delta(n).float()) for n in names}
        if poke_after is not None and k == poke_after:
            p = dict(model.named_parameters())["unimo.encoder.vision_layers.5.mlp.fc2.weight"]
            p.grad.add_(0.25)                                           # a write through p.grad between step() and the next zero_grad()
        if resume_at is not None and k == resume_at:
            saved = ({n: v.detach().clone() for n, v in lit.state_dict().items()},
                     {n: (v.detach().clone() if torch.is_tensor(v) else v) for n, v in tr.optimizer.state_dict().items()}, tr.global_step)
            del model, lit, tr, st
            torch.cuda.empty_cache()
    torch.cuda.synchronize()
    dw = delta(WORD)
    rec["wrows"] = dw[occ][:, ::int(g["word_cols"])].float().cpu().numpy()
    rec["wrows_norm"] = dw[occ].norm(dim=1).cpu().numpy()
    rec["never"] = st.m(WORD)[never].detach().cpu().numpy()
    rec["bias_delta"] = delta(BIAS)[ids].float().cpu().numpy()
    rec["dead"] = {n: (bool(torch.equal(st.m(n), w0[st.slots[n].offset:st.slots[n].offset + st.slots[n].numel].view(st.slots[n].shape))),
                       float(st.grad[st.slots[n].offset:st.slots[n].offset + st.slots[n].numel].abs().max())) for n in g["none_grad"].tolist()}
    rec["final_hash"] = float(st.master.double().sum()), float(st.master.double().abs().sum())
    rec["final"] = {n: _sample(st.m(n)) for n in names}
    return rec


@functools.lru_cache(maxsize=None)
def _run(precision, acc=1, variant="main"):
    if variant == "poke":
        return _drive(precision, acc, poke_after=3)
    if variant == "resume":
        return _drive(precision, acc, resume_at=3)
    return _drive(precision, acc)                                       # "main" and "again": two separate runs of the same thing


def _assert_same_run(a, b, precision):
    """Two runs of the same six steps.  The bf16 step has no float atomics on its gradient path (README "determinism"): bit-identical losses
    and weights.  The fp32-accurate step is the verification mode and sums bias / key / value gradients with float atomics by design
    (csrc/precise.hip), so two runs differ by the order of fp32 additions: there the runs must agree to the floors the path is held to against
    the reference (loss 1e-4, delta samples rel-L2 1e-3) -- rounding-level noise sits orders of magnitude below them, a step computed from
    other gradients, moments or weights does not."""
    assert a["lr"] == b["lr"], (a["lr"], b["lr"])
    if precision == "bf16":
        assert a["loss"] == b["loss"] and a["final_hash"] == b["final_hash"], (a["loss"], b["loss"])
        for k in a["snaps"]:
            for n in a["names"]:
                assert np.array_equal(a["snaps"][k][n], b["snaps"][k][n]), (k, n)
        assert all(np.array_equal(a["final"][n], b["final"][n]) for n in a["names"])
        return
    assert a["loss"][:2] == b["loss"][:2], "both losses at the initial weights: no atomics on the forward path"
    worst = max(abs(x - y) for x, y in zip(a["loss"], b["loss"]))
    rels = sorted(((_rel(a["snaps"][k][n], b["snaps"][k][n]), k, n) for k in a["snaps"] for n in a["names"]), reverse=True)
    print(f"\nfp32 path, two runs: max |dloss| {worst:.3e}, worst delta rel-L2 {rels[0][0]:.3e} ({rels[0][2]}, step {rels[0][1]})")
    assert worst <= FLOOR["fp32"]["loss"] and rels[0][0] <= FLOOR["fp32"]["rel"], (worst, rels[:3])


# ----------------------------------------------------------------------------------------------------------------- exact conditions
@pytest.mark.parametrize("precision", PRECISIONS)
def test_schedule_matches_reference_and_first_step_moves_nothing(precision):
    """lr before every step = the reference's (HF linear warm-up over 1.2 steps, then decay over 12) to 1e-12 relative; lr(0) = 0, so after the
    first step every master weight is bit-identical to its initial value (only m and v have moved)."""
    g, r = _gold(), _run(precision)
    assert len(r["lr"]) == 6
    for got, ref in zip(r["lr"], g["lr"].tolist()):
        assert abs(got - ref) <= 1e-12 * abs(ref), (r["lr"], g["lr"])
    assert r["lr"][0] == 0.0 and r["same_after_first"] is True


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dead_tensors_are_never_touched(precision):
    """Tensors whose gradient is None in the reference (torch.optim skips them: no update, NO weight decay) are bit-identical to their initial
    values after six steps and their gradient range is exactly zero."""
    r = _run(precision)
    assert len(r["dead"]) == 20
    moved = [n for n, (same, gmax) in r["dead"].items() if not same]
    dirty = [n for n, (same, gmax) in r["dead"].items() if gmax != 0.0]
    assert not moved and not dirty, (moved, dirty)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_unused_word_rows_shrink_by_weight_decay_only(precision):
    """Word-embedding rows that never occur and are not scored have a ZERO gradient in the reference (not None): m = v = 0, the Adam term is
    0 / (0 + eps) = 0, and the row becomes w0 * prod_k (1 - lr_k * 0.01).  Bound: per step the factor is rounded to fp32 (2^-24 relative) and
    the product is rounded again (2^-24), so <= 2^-23 |w| per step, 6 steps: |w - closed form| <= 6 * 2^-23 * |w0|; the same bound against
    the reference's own rows (torch's p.mul_(1 - lr * wd): the same two roundings)."""
    g, r = _gold(), _run(precision)
    w0 = g["never0"].astype(np.float64)
    f = np.prod([1.0 - lr * 0.01 for lr in g["lr"].tolist()])
    bound = 6 * 2.0 ** -23 * np.abs(w0)
    got = r["never"].astype(np.float64)
    assert f < 1.0 and np.all(np.abs(got - w0 * f) <= bound), float((np.abs(got - w0 * f) / (np.abs(w0) + 1e-30)).max())
    c = int(g["never_cols"])
    ref = _gold("main")["never::w6"].astype(np.float64)
    assert np.all(np.abs(got[:, ::c] - ref) <= bound[:, ::c])
    assert np.all(np.abs(ref - (w0 * f)[:, ::c]) <= bound[:, ::c])     # (the golden itself obeys the closed form)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("acc", [1, 2])
def test_gradient_buffer_is_zero_after_every_step(precision, acc):
    """Fused zeroing: after every stepping train_step the WHOLE gradient buffer is zero -- dead ranges and padding included, which the update
    kernel never visits although step() then calls the buffer clean.  A micro-batch that does not step leaves it dirty and says so."""
    r = _run(precision, acc)
    assert len(r["grad_max"]) == 6 // acc and all(x == 0.0 for x in r["grad_max"]), r["grad_max"]
    if acc == 2:
        assert r["dirty_is_clean"] == [False] * 3 and all(x > 0 for x in r["dirty_grad_max"]), (r["dirty_is_clean"], r["dirty_grad_max"])


def test_gradient_buffer_is_zero_with_run_mode_dead_tensors():
    """Pre-training without sep_idx: the adaptive weights are dead too (``extra_dead``, lit_models/transformer.py) -- outside the chunk table, so
    never zeroed by the update; their gradient range must stay zero all the same, and they must not move."""
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.trainer import Trainer
    model, lit, cfg = _product("bf16", pretrain=True)
    st = model.store
    bs = [D.make_batch(2, 96, seed=s, pretrain=True, device="cuda") for s in (31, 32, 33)]
    tr = Trainer(max_epochs=2)                                           # six training steps planned: lr(3) > 0
    tr._setup(lit, bs)
    aw = [n for n in st.slots if "adaptive_weight" in n]
    before = {n: st.m(n).clone() for n in aw}
    for i, b in enumerate(bs):
        tr.train_step(lit, b, i)
        assert float(st.grad.abs().max()) == 0.0, i
    assert len(aw) == 24 and all(torch.equal(st.m(n), before[n]) for n in aw)
    assert tr.optimizer.param_groups[0]["lr"] > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("acc", [1, 2])
def test_every_shadow_is_the_cast_of_its_master_after_every_step(precision, acc):
    """After every update: the bf16 shadow of the whole buffer, the fp16 shadow of every selected slot and W^T of every GEMM group."""
    r = _run(precision, acc)
    assert len(r["shadow_faults"]) == 6 // acc and not any(r["shadow_faults"]), [f[:5] for f in r["shadow_faults"]]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_runs_are_bit_identical(precision):
    """The project's run-to-run bit identity of a bf16 step, extended to six steps with the optimizer in between (see _assert_same_run for
    the fp32-accurate path, which uses float atomics)."""
    a, b = _run(precision), _run(precision, 1, "again")
    assert a is not b
    _assert_same_run(a, b, precision)


# ----------------------------------------------------------------------------------------------------------------- staleness probes
@pytest.mark.parametrize("precision", PRECISIONS)
def test_write_through_p_grad_between_steps_is_zeroed(precision):
    """torch semantics: whatever is written to ``p.grad`` after ``step()`` is gone after the next ``zero_grad()``.  With fused zeroing
    ``zero_grad()`` is skipped on the strength of FlatStore.grad_clean; a write through a ``p.grad`` view must revoke that."""
    a, b = _run(precision), _run(precision, 1, "poke")
    assert all(x == 0.0 for x in b["grad_max"]), b["grad_max"]
    _assert_same_run(a, b, precision)
    rows, bad = _gates(precision, 1, b)                                  # and, like the undisturbed run, inside the reference's gates
    assert [w for w, *_ in bad] == [w for w, *_ in _gates(precision, 1)[1]], bad[:5]


def test_micro_batches_accumulate_and_a_dirty_window_is_zeroed():
    """accumulate_grad_batches with fused zeroing: a micro-batch that does not step ADDS to the buffer (g(b0) then g(b1) on top = g(b0) + g(b1)
    to fp32 rounding: rel-L2 1e-5 allows ~100 roundings of 2^-24, a missing accumulation is an error of order 1), and ``zero_grad()`` does
    not skip a buffer that an unfinished window left dirty."""
    from mkg_analogy_amd.trainer import Trainer
    batches = _batches()
    model, lit, cfg = _product("bf16")
    st = model.store
    tr = Trainer(max_epochs=2, accumulate_grad_batches=3)
    tr._setup(lit, list(batches))
    tr.train_step(lit, batches[0], 0)
    g0 = st.grad.clone()
    tr.train_step(lit, batches[1], 1)
    g01 = st.grad.clone()
    assert float(g0.abs().max()) > 0 and not st.grad_is_clean()
    tr.train_step(lit, batches[1], 0)                                   # a new window begins although the last one never stepped
    g1 = st.grad.clone()
    err = float((g01.double() - (g0.double() + g1.double())).norm() / g01.double().norm())
    print(f"\naccumulated vs summed gradients: rel-L2 {err:.3e}")
    assert err < 1e-5
    assert not torch.equal(g1, g01)
    tr.optimizer.zero_grad()
    assert float(st.grad.abs().max()) == 0.0 and st.grad_is_clean()


# ----------------------------------------------------------------------------------------------------------------- measured conditions
def _gates(precision, acc, r=None):
    """(rows of the table, failures).  A row: quantity, measured, control, gate, measured / gate."""
    g, r = _gold(), (_run(precision, acc) if r is None else r)
    fl, ctl = FLOOR[precision], CTL[precision]
    rows, bad = [], []

    def add(what, got, c, mult, floor):
        gate = mult * c + floor
        rows.append((what, got, c, gate, got / gate))
        if not got <= gate:
            bad.append(rows[-1])

    pre = "" if acc == 1 else "acc2::"
    for i, (got, ref, c) in enumerate(zip(r["loss"], g[pre + "loss"].tolist(), g[ctl + "::" + pre + "loss"].tolist())):
        add(f"loss step {i}", abs(got - ref), abs(c - ref), 8, fl["loss"])
    if acc == 1:
        ref_f, ctl_f, dk = _gold("main"), _gold(ctl), lambda k, n: f"d{k}::{n}"
        ctl_key = dk
    else:
        ref_f = ctl_f = _gold("acc2")
        dk, ctl_key = (lambda k, n: f"d{k}::{n}"), (lambda k, n: f"{ctl}::d{k}::{n}")
    for k, snap in sorted(r["snaps"].items()):
        aw = [n for n in r["names"] if "adaptive_weight" in n]          # scalars: compared as ONE vector, as the gradient gates do
        groups = [(n, [n]) for n in r["names"] if n not in aw] + [("adaptive weights (vector)", aw)]
        for label, ns in groups:
            got = np.concatenate([snap[n].ravel() for n in ns])
            ref = np.concatenate([ref_f[dk(k, n)].ravel() for n in ns])
            c = np.concatenate([ctl_f[ctl_key(k, n)].ravel() for n in ns])
            assert np.linalg.norm(ref) >= 1e-9, (label, k)              # the cap: nothing is excluded, and nothing needs to be
            add(f"step {k} rel-L2 {label}", _rel(got, ref), _rel(c, ref), 4, fl["rel"])
            if len(got) > 1:
                add(f"step {k} 1-cos  {label}", _omc(got, ref), max(0.0, _omc(c, ref)), 4, fl["cos"])
    kl = max(r["snaps"])
    cf = _gold(ctl if acc == 1 else "acc2")
    cpre = "" if acc == 1 else ctl + "::"
    add(f"step {kl} rel-L2 word-embedding rows that occur (per-row delta norms)", _rel(r["wrows_norm"], ref_f[f"wrows_norm::d{kl}"]),
        _rel(cf[cpre + f"wrows_norm::d{kl}"], ref_f[f"wrows_norm::d{kl}"]), 4, fl["rel"])
    add(f"step {kl} rel-L2 word-embedding rows that occur (every 48th column)", _rel(r["wrows"], ref_f[f"wrows::d{kl}"]),
        _rel(cf[cpre + f"wrows::d{kl}"], ref_f[f"wrows::d{kl}"]), 4, fl["rel"])
    add(f"step {kl} rel-L2 scored slice of cls.predictions.bias", _rel(r["bias_delta"], ref_f[f"bias::d{kl}"]),
        _rel(cf[cpre + f"bias::d{kl}"], ref_f[f"bias::d{kl}"]), 4, fl["rel"])
    return rows, bad


def _report(title, rows, bad):
    lines = [f"# {title}", f"# {'quantity':<100} {'measured':>10} {'control':>10} {'gate':>10} {'meas/gate':>9}"]
    lines += [f"{w:<102} {m:10.3e} {c:10.3e} {gt:10.3e} {q:9.3f}" for w, m, c, gt, q in rows]
    worst = sorted(rows, key=lambda x: -x[4])[:5]
    lines += ["# closest to their gates: " + "; ".join(f"{w} ({q:.2f})" for w, *_, q in worst), ""]
    text = "\n".join(lines)
    print("\n" + "\n".join(lines[:2] + [l for l, row in zip(lines[2:], rows) if row[4] > 0.5 or row in worst] + lines[-2:]))
    out = os.environ.get("MART_GATES_OUT")
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")
    assert not bad, [(w, f"{m:.3e} > {gt:.3e}") for w, m, c, gt, q in bad][:8]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_trajectory_vs_reference(precision):
    """Per-step loss, and rel-L2 / 1 - cos of the sampled weight deltas after steps 2, 4, 6, against the reference (see the module docstring for
    the gates).  Measured on MI355X (profiles/r08_trajectory_gates.txt has every row)."""
    rows, bad = _gates(precision, 1)
    _report(f"six steps, {precision} path, control {CTL[precision]}", rows, bad)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_accumulated_trajectory_vs_reference(precision):
    """The same six batches as three optimizer steps of two micro-batches (accumulate_grad_batches = 2) against the reference's ``acc2`` run."""
    g, r = _gold(), _run(precision, 2)
    for got, ref in zip(r["lr"], g["acc2::lr"].tolist()):
        assert abs(got - ref) <= 1e-12 * abs(ref), (r["lr"], g["acc2::lr"])
    assert r["same_after_first"] is True
    rows, bad = _gates(precision, 2)
    _report(f"three steps of two micro-batches, {precision} path, control {CTL[precision]}", rows, bad)


# ----------------------------------------------------------------------------------------------------------------- save / resume
@pytest.mark.parametrize("precision", PRECISIONS)
def test_resume_after_three_steps_is_bit_identical(precision):
    """Three steps, ``lit.state_dict()`` + the optimizer's state (moments, step count, schedule), a FRESH product with other weights, the model
    loaded through the lit model, three more steps: the same as the uninterrupted run (bit for bit on the bf16 path, _assert_same_run), inside
    the reference's gates, and every shadow is fresh right after the load."""
    a, b = _run(precision), _run(precision, 1, "resume")
    assert b["resume_faults"] == []
    _assert_same_run(a, b, precision)
    rows, bad = _gates(precision, 1, b)                                  # inside the reference's gates wherever the uninterrupted run is
    assert [w for w, *_ in bad] == [w for w, *_ in _gates(precision, 1)[1]], bad[:5]


def test_optimizer_state_of_another_layout_is_refused():
    """FusedAdamW's state is flat m / v: without the layout it was written for it loads, silently, onto other parameters."""
    from mkg_analogy_amd.trainer import Trainer
    model, lit, cfg = _product("bf16")
    tr = Trainer(max_epochs=2)
    tr._setup(lit, list(_batches()))
    tr.train_step(lit, _batches()[0], 0)
    sd = tr.optimizer.state_dict()
    assert [e[0] for e in sd["layout"]] == list(model.store.slots) and sd["scheduler"] == {"last_epoch": 1} and sd["steps"] == 1
    tr.optimizer.load_state_dict(sd)                                     # its own state passes
    swapped = dict(sd)
    swapped["layout"] = list(sd["layout"])
    swapped["layout"][3], swapped["layout"][40] = swapped["layout"][40], swapped["layout"][3]
    with pytest.raises(ValueError, match="another parameter layout"):
        tr.optimizer.load_state_dict(swapped)
    with pytest.raises(ValueError, match="no parameter layout"):
        tr.optimizer.load_state_dict({k: v for k, v in sd.items() if k != "layout"})
    assert tr.optimizer.steps == 1
