"""Gradient clipping and gradient-norm tracking on the GPU (include/mart_clip.h, optim.GradClip, Trainer(gradient_clip_val=..., track_grad_norm=...)).

Kernel level: synthetic flat buffers with hand-made chunk tables, against torch on the same device tensor.  Every accumulation of the norm kernels is
in float64, so the gate needs no measured tolerance: the fp32 result equals ``float32(sqrt(sum(g.double() ** 2)))`` or is its neighbour (1 ulp: the two
float64 sums differ in their last bits, which can only move the final rounding to fp32 across one boundary); the inf-norm is exact; the clip
coefficient, the scaled gradients and the clamped gradients are compared with torch's fp32 expressions bit for bit.

Model level: the MKGformer step (B = 4, L = 57, 49 patches) through the Trainer, against a torch restatement built from the very gradients the
step's clip saw (snapshotted at ``optimizer.step()``): ``torch.nn.utils.clip_grad_norm_`` / ``clip_grad_value_`` and ``torch.optim`` on cloned masters.
The masters are held to the tolerance of the AdamW-vs-torch.optim.AdamW kernel test (tests/test_kernels_gpu.py: 1e-6 absolute + 1e-6 relative).
The first Adam step is nearly invariant under a rescaling of the gradients, so the first moment (0.1 x the clipped gradient) is compared as
well: within 1e-5 relative -- torch's own fp32 norm, which sets its coefficient, carries up to ~1e-6 relative, and the kernel forms 1 - beta1 in
fp32 (2.4e-7) -- against a factor of two if the clip had not been applied.
"""
import argparse
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I32 = torch.float32, torch.float64, torch.int32
ZERO_ONLY = 4
VISION = ("unimo.vision_", "unimo.encoder.vision_layers.")


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mkg_analogy_amd import ops as o
    o.require_gpu()
    return o


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """The module shares one model, its first weights and a few recorded runs (several GB): nothing of it outlives the module -- tests that come later in
    the same process measure the allocator (tests/test_model_gpu.py) and must find it as a fresh process would."""
    yield
    import gc
    for cached in (_mkg, _small, _plain_unstreamed, _first_norm):
        cached.cache_clear()
    gc.collect()                                                        # (trainer <-> lit model, wrapped step() closures: reference cycles)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _bits(t):
    return t.contiguous().view(I32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ulps(a, b):
    """Distance in representable fp32 values between two finite fp32 scalars of the same sign."""
    return abs(int(_bits(a.reshape(1)).item()) - int(_bits(b.reshape(1)).item()))


# ------------------------------------------------------------------------------------------------ kernel level
def _table(lengths, first_starts=(0, 3), zero_only_after=None, seed=0, scale=1.0):
    """A flat buffer and a chunk table: chunk i has ``lengths[i]`` elements; the first chunks start at ``first_starts``, the later ones at a running
    ODD offset (every gap is 1 or 2 elements wide).  Gaps and the tail hold NaN; ``zero_only_after``: a ZERO_ONLY chunk of 70 elements filled
    with 1e30 is inserted after that many live chunks.  Returns (buffer, int32 table on the device, bool mask of the live elements)."""
    rows, pos = [], 0
    for i, n in enumerate(lengths):
        if zero_only_after is not None and i == zero_only_after:
            pos += 1 + (pos % 2)
            rows.append([pos, 70, ZERO_ONLY | 1])
            pos += 70
        start = first_starts[i] if i < len(first_starts) else pos + 1 + (pos % 2)      # odd
        assert start >= pos and (i < len(first_starts) or start % 2 == 1)
        rows.append([start, n, i % 4 if i % 4 != 0 else 1])            # flag bits 0 / 1 mean nothing to these kernels
        pos = start + n
    total = pos + 37
    gen = torch.Generator(device="cuda").manual_seed(seed)
    buf = torch.full((total,), float("nan"), device="cuda", dtype=F32)
    live = torch.zeros(total, dtype=torch.bool, device="cuda")
    for s, n, f in rows:
        if f & ZERO_ONLY:
            buf[s:s + n] = 1e30
        else:
            buf[s:s + n] = torch.randn(n, device="cuda", generator=gen) * scale
            live[s:s + n] = True
    return buf, torch.tensor(rows, dtype=I32, device="cuda"), live


def _norm(ops, buf, table, mode, grad_scale=1.0, max_norm=0.0, log=None, log_index=0, extra_partials=0):
    n = int(table.shape[0])
    partials = torch.full((ops.clip_partials_needed(n) + extra_partials,), -7.0, device="cuda", dtype=F64)
    out = torch.full((2,), -7.0, device="cuda", dtype=F32)
    ops.clip_sumsq(buf, table, n, mode, partials)
    ops.clip_finalize(partials, mode, out, grad_scale=grad_scale, max_norm=max_norm, log=log, log_index=log_index)
    return partials, out


def _torch_coef(total, max_norm):
    return torch.clamp(max_norm / (total + 1e-6), max=1.0)            # torch.nn.utils.clip_grad_norm_, on an fp32 device scalar


LENGTHS = [1, 2, 3, 5, 63, 64, 65, 65535, 65536]


@functools.lru_cache(maxsize=None)
def _small():
    return _table(LENGTHS, zero_only_after=4, seed=1)


def test_two_norm_of_the_live_chunks_is_within_one_ulp_of_the_double_reference(ops):
    buf, table, live = _small()
    assert int(table[0, 0]) == 0 and int(table[1, 0]) == 3 and all(int(s) % 2 == 1 for s in table[2:, 0]) and int((table[:, 2] & ZERO_ONLY != 0).sum()) == 1
    before = buf.clone()
    ref = buf[live].double().pow(2).sum().sqrt().float()
    partials, out = _norm(ops, buf, table, 0)
    print(f"\n2-norm {float(out[0]):.9g} reference {float(ref):.9g} ({_ulps(out[0], ref)} ulp)")
    assert torch.isfinite(out[0]) and _ulps(out[0], ref) <= 1           # neither the NaN gaps nor the 1e30 frozen chunk reached it
    assert float(out[1]) == 1.0                                          # max_norm <= 0: track only
    assert _same_bits(buf, before)
    zrow = int((table[:, 2] & ZERO_ONLY != 0).nonzero()[0])
    assert float(partials[8 * zrow:8 * zrow + 8].abs().max()) == 0.0     # the skipped chunk's work items own their slots and write 0
    # per-chunk partial sums against torch, chunk by chunk: both are float64 sums of positive terms in which no value passes through more than
    # ~50 additions (32 per lane, then trees), so each is within 50 x 2^-53 = 6e-15 relative of the exact sum
    for ci, (s, n, f) in enumerate(table.tolist()):
        if not f & ZERO_ONLY:
            got, want = float(partials[8 * ci:8 * ci + 8].sum()), float(buf[s:s + n].double().pow(2).sum())
            assert abs(got - want) <= 1e-13 * want, (ci, got, want)


def test_inf_norm_is_exact_and_scaled(ops):
    buf, table, live = _small()
    ref = buf[live].abs().max()
    _, out = _norm(ops, buf, table, 1)
    assert _same_bits(out[:1], ref.reshape(1))
    _, out = _norm(ops, buf, table, 1, grad_scale=0.125)
    assert _same_bits(out[:1], (ref * 0.125).reshape(1))
    ref2 = (buf[live].double().pow(2).sum().sqrt() * 0.125).float()
    _, out = _norm(ops, buf, table, 0, grad_scale=0.125)
    assert _ulps(out[0], ref2) <= 1


def test_coefficient_is_torchs_fp32_expression_bit_for_bit(ops):
    buf, table, live = _small()
    _, base = _norm(ops, buf, table, 0)
    total = float(base[0])
    for max_norm in (0.5 * total, total / 3.0, 1e-3, 0.999999 * total, total, 1.000001 * total, 2.0 * total, 1e30):
        _, out = _norm(ops, buf, table, 0, max_norm=max_norm)
        assert _same_bits(out[:1], base[:1])
        assert _same_bits(out[1:], _torch_coef(out[0], max_norm).reshape(1)), max_norm
    _, out = _norm(ops, buf, table, 0, max_norm=0.5 * total)
    assert 0.49 < float(out[1]) < 0.51
    log = torch.zeros(5, device="cuda")
    _, out = _norm(ops, buf, table, 0, log=log, log_index=3)
    assert log.tolist() == [0.0, 0.0, 0.0, float(out[0]), 0.0]


def test_partials_beyond_the_needed_ones_are_zeroed_and_runs_are_bit_identical(ops):
    buf, table, live = _small()
    p1, o1 = _norm(ops, buf, table, 0, max_norm=1.0)
    p2, o2 = _norm(ops, buf, table, 0, max_norm=1.0)
    assert _same_bits(p1.view(F32), p2.view(F32)) and _same_bits(o1, o2)
    p3, o3 = _norm(ops, buf, table, 0, max_norm=1.0, extra_partials=300)       # a caller whose buffer is larger than needed
    assert float(p3[p1.numel():].abs().max()) == 0.0 and _same_bits(p3[:p1.numel()].view(F32), p1.view(F32)) and _same_bits(o3, o1)
    q1, r1 = _norm(ops, buf, table, 1, max_norm=1.0)
    q2, r2 = _norm(ops, buf, table, 1, max_norm=1.0)
    assert _same_bits(q1.view(F32), q2.view(F32)) and _same_bits(r1, r2)


def test_apply_scales_live_chunks_only_and_skips_the_pass_when_the_clip_does_not_trigger(ops):
    buf, table, live = _small()
    n = int(table.shape[0])
    total = float(_norm(ops, buf, table, 0)[1][0])
    _, out = _norm(ops, buf, table, 0, max_norm=0.25 * total)
    assert float(out[1]) < 1.0
    g = buf.clone()
    ops.clip_apply(g, table, n, coef=out[1:])
    assert _same_bits(g[live], buf[live] * out[1])                      # torch's fp32 product
    assert _same_bits(g[~live], buf[~live])                             # NaN gaps, tail and the 1e30 frozen chunk: bit-unchanged
    # total <= max_norm: coef is exactly 1 and the whole buffer keeps its bits
    _, out = _norm(ops, buf, table, 0, max_norm=2.0 * float(out[0]))
    assert float(out[1]) == 1.0
    g = buf.clone()
    ops.clip_apply(g, table, n, coef=out[1:])
    assert _same_bits(g, buf)


def test_apply_by_value_is_torch_clamp(ops):
    buf, table, live = _small()
    n = int(table.shape[0])
    buf = buf.clone()
    first = int(live.nonzero()[5])
    buf[first] = float("nan")                                           # a NaN inside a live chunk stays NaN, as torch.clamp
    buf[int(live.nonzero()[6])] = -0.0
    for v in (0.5, 1e-3, 3.0):
        g = buf.clone()
        ops.clip_apply(g, table, n, clip_value=v)
        assert _same_bits(g[live], torch.clamp(buf[live], -v, v)) and _same_bits(g[~live], buf[~live]), v
        assert bool(torch.isnan(g[first]))


def test_more_work_items_than_one_grid_sweep(ops):
    """600 chunks of 65536 elements at odd starts: 4800 work items for a grid of 2048 workgroups."""
    buf, table, live = _table([65536] * 600, first_starts=(), zero_only_after=300, seed=3)
    n = int(table.shape[0])
    assert n == 601 and ops.clip_partials_needed(n) == 4808
    ref = buf[live].double().pow(2).sum().sqrt().float()
    _, out = _norm(ops, buf, table, 0, max_norm=100.0)
    assert _ulps(out[0], ref) <= 1 and _same_bits(out[1:], _torch_coef(out[0], 100.0).reshape(1)) and float(out[1]) < 1.0
    _, oi = _norm(ops, buf, table, 1)
    assert _same_bits(oi[:1], buf[live].abs().max().reshape(1))
    g = buf.clone()
    ops.clip_apply(g, table, n, coef=out[1:])
    assert _same_bits(g[live], buf[live] * out[1]) and _same_bits(g[~live], buf[~live])
    ops.clip_apply(g, table, n, clip_value=0.01)
    assert _same_bits(g[live], torch.clamp(buf[live] * out[1], -0.01, 0.01)) and _same_bits(g[~live], buf[~live])


@pytest.mark.parametrize("value", [1e20, 1e-30])
def test_huge_and_tiny_entries_neither_overflow_nor_vanish(ops, value):
    n = 70001
    buf = torch.full((n + 8,), value, device="cuda", dtype=F32)
    table = torch.tensor([[3, n, 1]], dtype=I32, device="cuda")
    ref = buf[3:3 + n].double().pow(2).sum().sqrt().float()
    _, out = _norm(ops, buf, table, 0, max_norm=1.0)
    assert torch.isfinite(out[0]) and float(out[0]) > 0 and _ulps(out[0], ref) <= 1
    assert _same_bits(out[1:], _torch_coef(out[0], 1.0).reshape(1))
    _, oi = _norm(ops, buf, table, 1)
    assert _same_bits(oi[:1], buf[3:4])


def test_a_nan_entry_poisons_norm_coefficient_and_gradients_as_in_torch(ops):
    buf, table, live = _table([5, 64, 4097], first_starts=(), seed=5)
    n = int(table.shape[0])
    buf[int(table[2, 0]) + 4000] = float("nan")
    for mode in (0, 1):
        _, out = _norm(ops, buf, table, mode, max_norm=1.0)
        assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[1])), mode
    g = buf.clone()
    ops.clip_apply(g, table, n, coef=out[1:])
    assert bool(torch.isnan(g[live]).all()) and _same_bits(g[~live], buf[~live])
    p = torch.nn.Parameter(torch.zeros(int(live.sum()), device="cuda"))
    p.grad = buf[live].clone()
    assert bool(torch.isnan(torch.nn.utils.clip_grad_norm_([p], 1.0))) and bool(torch.isnan(p.grad).all())      # torch does the same


def test_functional_wrappers_on_a_bare_store(ops):
    """Fn.grad_norm / Fn.clip_grad_norm_ / Fn.clip_grad_value_ take a model (``.store``) or the store itself; all they read is grad, chunks, n_chunks."""
    import types
    from mkg_analogy_amd import functional as Fn
    buf, table, live = _small()
    store = types.SimpleNamespace(grad=buf.clone(), chunks=table, n_chunks=int(table.shape[0]))
    model = types.SimpleNamespace(store=store)
    ref = buf[live].double().pow(2).sum().sqrt()
    assert _ulps(Fn.grad_norm(store), ref.float()) <= 1 and _ulps(Fn.grad_norm(model, 2, grad_scale=0.25), (ref * 0.25).float()) <= 1
    assert _same_bits(Fn.grad_norm(model, "inf").reshape(1), buf[live].abs().max().reshape(1))
    assert _same_bits(store.grad, buf)
    total = Fn.clip_grad_norm_(model, 2.0 * float(ref))                 # does not trigger: returns the norm, touches nothing
    assert _ulps(total, ref.float()) <= 1 and _same_bits(store.grad, buf)
    total = Fn.clip_grad_norm_(model, 0.125 * float(ref), grad_scale=0.5)      # the norm of 0.5 g is 0.5 |g|: coef ~ 0.25
    assert _ulps(total, (ref * 0.5).float()) <= 1
    coef = _torch_coef(total, 0.125 * float(ref))
    assert 0.24 < float(coef) < 0.26 and _same_bits(store.grad[live], buf[live] * coef) and _same_bits(store.grad[~live], buf[~live])
    store.grad = buf.clone()
    Fn.clip_grad_value_(store, 0.5, grad_scale=0.25)                    # clamp(0.25 g, +-0.5) = 0.25 clamp(g, +-2)
    assert _same_bits(store.grad[live], torch.clamp(buf[live], -2.0, 2.0)) and _same_bits(store.grad[~live], buf[~live])
    inf = Fn.clip_grad_norm_(store, 1.0, norm_type="inf")
    assert _same_bits(inf.reshape(1), torch.clamp(buf[live], -2.0, 2.0).abs().max().reshape(1)) and float(store.grad[live].abs().max()) <= 1.0


# ------------------------------------------------------------------------------------------------ model level
@functools.lru_cache(maxsize=None)
def _mkg():
    """One MKGformer (12 layers, H = 768, patch 32: 49 patches per image) for the whole module; ``_fresh`` puts it back to its first state."""
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.lit_models import TransformerLitModel
    from mkg_analogy_amd.models import MKGformerKGC, TextConfig, VisionConfig
    torch.manual_seed(0)
    model = MKGformerKGC(VisionConfig(patch_size=32), TextConfig())
    cfg = D.data_config(seed=1234)
    args = argparse.Namespace(label_smoothing=0.1, alpha=0.43, pretrain=0, lr=5e-5, weight_decay=0.01, optimizer="AdamW", warm_up_radio=0.0)
    lit = TransformerLitModel(model=model, args=args, tokenizer=D.FakeTokenizer(), data_config=cfg)
    model.cuda()
    lit._init_relation_word()
    D.load_seeded_weights(model, lit, seed=3, conditioned=True)
    model.finalize()
    batches = tuple(D.make_batch(4, 57, seed=100 + i, device="cuda") for i in range(4))
    return model, lit, model.store.master.detach().clone(), batches


def _fresh(precision="bf16", optimizer="AdamW", freeze=()):
    model, lit, w0, batches = _mkg()
    st = model.store
    model.set_precision(precision)
    model.unfreeze()
    if freeze:
        model.freeze(*freeze)
    model.sync_trainable()
    with torch.no_grad():
        st.master.copy_(w0)
    st.refresh_shadows()
    st.zero_grad()
    model._step = 0                                                     # the dropout seed is a function of base_seed and this counter alone
    model.engine.grad_ready = model.engine.grad_ready_async = None
    lit.optimizer_name = optimizer
    return model, lit, batches


def _run(steps=1, precision="bf16", optimizer="AdamW", freeze=(), acc=1, env=None, **trainer_kw):
    """``steps`` train_steps on the fresh model.  Returns the final masters, the gradient buffer as each optimizer step found it, the per-step
    (norm, coef) device scalars, max |grad| after each optimizer step, the optimizer and the trainer."""
    from mkg_analogy_amd.trainer import Trainer
    model, lit, batches = _fresh(precision, optimizer, freeze)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        tr = Trainer(max_epochs=1, accumulate_grad_batches=acc, world_size=1, **trainer_kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    tr._setup(lit, list(batches[:steps]) * 2)
    st, opt = model.store, tr.optimizer
    rec = dict(snaps=[], norms=[], coefs=[], grad_max=[], grad_scale=opt.grad_scale, tr=tr, opt=opt, store=st, lr=opt.param_groups[0]["lr"])
    inner = opt.step

    def step(*a, **k):
        rec["snaps"].append(st.grad.detach().clone())
        out = inner(*a, **k)
        rec["norms"].append(None if opt.last_grad_norm is None else opt.last_grad_norm.clone())
        rec["coefs"].append(None if opt.last_clip_coef is None else opt.last_clip_coef.clone())
        rec["grad_max"].append(float(st.grad.abs().max()))
        return out
    opt.step = step
    for i in range(steps):
        tr.train_step(lit, batches[i], i)
    torch.cuda.synchronize()
    rec["master"] = st.master.detach().clone()
    rec["trainable"] = list(st.trainable_names())
    rec["slots"] = {n: (s.offset, s.numel) for n, s in st.slots.items()}
    model.engine.grad_ready = model.engine.grad_ready_async = None
    return rec


def _slices(rec, buf, names=None):
    return [buf[o:o + k] for o, k in (rec["slots"][n] for n in (names or rec["trainable"]))]


def _double_norm(rec, snap, inf=False):
    """The norm of grad_scale x the gradients of the trainable tensors, accumulated in float64, rounded to fp32 once."""
    parts = _slices(rec, snap)
    if inf:
        return (torch.stack([p.abs().max() for p in parts]).max().double() * rec["grad_scale"]).float()
    return (torch.stack([p.double().pow(2).sum() for p in parts]).sum().sqrt() * rec["grad_scale"]).float()


def _restate(rec, clip_val, algorithm="norm", optimizer="AdamW"):
    """torch on clones: the trainable gradients the step saw x grad_scale, torch's clipping, torch's optimizer with the lit model's two weight-decay
    groups on clones of the initial masters.  Returns (masters, first moments, the norm torch returned) per trainable tensor."""
    from mkg_analogy_amd.params import NO_DECAY
    w0 = _mkg()[2]
    names = rec["trainable"]
    params = [torch.nn.Parameter(w.clone()) for w in _slices(rec, w0)]
    for p, g in zip(params, _slices(rec, rec["snaps"][0])):
        p.grad = g.clone() * rec["grad_scale"]
    norm = None
    if algorithm == "norm":
        norm = torch.nn.utils.clip_grad_norm_(params, clip_val)
    else:
        torch.nn.utils.clip_grad_value_(params, clip_val)
    decay = [p for n, p in zip(names, params) if not any(nd in n for nd in NO_DECAY)]
    no_decay = [p for n, p in zip(names, params) if any(nd in n for nd in NO_DECAY)]
    opt = getattr(torch.optim, optimizer)([{"params": decay, "weight_decay": 0.01}, {"params": no_decay, "weight_decay": 0}], lr=rec["lr"], eps=1e-8)
    opt.step()
    return [p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], norm


def _check_against_restatement(rec, clip_val, algorithm="norm", optimizer="AdamW", m_of=None):
    masters, moments, norm = _restate(rec, clip_val, algorithm, optimizer)
    got = _slices(rec, rec["master"])
    w0 = _slices(rec, _mkg()[2])
    worst, moved = 0.0, 0
    for n, a, b, w in zip(rec["trainable"], got, masters, w0):
        err = (a - b).abs()
        tol = 1e-6 + 1e-6 * b.abs()
        worst = max(worst, float((err / tol).max()))
        moved += int((a != w).sum())
    assert worst <= 1.0 and moved > 0, (worst, moved)
    if m_of is not None:
        mw = 0.0
        for a, b in zip(m_of, moments):
            mw = max(mw, float(((a - b).abs() / (1e-5 * b.abs() + 1e-30)).max()))
        assert mw <= 1.0, mw
    return norm


@functools.lru_cache(maxsize=None)
def _plain_unstreamed(steps=3):
    """The schedule clipping forces, without clipping: MART_STREAM_OPT=0."""
    rec = _run(steps, env={"MART_STREAM_OPT": "0"})
    assert not rec["tr"].stream_optimizer and rec["opt"]._clip is None
    return rec["master"]


@functools.lru_cache(maxsize=None)
def _first_norm():
    rec = _run(1, track_grad_norm=2)
    ref = _double_norm(rec, rec["snaps"][0])
    assert _ulps(rec["norms"][0], ref) <= 1 and float(rec["coefs"][0] if rec["coefs"][0] is not None else 1.0) == 1.0
    return float(rec["norms"][0]), rec["master"]


def test_defaults_are_the_parents_step_bit_for_bit():
    a = _run(3)
    assert a["tr"].stream_optimizer and a["opt"]._clip is None and a["norms"] == [None] * 3
    b = _run(3, gradient_clip_val=None, gradient_clip_algorithm="norm", track_grad_norm=None)
    assert b["tr"].stream_optimizer and _same_bits(a["master"], b["master"])
    assert not _same_bits(a["master"], _mkg()[2])


def test_a_clip_that_never_triggers_is_a_no_op_on_the_weights():
    c = _run(3, gradient_clip_val=1e30)
    assert not c["tr"].stream_optimizer and all(float(x) == 1.0 for x in c["coefs"]) and all(float(x) > 0 for x in c["norms"])
    assert _same_bits(c["master"], _plain_unstreamed())
    assert c["grad_max"] == [0.0] * 3                                   # the fused_zero_grad invariant holds with the clip in front of the update


def test_a_triggering_clip_against_torch():
    norm0, _ = _first_norm()
    clip = 0.5 * norm0
    rec = _run(1, gradient_clip_val=clip)
    st, opt = rec["store"], rec["opt"]
    assert 0.49 < float(rec["coefs"][0]) < 0.51
    ref = _double_norm(rec, rec["snaps"][0])
    print(f"\nlast_grad_norm {float(rec['norms'][0]):.9g}, double reference {float(ref):.9g}")
    assert _ulps(rec["norms"][0], ref) <= 1
    tnorm = _check_against_restatement(rec, clip, m_of=_slices(rec, opt.m))
    assert abs(float(tnorm) - float(ref)) <= 1e-5 * float(ref)          # (torch's own fp32 norm, for the record: not the yardstick)
    assert _same_bits(rec["coefs"][0].reshape(1), _torch_coef(rec["norms"][0], clip).reshape(1))
    assert rec["grad_max"] == [0.0]


def test_accumulated_micro_batches_clip_the_norm_of_the_mean_gradient():
    norm0, _ = _first_norm()
    rec = _run(2, acc=2, gradient_clip_val=0.25 * norm0, track_grad_norm=2)
    assert rec["grad_scale"] == 0.5 and len(rec["snaps"]) == 1
    ref = _double_norm(rec, rec["snaps"][0])                            # the buffer holds the SUM of the two micro-batches; x 1/2
    assert _ulps(rec["norms"][0], ref) <= 1 and float(rec["coefs"][0]) < 1.0
    _check_against_restatement(rec, 0.25 * norm0, m_of=_slices(rec, rec["opt"].m))


def test_frozen_vision_tower_takes_no_part_in_the_norm():
    """F2 of DESIGN section 11: the frozen tower has no chunk (its launches are skipped); the norm is torch's over the trainable tensors."""
    norm0, _ = _first_norm()
    rec = _run(1, freeze=VISION, gradient_clip_val=0.5 * norm0)
    names = set(rec["trainable"])
    assert names and not any(n.startswith(VISION) for n in names) and len(names) < len(rec["slots"]) - 20
    ref = _double_norm(rec, rec["snaps"][0])
    assert _ulps(rec["norms"][0], ref) <= 1 and float(ref) < norm0
    assert rec["grad_max"] == [0.0]
    _check_against_restatement(rec, 0.5 * norm0, m_of=_slices(rec, rec["opt"].m))


def test_zero_only_chunks_of_a_frozen_tensor_are_left_to_the_update():
    """FLAVA computes every gradient; a frozen tensor gets a ZERO_ONLY chunk: not in the norm, not scaled, cleared by the update as before."""
    import bench
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.trainer import Trainer
    model, lit, cfg = bench.build(32, seed=0, device=torch.device("cuda", 0), backbone="flava")
    frozen = next(n for n, p in model.named_parameters() if n.endswith("attention.attention.query.weight"))
    model.freeze(frozen)
    lit.args.warm_up_radio = 0.0
    batch = D.make_batch(2, 64, seed=17, device="cuda")
    tr = Trainer(max_epochs=1, world_size=1, gradient_clip_val=1e-3)
    tr._setup(lit, [batch] * 2)
    st, opt = model.store, tr.optimizer
    ch = st.chunks.cpu()
    assert int((ch[:, 2] & ZERO_ONLY != 0).sum()) > 0
    snaps, inner = [], opt.step

    def step():
        snaps.append(st.grad.detach().clone())
        return inner()
    opt.step = step
    w_before = st.m(frozen).clone()
    tr.train_step(lit, batch, 0)
    s = st.slots[frozen]
    assert float(snaps[0][s.offset:s.offset + s.numel].abs().max()) > 0      # its gradient WAS written ...
    parts = [snaps[0][st.slots[n].offset:st.slots[n].offset + st.slots[n].numel] for n in st.trainable_names()]
    assert frozen not in st.trainable_names()
    ref = torch.stack([p.double().pow(2).sum() for p in parts]).sum().sqrt().float()
    assert _ulps(opt.last_grad_norm, ref) <= 1 and float(opt.last_clip_coef) < 1.0      # ... and is not in the norm
    assert float(st.grad.abs().max()) == 0.0 and torch.equal(st.m(frozen), w_before)
    m = opt.m[s.offset:s.offset + s.numel]
    assert float(m.abs().max()) == 0.0
    live = next(n for n in st.trainable_names() if n.endswith("attention.attention.key.weight"))
    sl = st.slots[live]
    want = 0.1 * snaps[0][sl.offset:sl.offset + sl.numel] * opt.last_clip_coef
    got = opt.m[sl.offset:sl.offset + sl.numel]
    assert float(((got - want).abs() / (1e-5 * want.abs() + 1e-30)).max()) <= 1.0
    model.engine.grad_ready = model.engine.grad_ready_async = None


def test_clip_by_value_against_torch():
    rec = _run(1, gradient_clip_val=1e-4, gradient_clip_algorithm="value")
    assert rec["norms"] == [None] and not rec["tr"].stream_optimizer
    assert float(torch.cat([s.abs().max().reshape(1) for s in _slices(rec, rec["snaps"][0])]).max()) > 1e-4      # the clamp bites
    _check_against_restatement(rec, 1e-4, algorithm="value", m_of=_slices(rec, rec["opt"].m))
    rec = _run(2, acc=2, gradient_clip_val=1e-4, gradient_clip_algorithm="value")      # threshold handed down as clip_val / grad_scale
    _check_against_restatement(rec, 1e-4, algorithm="value", m_of=_slices(rec, rec["opt"].m))


def test_tracking_the_inf_norm_alone_changes_no_weight():
    rec = _run(3, track_grad_norm="inf")
    assert not rec["tr"].stream_optimizer and rec["coefs"] == [None] * 3
    for snap, got in zip(rec["snaps"], rec["norms"]):
        assert _same_bits(got.reshape(1), _double_norm(rec, snap, inf=True).reshape(1))
    assert _same_bits(rec["master"], _plain_unstreamed())


def test_torch_optimizer_on_store_with_clipping():
    norm0, _ = _first_norm()
    rec = _run(1, optimizer="Adam", gradient_clip_val=0.5 * norm0)
    from mkg_analogy_amd.optim import TorchOptimizerOnStore
    assert isinstance(rec["opt"], TorchOptimizerOnStore)
    assert _ulps(rec["norms"][0], _double_norm(rec, rec["snaps"][0])) <= 1 and 0.49 < float(rec["coefs"][0]) < 0.51
    named = dict(_mkg()[0].named_parameters())
    m_of = [rec["opt"].inner.state[named[n]]["exp_avg"].reshape(-1) for n in rec["trainable"]]
    _check_against_restatement(rec, 0.5 * norm0, optimizer="Adam", m_of=m_of)


def test_fp32_verification_mode_step_with_clipping():
    """The fp32 engine's training step is the verification mode: no dropout replay, so the shared configuration's dropout is 0 for its duration."""
    tc = _mkg()[0].engine.tc
    old = (tc.hidden_dropout_prob, tc.attention_probs_dropout_prob)
    tc.hidden_dropout_prob = tc.attention_probs_dropout_prob = 0.0
    try:
        rec = _run(1, precision="fp32", track_grad_norm=2)
        n32 = float(rec["norms"][0])
        assert np.isfinite(n32) and n32 > 0
        rec = _run(1, precision="fp32", gradient_clip_val=0.5 * n32)
        assert _ulps(rec["norms"][0], _double_norm(rec, rec["snaps"][0])) <= 1 and 0.49 < float(rec["coefs"][0]) < 0.51
        _check_against_restatement(rec, 0.5 * n32, m_of=_slices(rec, rec["opt"].m))
    finally:
        tc.hidden_dropout_prob, tc.attention_probs_dropout_prob = old
        _fresh()                                                         # back to bf16 for whoever comes next


def test_trainer_logs_one_norm_per_optimizer_step():
    from mkg_analogy_amd.trainer import Trainer
    norm0, _ = _first_norm()
    model, lit, batches = _fresh()
    tr = Trainer(max_epochs=1, world_size=1, gradient_clip_val=0.9 * norm0, log_every=2)
    seen, inner = [], tr.train_step

    def train_step(*a, **k):
        out = inner(*a, **k)
        seen.append((float(tr.optimizer.last_grad_norm), float(tr.optimizer.last_clip_coef)))
        return out
    tr.train_step = train_step
    hist = tr.fit(lit, list(batches))
    assert len(seen) == 4 and tr.grad_norms.dtype == np.float32 and tr.grad_norms.shape == (4,) and np.isfinite(tr.grad_norms).all()
    assert tr.grad_norms.tolist() == [n for n, _ in seen]
    assert hist[0]["clipped_steps"] == sum(1 for _, c in seen if c < 1.0) and 1 <= hist[0]["clipped_steps"] <= 4
    assert hist[0]["grad_norm_max"] == max(n for n, _ in seen) and abs(hist[0]["grad_norm_mean"] - np.mean([n for n, _ in seen])) < 1e-5 * norm0
    model.engine.grad_ready = model.engine.grad_ready_async = None


def test_streamed_range_then_clip_is_refused():
    from mkg_analogy_amd.trainer import Trainer
    model, lit, batches = _fresh()
    tr = Trainer(max_epochs=1, world_size=1, gradient_clip_val=1.0)
    tr._setup(lit, list(batches))
    opt, st = tr.optimizer, model.store
    opt.zero_grad()
    opt.begin_step()
    st.touch_grad()
    opt.ready(st.total)                                                 # the whole update went out before the norm could be taken
    with pytest.raises(RuntimeError, match="global norm"):
        opt.step()
    torch.cuda.synchronize()


def test_one_rank_process_group_with_clipping_matches_the_plain_run():
    """MART_FORCE_PG=1: the bucketed, backward-overlapped all-reduce of a 1-rank nccl group in front of the clip (tests/_grad_clip_pg_worker.py)."""
    env = dict(os.environ, MART_FORCE_PG="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29563",
           os.path.join(ROOT, "tests", "_grad_clip_pg_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print("\n", out)
    assert out["reducer_on"] and not out["reducer_off"] and out["coef_pg"] < 1.0
    assert out["masters_equal"] and out["norm_pg"] == out["norm_plain"] and out["moved"] > 0
