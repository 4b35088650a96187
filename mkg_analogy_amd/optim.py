"""Fused AdamW over the flat parameter buffer + the linear warmup/decay schedule
(reference: lit_models/transformer.py:224-241; torch.optim.AdamW and HF get_linear_schedule_with_warmup semantics)."""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from . import ops
from .params import NO_DECAY, check_layout, layout_list


def norm_mode(norm_type) -> int:
    """``2`` / ``2.0`` / ``"2"`` -> ops.CLIP_NORM_2, ``inf`` / ``"inf"`` -> ops.CLIP_NORM_INF: the two norms the clip kernels compute."""
    try:
        v = float(norm_type)
    except (TypeError, ValueError):
        v = None
    if v == 2.0:
        return ops.CLIP_NORM_2
    if v == math.inf:
        return ops.CLIP_NORM_INF
    raise ValueError(f"clip: norm_type must be 2 or inf, got {norm_type!r}")


class GradClip:
    """pl.Trainer's ``gradient_clip_val`` / ``gradient_clip_algorithm`` / ``track_grad_norm`` on the flat gradient buffer, as kernels that run between
    the backward pass and the AdamW launch (include/mart_clip.h): per norm one streaming pass into float64 partials and a one-workgroup finalize that
    leaves (norm, clip coefficient) on the device, then one pass that scales -- and returns at once when the coefficient is 1 -- or clamps.  The
    chunk table says which elements are gradients of trainable parameters.  Nothing here synchronises with the host, and every buffer (partials, one
    (norm, coef) pair and one log row of ``log_slots`` steps per norm) is allocated here, once.

    ``clip_val`` None or <= 0: no clipping (PL).  ``algorithm`` "norm": the 2-norm of all gradients together is brought down to ``clip_val``;
    "value": every element is clamped to +-``clip_val``.  ``track_norm`` 2 / "inf" / None: the norm to report (before clipping, as PL); a tracked
    2-norm and norm clipping share their pass."""

    def __init__(self, store, clip_val=None, algorithm: str = "norm", track_norm=None, log_slots: int = 1024):
        if algorithm not in ("norm", "value"):
            raise ValueError(f"clip: gradient_clip_algorithm must be 'norm' or 'value', got {algorithm!r}")
        self.clip_val = float(clip_val) if clip_val is not None and float(clip_val) > 0 else None
        self.algorithm = algorithm
        self.track_mode = None if track_norm is None else norm_mode(track_norm)
        by_norm = self.clip_val is not None and algorithm == "norm"
        self.passes = []                                             # (mode, max_norm): one sumsq + finalize each; max_norm 0 = track only
        self.i_track = self.i_clip = None
        if self.track_mode is not None and not (by_norm and self.track_mode == ops.CLIP_NORM_2):
            self.i_track = len(self.passes)
            self.passes.append((self.track_mode, 0.0))
        if by_norm:
            self.i_clip = len(self.passes)
            self.passes.append((ops.CLIP_NORM_2, self.clip_val))
            if self.track_mode == ops.CLIP_NORM_2:
                self.i_track = self.i_clip
        self.active = self.clip_val is not None or self.track_mode is not None
        dev = store.grad.device
        self.log_slots = max(1, int(log_slots))
        self.log_index = 0
        self.partials = torch.zeros(ops.clip_partials_needed(max(1, store.n_chunks)), device=dev, dtype=torch.float64)
        self._n_chunks = store.n_chunks
        self.outs = torch.zeros(max(1, len(self.passes)), 2, device=dev, dtype=torch.float32)
        self.logs = torch.zeros(max(1, len(self.passes)), self.log_slots, device=dev, dtype=torch.float32)

    def plan(self, grad_scale: float = 1.0) -> dict:
        """What one step launches (pure host logic): the norm passes, and how the gradients are changed.  The buffer holds the unscaled sum
        and AdamW multiplies by ``grad_scale`` later, so the norm is scaled in the finalize and a value threshold is divided by it:
        clamp(s g, +-v) = s clamp(g, +-v / s)."""
        by_value = self.clip_val is not None and self.algorithm == "value"
        return {"passes": list(self.passes), "apply": "norm" if self.i_clip is not None else "value" if by_value else None,
                "clip_value": self.clip_val / float(grad_scale) if by_value else 0.0}

    def run(self, store, grad_scale: float = 1.0) -> None:
        if not store.grad.is_cuda:
            raise ValueError("clip: the gradient buffer must live on the HIP device (there is no CPU path)")
        n = store.n_chunks
        if n != self._n_chunks:                                      # the chunk table was rebuilt: more rows (a thaw) is the one case that allocates
            if ops.clip_partials_needed(n) > self.partials.numel():
                self.partials = torch.zeros(ops.clip_partials_needed(n), device=store.grad.device, dtype=torch.float64)
            self._n_chunks = n
        plan = self.plan(grad_scale)
        slot = self.log_index if self.log_index < self.log_slots else None          # a full log stops recording
        for i, (mode, max_norm) in enumerate(plan["passes"]):
            ops.clip_sumsq(store.grad, store.chunks, n, mode, self.partials)
            ops.clip_finalize(self.partials, mode, self.outs[i], grad_scale=grad_scale, max_norm=max_norm,
                              log=None if slot is None else self.logs[i], log_index=slot or 0)
        if plan["apply"] == "norm":
            ops.clip_apply(store.grad, store.chunks, n, coef=self.outs[self.i_clip, 1:])
        elif plan["apply"] == "value":
            ops.clip_apply(store.grad, store.chunks, n, clip_value=plan["clip_value"])
        self.log_index += 1

    @property
    def last_norm(self):
        """Device scalar: the tracked norm of the last step, or the clip's 2-norm when nothing else is tracked (None: value clipping alone)."""
        i = self.i_track if self.i_track is not None else self.i_clip
        return None if i is None else self.outs[i, 0]

    @property
    def last_coef(self):
        """Device scalar: the factor the last step's gradients were multiplied by (1: the clip did not trigger; None without norm clipping)."""
        return None if self.i_clip is None else self.outs[self.i_clip, 1]

    def read_log(self, reset: bool = True):
        """(norms, clipped_steps) of the steps since the last reset: one device-to-host copy (the only synchronisation, at a place the caller
        chooses).  ``norms``: float32 numpy array, one entry per step (None when no norm is computed); ``clipped_steps``: steps whose clip
        coefficient -- recomputed from the logged norm with the kernel's fp32 expression -- was below 1 (None without norm clipping)."""
        import numpy as np
        n = min(self.log_index, self.log_slots)
        logs = self.logs[:, :n].cpu().numpy()
        if reset:
            self.log_index = 0
        i = self.i_track if self.i_track is not None else self.i_clip
        norms = None if i is None else logs[i].copy()
        clipped = None
        if self.i_clip is not None:
            with np.errstate(all="ignore"):
                coef = (np.float32(1.0) / (logs[self.i_clip] + np.float32(1e-6))) * np.float32(self.clip_val)
            clipped = int((coef < 1).sum())
        return norms, clipped


class _ClipsGradients:
    """``set_grad_clip`` and the two device scalars of the optimizers that own a FlatStore."""
    _clip: Optional[GradClip] = None

    def set_grad_clip(self, clip_val=None, algorithm: str = "norm", track_norm=None, log_slots: int = 1024) -> None:
        """Clip (and / or report the norm of) the gradients inside every ``step()``, before the update: see :class:`GradClip`.  With neither
        ``clip_val`` nor ``track_norm`` the step is again exactly the unclipped one."""
        gc = GradClip(self.model.store, clip_val, algorithm, track_norm, log_slots)
        self._clip = gc if gc.active else None

    def read_norm_log(self, reset: bool = True):
        """(norms, clipped_steps) of the optimizer steps since the last reset (GradClip.read_log: one device-to-host copy); (None, None) when off."""
        return (None, None) if self._clip is None else self._clip.read_log(reset)

    @property
    def last_grad_norm(self):
        return None if self._clip is None else self._clip.last_norm

    @property
    def last_clip_coef(self):
        return None if self._clip is None else self._clip.last_coef


class FusedAdamW(torch.optim.Optimizer, _ClipsGradients):
    """One multi-tensor HIP launch per step: fp32 master/m/v update + bf16 shadow refresh, then W^T shadows.

    ``param_groups`` mirrors the reference's two groups (decay 0.01 / 0 by the substring rule) for inspection and
    for the scheduler's ``lr`` plumbing; tensors that never receive a gradient in the reference (dead pooler /
    post-layernorm: grad None => torch skips them entirely) and frozen tensors (``requires_grad = False`` when
    ``model.sync_trainable()`` / ``configure_optimizers()`` read the flags) are left untouched: no update, no weight
    decay, and their m / v / master / shadows never change.
    """

    def __init__(self, model, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale: float = 1.0):
        self.model = model
        store = model.store
        # the groups name exactly the tensors the chunk table updates: the trainable set the store was last handed (HipMaskedLM.sync_trainable --
        # requires_grad minus the dead tensors, read once), not a second reading of the flags
        named = dict(model.named_parameters())
        names = store.trainable_names()
        decay = [named[n] for n in names if not any(nd in n for nd in NO_DECAY)]
        no_decay = [named[n] for n in names if any(nd in n for nd in NO_DECAY)]
        groups = [{"params": decay, "weight_decay": weight_decay}, {"params": no_decay, "weight_decay": 0}]
        super().__init__(groups, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.m = torch.zeros_like(store.master)
        self.v = torch.zeros_like(store.master)
        self.steps = 0
        self.grad_scale = grad_scale
        self._store_id = id(store)
        self._stream = None
        self._streaming = False
        # MART_ASYNC_STEP=1: step-boundary work that the NEXT forward pass does not need -- the gradient zero-fill and the refresh of the transposed
        # weight shadows (read by data-gradient GEMMs only) -- stays on the optimizer stream; the backward pass joins it (FlatStore.join_pending).
        # Off by default: measured within noise of the in-order form (87.24 / 87.50 vs 87.47 / 87.36 ms: the un-profiled step boundary has no idle
        # time to recover, docs/LAB_r01-r05.md section 4.3), and with it ``zero_grad()`` returns before ``p.grad`` reads as zero on the caller's stream.
        self.async_step = os.environ.get("MART_ASYNC_STEP", "0") == "1"
        # fused_zero_grad: the update kernel writes 0 back to the gradient elements it has just consumed, and the next ``zero_grad()`` finds the buffer
        # clean (FlatStore.grad_clean) and skips its 0.94 GB fill -- 0.13-0.19 ms at the head of every step on the main queue, moved under the backward
        # pass where the update ranges already run.  torch semantics differ in ONE observable way: ``p.grad`` reads zero after ``optimizer.step()``
        # instead of keeping the step's gradients until the next ``zero_grad()``.  The Trainer (which owns both calls, lit_models hooks see the
        # gradients between backward and step as in PL) turns it on; a bare ``FusedAdamW`` keeps torch's behaviour (MART_FUSED_ZERO_GRAD=0: off everywhere).
        self.fused_zero_grad = False

    def _side(self):
        if self._stream is None:
            self._stream = torch.cuda.Stream(priority=int(os.environ.get("MART_OPT_PRIO", "0")))
        return self._stream

    def zero_grad(self, set_to_none: bool = False):
        """With ``async_step`` the 0.94 GB fill runs on the optimizer stream, next to the forward pass (which never touches the gradient buffer); whatever
        writes gradients waits for it first (FlatStore.join_pending: the model's forward call joins before returning, and every
        backward kernel is enqueued later).  Default (``MART_ASYNC_STEP=0``): the plain in-order fill."""
        store = self.model.store
        if store.grad_is_clean():
            return                                                       # zeroed by the last update (fused_zero_grad) and not written since (by a kernel or through p.grad)
        if not (self.async_step and store.grad.is_cuda):
            store.zero_grad()
            return
        st = self._side()
        st.wait_stream(torch.cuda.current_stream())                      # readers / writers of the gradients enqueued so far
        with torch.cuda.stream(st):
            store.grad.zero_()
        store.pending(st)

    # ---- streamed step: the update of a parameter range is launched as soon as its gradients are final (the backward
    # pass reports "everything below flat offset X is final", layout order == completion order), on its own stream, under
    # the rest of the backward pass: AdamW is HBM-bound, the backward GEMMs are not, and the ~1.4 ms of the update
    # otherwise run alone at the end of every step.  The weights of a finished range are not read again in this step.
    def begin_step(self) -> None:
        """Call before the backward pass whose gradients this step consumes; ``ready`` / ``step`` then finish it."""
        store = self.model.store
        if id(store) != self._store_id:
            raise RuntimeError("the model's parameter storage was rebuilt (resize/.to()) after the optimizer was created")
        self.steps += 1
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        self._hp = dict(lr=float(g0["lr"]), beta1=b1, beta2=b2, eps=g0["eps"], weight_decay=float(g0["weight_decay"]),
                        bc1=1.0 - b1 ** self.steps, bc2=1.0 - b2 ** self.steps, grad_scale=self.grad_scale, zero_grad=bool(self.fused_zero_grad))
        if getattr(self, "_ends_key", None) is not store.chunks:          # host copy of the chunk ends (rebuilt with the table)
            c = store.chunks.cpu()
            self._ends = (c[:, 0].long() + c[:, 1].long()).tolist()
            self._ends_key = store.chunks
        self._cursor = 0
        self._streaming = True

    def _launch(self, upto_chunk: int) -> None:
        store = self.model.store
        if upto_chunk > self._cursor:
            ops.adamw(master=store.master, grad=store.grad, m=self.m, v=self.v, shadow=store.shadow, shadow_f16=store.shadow_h,
                      chunks=store.chunks[self._cursor:upto_chunk],
                      n_chunks=upto_chunk - self._cursor, **self._hp)
            self._cursor = upto_chunk

    @torch.no_grad()
    def ready(self, upto: int, events=()) -> None:
        """Gradients below flat offset ``upto`` are final once ``events`` (and the current stream) have passed."""
        if not getattr(self, "_streaming", False):
            return
        import bisect
        j = bisect.bisect_right(self._ends, upto)
        if j <= self._cursor:
            return
        if not self.m.is_cuda:
            self._launch(j)
            return
        self._side()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._stream.wait_event(ev)
        for e in events:
            self._stream.wait_event(e)
        with torch.cuda.stream(self._stream):
            self._launch(j)

    @torch.no_grad()
    def step(self, closure=None):
        store = self.model.store
        if self._clip is not None:
            # the norm is global: every gradient must be final, and no weight may have moved, before the first update -- so the step is not
            # streamed under the backward pass (the Trainer does not call begin_step() / ready() then) and the one launch below covers all chunks
            if getattr(self, "_streaming", False) and self._cursor > 0:
                raise RuntimeError("gradient clipping / norm tracking is set (set_grad_clip) but part of this step was already applied by ready(): "
                                   "a global norm cannot be applied to weights that have moved -- do not stream the update (begin_step / ready)")
            if not getattr(self, "_streaming", False):
                self.begin_step()
            self._clip.run(store, self.grad_scale)                        # current stream: after the backward pass, before the update (ready() orders the side stream behind it)
        if not getattr(self, "_streaming", False):
            self.begin_step()
        self.ready(store.total)                                           # whatever the backward pass did not release
        self._launch(store.n_chunks)
        self._streaming = False
        if self.fused_zero_grad:
            # every chunk's gradients were zeroed by its update; the ranges outside the chunk table (dead tensors) are never written by a kernel, so
            # they still hold the zeros of the last fill -- and if anything else wrote them, through p.grad, grad_is_clean() sees the version move
            store.mark_grad_clean()
        if self._stream is not None:
            torch.cuda.current_stream().wait_stream(self._stream)       # master + bf16 / fp16 shadows are final for the next forward pass
        if self.async_step and self._stream is not None and store.grad.is_cuda:
            with torch.cuda.stream(self._stream):
                store.refresh_transposed()                               # W^T shadows: only the NEXT backward pass reads them
            store.pending(self._stream)
        else:
            store.refresh_transposed()

    def state_dict(self):
        """Flat ``m`` / ``v`` (one element per element of the master buffer) WITH the layout they belong to, the step count, and the state of the
        schedule that drives ``lr`` (LinearWarmupSchedule attaches itself), so that a resume needs nothing else."""
        sd = {"m": self.m, "v": self.v, "steps": self.steps, "lr": self.param_groups[0]["lr"], "layout": layout_list(self.model.store.slots)}
        if getattr(self, "_schedule", None) is not None:
            sd["scheduler"] = self._schedule.state_dict()
        return sd

    def load_state_dict(self, sd):
        check_layout(sd.get("layout"), self.model.store.slots)
        if tuple(sd["m"].shape) != tuple(self.m.shape) or tuple(sd["v"].shape) != tuple(self.v.shape):
            raise ValueError(f"optimizer state holds {tuple(sd['m'].shape)} moments, this model stores {tuple(self.m.shape)}")
        self.m.copy_(sd["m"]); self.v.copy_(sd["v"]); self.steps = int(sd["steps"])
        for g in self.param_groups:
            g["lr"] = sd["lr"]
        if "scheduler" in sd and getattr(self, "_schedule", None) is not None:
            self._schedule.load_state_dict(sd["scheduler"])


class TorchOptimizerOnStore(_ClipsGradients):
    """Any other ``torch.optim`` class by name, as the reference allows (lit_models/base.py:31 ``getattr(torch.optim, optimizer)``;
    lit_models/transformer.py:224-232: the same two weight-decay groups, ``lr``, ``eps=1e-8`` -- so, as there, only classes that take ``eps``).
    The update is torch's own (its kernels, on the fp32 master views: ``p`` / ``p.grad`` are views of FlatStore.master / .grad); afterwards the
    bf16 / fp16 / W^T operand shadows follow.  Tensors that never receive a gradient in the reference (grad None: torch skips them -- no update,
    no weight decay) are left out, like FusedAdamW's chunk table does.  Not the fast path: AdamW is the fused kernel."""

    def __init__(self, model, name: str, lr=5e-5, eps=1e-8, weight_decay=0.01, extra_dead=()):
        cls = getattr(torch.optim, name)                       # AttributeError for an unknown name, as the reference
        store = model.store
        dead = tuple(store.dead) + tuple(extra_dead)
        every = dict(model.named_parameters())
        named = {n: every[n] for n in store.trainable_names() if not (dead and n.startswith(dead))}     # the set FusedAdamW's chunk table uses
        decay = [p for n, p in named.items() if not any(nd in n for nd in NO_DECAY)]
        no_decay = [p for n, p in named.items() if any(nd in n for nd in NO_DECAY)]
        self.inner = cls([{"params": decay, "weight_decay": weight_decay}, {"params": no_decay, "weight_decay": 0}], lr=lr, eps=eps)
        self.model, self.grad_scale, self._store_id = model, 1.0, id(store)

    @property
    def param_groups(self):
        return self.inner.param_groups

    def zero_grad(self, set_to_none: bool = False):
        self.model.store.zero_grad()                           # the gradient buffer is persistent (kernels accumulate into it): never None

    @torch.no_grad()
    def step(self, closure=None):
        store = self.model.store
        if id(store) != self._store_id:
            raise RuntimeError("the model's parameter storage was rebuilt (resize/.to()) after the optimizer was created")
        if self.grad_scale != 1.0:
            store.grad.mul_(self.grad_scale)                   # 1 / world (DDP mean) and 1 / accumulation windows
        if self._clip is not None:
            self._clip.run(store, 1.0)                         # the gradients are scaled already
        self.inner.step()
        store.refresh_shadows()

    def state_dict(self):
        return self.inner.state_dict()

    def load_state_dict(self, sd):
        self.inner.load_state_dict(sd)


class LinearWarmupSchedule:
    """lambda(t) = t/max(1,w) for t<w else max(0,(T-t)/max(1,T-w)); w may be fractional (0.1*T)."""

    def __init__(self, optimizer, num_warmup_steps, num_training_steps, last_epoch: int = -1):
        self.optimizer = optimizer
        self.w, self.T = num_warmup_steps, num_training_steps
        self.base_lrs = [g["lr"] for g in optimizer.param_groups]
        self.last_epoch = last_epoch
        if hasattr(optimizer, "fused_zero_grad"):
            optimizer._schedule = self                                 # FusedAdamW.state_dict carries the schedule's step
        self.step()                                                    # like torch's LambdaLR: lr(0) applied at construction

    def lr_lambda(self, t: int) -> float:
        if t < self.w:
            return float(t) / float(max(1, self.w))
        return max(0.0, float(self.T - t) / float(max(1, self.T - self.w)))

    def step(self):
        self.last_epoch += 1
        f = self.lr_lambda(self.last_epoch)
        for g, b in zip(self.optimizer.param_groups, self.base_lrs):
            g["lr"] = b * f

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"last_epoch": self.last_epoch}

    def load_state_dict(self, sd):
        self.last_epoch = sd["last_epoch"] - 1
        self.step()
