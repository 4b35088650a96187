"""Gradient clipping / norm tracking on a GPU-less box: the four mart_clip_* entry points beside the C ABI (exported, declared in include/mart_clip.h
as the ctypes table binds them, ABI version and entry-point count of mart_hip.h untouched), their host-side refusals, the refusals of the functional
wrappers, and the host logic of optimizer and Trainer with stubs (no launch anywhere)."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = ("mart_clip_partials_needed", "mart_clip_sumsq", "mart_clip_finalize", "mart_clip_apply")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mkg_analogy_amd import _lib
    return _lib


def _so(lib):
    so = ctypes.CDLL(lib.LIB_PATH)                      # plain dlopen: no GPU needed
    for n in CLIP:
        getattr(so, n).restype, getattr(so, n).argtypes = lib._CLIP_SIGS[n]
    so.mart_last_error.restype = ctypes.c_char_p
    return so


def test_clip_entry_points_are_exported_beside_the_abi(lib):
    so = ctypes.CDLL(lib.LIB_PATH)
    assert tuple(lib._CLIP_SIGS) == CLIP and all(hasattr(so, n) for n in CLIP)
    so.mart_abi_version.restype = ctypes.c_int
    assert so.mart_abi_version() == lib.EXPECTED_ABI == 10
    assert len(lib.EXPORTS) == 71 and not set(CLIP) & set(lib.EXPORTS) and not set(CLIP) & set(lib._SIGS)
    assert "mart_clip" not in open(os.path.join(ROOT, "include", "mart_hip.h")).read()
    assert all(getattr(lib.lib(), n).argtypes == lib._CLIP_SIGS[n][1] for n in CLIP)      # bound by lib() next to _SIGS


def test_clip_header_matches_the_ctypes_table(lib):
    hdr = open(os.path.join(ROOT, "include", "mart_clip.h")).read()
    decl = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    found = dict(re.findall(r"\bint (mart_clip_\w+)\(([^)]*)\);", decl))
    assert tuple(found) == CLIP
    kind = {"int": lib.i32, "float": lib.f32}
    for name, params in found.items():
        args = []
        for p in params.split(","):
            p = p.strip()
            args.append(lib.vp if "*" in p else kind[p.split()[0]])
        res, want = lib._CLIP_SIGS[name]
        assert res is lib.i32 and args == want, (name, params)
    assert "int mart_clip_sumsq(const float* grad, const int32_t* chunks, int n_chunks, int mode, double* partials, int n_partials, void* stream);" in decl
    assert "#define MART_CLIP_PARTS 8" in hdr


def test_clip_entry_points_refuse_bad_arguments_without_a_launch(lib):
    """Host pointers and a null stream: everything below must be refused before anything is dereferenced or launched."""
    so = _so(lib)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(rc):
        assert rc != 0 and b"clip" in so.mart_last_error()

    assert so.mart_clip_partials_needed(1) == 8 and so.mart_clip_partials_needed(7) == 56
    refused(so.mart_clip_partials_needed(0))
    refused(so.mart_clip_partials_needed(-3))
    refused(so.mart_clip_partials_needed(2 ** 31 - 1))               # 8 x n_chunks would not fit an int
    for grad, chunks, n, mode, part, npart in ((None, p, 2, 0, p, 16), (p, None, 2, 0, p, 16), (p, p, 2, 0, None, 16), (p, p, 0, 0, p, 16),
                                               (p, p, -1, 0, p, 16), (p, p, 2, 0, p, 15), (p, p, 2, 0, p, 0), (p, p, 2, 2, p, 16), (p, p, 2, -1, p, 16)):
        refused(so.mart_clip_sumsq(grad, chunks, n, mode, part, npart, None))
    for part, npart, mode, out, log, li in ((None, 8, 0, p, None, 0), (p, 8, 0, None, None, 0), (p, 0, 0, p, None, 0), (p, -8, 1, p, None, 0),
                                            (p, 8, 2, p, None, 0), (p, 8, 0, p, p, -1), (p, 8, 1, p, None, -1)):
        refused(so.mart_clip_finalize(part, npart, mode, 1.0, 1.0, out, log, li, None))
    for grad, chunks, n, coef, value in ((None, p, 2, p, 0.0), (p, None, 2, p, 0.0), (p, p, 0, p, 0.0), (p, p, -2, p, 1.0), (p, p, 2, None, 0.0),
                                         (p, p, 2, None, -1.0), (None, p, 2, None, 1.0)):
        refused(so.mart_clip_apply(grad, chunks, n, coef, value, None))


def test_functional_clip_refuses_on_the_host(lib):
    from mkg_analogy_amd import functional as Fn
    store = types.SimpleNamespace(grad=torch.zeros(512), chunks=torch.tensor([[0, 512, 1]], dtype=torch.int32), n_chunks=1)
    model = types.SimpleNamespace(store=store)
    for bad in (1, 1.0, 3, "fro", None, 0.5):
        with pytest.raises(ValueError, match="clip"):
            Fn.clip_grad_norm_(model, 1.0, norm_type=bad)              # refused before the device is looked at
        with pytest.raises(ValueError, match="clip"):
            Fn.grad_norm(store, norm_type=bad)
    for ok in (2, 2.0, "2", float("inf"), "inf"):
        with pytest.raises(ValueError, match="HIP device"):
            Fn.clip_grad_norm_(model, 1.0, norm_type=ok)               # valid arguments, but no CPU path: an error, never a fallback
        with pytest.raises(ValueError, match="HIP device"):
            Fn.grad_norm(store, norm_type=ok)
    with pytest.raises(ValueError, match="clip"):
        Fn.clip_grad_norm_(model, 0.0)
    with pytest.raises(ValueError, match="HIP device"):
        Fn.clip_grad_value_(model, 0.5)
    with pytest.raises(ValueError, match="clip"):
        Fn.clip_grad_value_(model, -0.5)
    assert torch.equal(store.grad, torch.zeros(512))


# ------------------------------------------------------------------------------------------------ host logic with stubs
class _StubOptimizer:
    """Records what the Trainer calls; ``begin_step`` / ``ready`` exist, as on FusedAdamW."""

    def __init__(self):
        self.calls, self.param_groups, self.grad_scale, self.clip = [], [{"lr": 1e-3}], 1.0, None

    def zero_grad(self):
        self.calls.append("zero_grad")

    def begin_step(self):
        self.calls.append("begin_step")

    def ready(self, upto, events=()):
        self.calls.append("ready")

    def step(self):
        self.calls.append("step")

    def set_grad_clip(self, clip_val=None, algorithm="norm", track_norm=None, log_slots=1024):
        self.clip = dict(clip_val=clip_val, algorithm=algorithm, track_norm=track_norm, log_slots=log_slots)


class _StubLit:
    def __init__(self):
        self.opt = _StubOptimizer()
        self.model = types.SimpleNamespace(engine=types.SimpleNamespace(grad_ready=None, grad_ready_async=None), finalize=lambda: None, train=lambda: None)
        self.w = torch.zeros(1, requires_grad=True)

    def configure_optimizers(self):
        return {"optimizer": self.opt, "lr_scheduler": {"scheduler": types.SimpleNamespace(step=lambda: None)}}

    def training_step(self, batch, idx):
        if self.model.engine.grad_ready_async is not None:
            self.model.engine.grad_ready_async(0)                      # what the engine does while the backward pass runs
        return (self.w * 1.0).sum()


def _stub_trainer(monkeypatch, world=1, **kw):
    from mkg_analogy_amd import trainer as T
    sync = types.SimpleNamespace(grad_scale=1.0 / world, reducer=None, begin=lambda: None, finish=lambda: None, broadcast_optimizer=lambda o: None)
    monkeypatch.setattr(T, "GradSync", lambda model: sync)
    lit = _StubLit()
    tr = T.Trainer(world_size=world, **kw)
    tr._setup(lit, [{}] * 8)
    return tr, lit


def test_trainer_with_clipping_never_streams_the_update(lib, monkeypatch):
    monkeypatch.delenv("MART_STREAM_OPT", raising=False)
    tr, lit = _stub_trainer(monkeypatch, gradient_clip_val=1.0)
    assert tr.clips_gradients and not tr.stream_optimizer
    assert lit.opt.clip == dict(clip_val=1.0, algorithm="norm", track_norm=None, log_slots=8)
    for i in range(3):
        tr.train_step(lit, {}, i)
    assert lit.opt.calls == ["zero_grad", "step"] * 3                  # no begin_step(), and the engine's hook was never routed to ready()
    assert lit.model.engine.grad_ready_async is None
    tr, lit = _stub_trainer(monkeypatch, track_grad_norm="inf", accumulate_grad_batches=2)
    assert lit.opt.clip == dict(clip_val=None, algorithm="norm", track_norm="inf", log_slots=4) and not tr.stream_optimizer
    for i in range(4):
        tr.train_step(lit, {}, i)
    assert lit.opt.calls == ["zero_grad", "step"] * 2


def test_trainer_defaults_do_what_they_did(lib, monkeypatch):
    monkeypatch.delenv("MART_STREAM_OPT", raising=False)
    for kw in ({}, dict(gradient_clip_val=None, track_grad_norm=None), dict(gradient_clip_val=0.0)):       # (PL: a clip value of 0 is "off")
        tr, lit = _stub_trainer(monkeypatch, **kw)
        assert tr.stream_optimizer and not tr.clips_gradients and lit.opt.clip is None and tr.grad_norms is None
        for i in range(2):
            tr.train_step(lit, {}, i)
        assert lit.opt.calls == ["zero_grad", "begin_step", "ready", "step"] * 2       # streamed: ranges released from inside the backward pass
    from mkg_analogy_amd.trainer import Trainer
    for bad in (dict(gradient_clip_algorithm="l2"), dict(track_grad_norm=1), dict(track_grad_norm="fro")):
        with pytest.raises(ValueError):
            Trainer(world_size=1, **bad)


def test_value_threshold_and_norm_scale_follow_grad_scale(lib, monkeypatch):
    """The buffer holds the unscaled sum over ranks and accumulation windows; AdamW multiplies by grad_scale = 1 / (world x windows) later.  So the
    norm is scaled in the finalize, and a value threshold is handed down as clip_val / grad_scale."""
    from mkg_analogy_amd import ops
    from mkg_analogy_amd.optim import GradClip
    tr, lit = _stub_trainer(monkeypatch, world=4, accumulate_grad_batches=2, gradient_clip_val=0.5, gradient_clip_algorithm="value")
    assert lit.opt.grad_scale == 1.0 / 8 and lit.opt.clip["algorithm"] == "value"
    store = types.SimpleNamespace(grad=torch.zeros(512), chunks=torch.tensor([[0, 512, 1]], dtype=torch.int32), n_chunks=1)
    gc = GradClip(store, **{k: v for k, v in lit.opt.clip.items()})
    assert gc.plan(lit.opt.grad_scale) == {"passes": [], "apply": "value", "clip_value": 0.5 / (1.0 / 8)} and gc.last_norm is None
    assert GradClip(store, 0.5, "value", 2).plan(0.25) == {"passes": [(ops.CLIP_NORM_2, 0.0)], "apply": "value", "clip_value": 2.0}
    both = GradClip(store, 0.5, "norm", 2)
    assert both.plan(0.125) == {"passes": [(ops.CLIP_NORM_2, 0.5)], "apply": "norm", "clip_value": 0.0} and both.i_track == both.i_clip == 0
    two = GradClip(store, 0.5, "norm", "inf")                          # an inf-norm to report and the 2-norm to clip by: two passes
    assert two.plan()["passes"] == [(ops.CLIP_NORM_INF, 0.0), (ops.CLIP_NORM_2, 0.5)] and (two.i_track, two.i_clip) == (0, 1)
    assert GradClip(store, None, "norm", "inf").plan() == {"passes": [(ops.CLIP_NORM_INF, 0.0)], "apply": None, "clip_value": 0.0}
    assert not GradClip(store).active and not GradClip(store, 0.0).active
    assert tuple(both.partials.shape) == (8,) and both.partials.dtype == torch.float64 and tuple(both.logs.shape) == (1, 1024)
    with pytest.raises(ValueError, match="HIP device"):
        both.run(store, 1.0)                                           # a CPU store: refused, nothing computed on the host instead
    with pytest.raises(ValueError, match="clip"):
        GradClip(store, 1.0, "l2")
    with pytest.raises(ValueError, match="clip"):
        GradClip(store, 1.0, "norm", 3)


def test_optimizer_step_refuses_a_clip_after_a_streamed_range(lib):
    """FusedAdamW.step() with clipping set: if ready() already applied part of the update, a global norm can no longer be applied."""
    from mkg_analogy_amd import optim
    assert issubclass(optim.FusedAdamW, optim._ClipsGradients) and issubclass(optim.TorchOptimizerOnStore, optim._ClipsGradients)
    store = types.SimpleNamespace(grad=torch.zeros(512), chunks=torch.tensor([[0, 512, 1]], dtype=torch.int32), n_chunks=1, total=512)
    opt = optim.FusedAdamW.__new__(optim.FusedAdamW)                   # the guard reads nothing but these attributes
    opt.model = types.SimpleNamespace(store=store)
    opt.set_grad_clip(1.0)
    assert opt._clip is not None and opt.last_grad_norm is not None and opt.last_clip_coef is not None
    opt._streaming, opt._cursor = True, 1
    opt._optimizer_step_pre_hooks = {}                                 # (torch wraps step() of a class once an instance was constructed)
    with pytest.raises(RuntimeError, match="global norm"):
        opt.step()
    opt.set_grad_clip(None, track_norm=None)
    assert opt._clip is None and opt.last_grad_norm is None


def test_lit_model_parser_adds_the_trainer_arguments_once(lib):
    import argparse
    from mkg_analogy_amd.lit_models.base import BaseLitModel
    a = BaseLitModel.add_to_argparse(argparse.ArgumentParser()).parse_args([])
    assert (a.gradient_clip_val, a.gradient_clip_algorithm, a.track_grad_norm) == (None, "norm", None)
    a = BaseLitModel.add_to_argparse(argparse.ArgumentParser()).parse_args(["--gradient_clip_val", "0.5", "--gradient_clip_algorithm", "value",
                                                                            "--track_grad_norm", "inf"])
    assert (a.gradient_clip_val, a.gradient_clip_algorithm, a.track_grad_norm) == (0.5, "value", "inf")
    p = argparse.ArgumentParser()                                      # a caller (pl.Trainer.add_argparse_args) that brought its own
    p.add_argument("--gradient_clip_val", type=float, default=7.0)
    p.add_argument("--track_grad_norm", default=-1)
    a = BaseLitModel.add_to_argparse(p).parse_args([])
    assert (a.gradient_clip_val, a.gradient_clip_algorithm, a.track_grad_norm) == (7.0, "norm", -1)
