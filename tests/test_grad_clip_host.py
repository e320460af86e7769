"""Gradient clipping and gradient-norm tracking, the part that needs no GPU: the four new entry points are declared, exported and bound
and refuse bad arguments before the device is touched; DataParallelTrainer's ``gradient_clip_val`` /
``gradient_clip_algorithm`` / ``track_grad_norm`` on the unfused path (torch's optimizer on a CPU module) against a hand-rolled loop
with torch's own clipping functions."""

import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ("tq_grad_sumsq", "tq_grad_clip_coef", "tq_adam_ema_step_clipped", "tq_radam_ema_step_clipped")
ERR_ARG = -1


def _lib_and_header():
    from tqdne_amd import _build, _lib
    _build.build(verbose=False)
    return _lib, _lib.load(), open(os.path.join(ROOT, "include", "tqdne_hip.h")).read()


def test_new_entry_points_are_declared_exported_and_bound():
    _lib, lib, header = _lib_and_header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*const (TqAdamChunk|double)\*", header), name
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
    assert lib.tq_abi_version() == _lib.ABI_VERSION


def test_new_entry_points_refuse_bad_arguments_before_the_device_is_touched():
    """(this box has no device: anything that got as far as a launch would not return TQ_ERR_ARG)"""
    _lib, lib, _ = _lib_and_header()
    table = C.cast((_lib.TqAdamChunk * 1)(), C.c_void_p)
    buf = C.cast((C.c_double * 4)(), C.c_void_p)   # stands for a device buffer; never dereferenced on these paths
    assert lib.tq_grad_sumsq(None, 4, buf, None) == ERR_ARG
    assert lib.tq_grad_sumsq(table, 4, None, None) == ERR_ARG
    assert lib.tq_grad_sumsq(table, 0, buf, None) == ERR_ARG
    assert lib.tq_grad_sumsq(table, -3, buf, None) == ERR_ARG
    assert lib.tq_grad_clip_coef(None, 4, 1.0, 1.0, buf, None) == ERR_ARG
    assert lib.tq_grad_clip_coef(buf, 4, 1.0, 1.0, None, None) == ERR_ARG
    assert lib.tq_grad_clip_coef(buf, 0, 1.0, 1.0, buf, None) == ERR_ARG
    assert lib.tq_grad_clip_coef(buf, -1, 1.0, 1.0, buf, None) == ERR_ARG
    adam = (1e-3, 0.9, 0.999, 1e-8, 1.0, 0.0, 1.0, 1.0, None)    # ... decay_factor, skip_flag
    radam = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 1.0, None)        # ... grad_scale, skip_flag
    for fn, args in ((lib.tq_adam_ema_step_clipped, adam), (lib.tq_radam_ema_step_clipped, radam)):
        assert fn(None, 4, *args, buf, 0.0, None) == ERR_ARG
        assert fn(table, 0, *args, buf, 0.0, None) == ERR_ARG
        assert fn(table, -3, *args, None, 0.5, None) == ERR_ARG
        assert fn(table, 4, *args, None, -0.5, None) == ERR_ARG   # a negative clip_value


class _Toy(torch.nn.Module):
    """CPU module as the trainer sees one: ``configure_optimizers`` in Lightning's dict form, ``step_and_backward`` leaves ``p.grad``
    as views of one flat buffer (the plans' layout)."""

    def __init__(self, lr=1e-2):
        super().__init__()
        torch.manual_seed(0)
        self.net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.SiLU(), torch.nn.Linear(32, 4))
        self.lr = lr
        self.flat = torch.zeros(sum(p.numel() for p in self.parameters()))

    def configure_optimizers(self):
        opt = torch.optim.Adam(self.parameters(), lr=self.lr)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=100)}}

    def step_and_backward(self, batch):
        loss = (10.0 * (self.net(batch["signal"]) - batch["cond"]) ** 2).mean()
        grads = torch.autograd.grad(loss, list(self.parameters()))
        o = 0
        for p, g in zip(self.parameters(), grads):
            self.flat[o:o + p.numel()].copy_(g.reshape(-1))
            p.grad = self.flat[o:o + p.numel()].view_as(p)
            o += p.numel()
        return loss.detach(), self.flat


def _batches(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [{"signal": torch.randn(8, 16, generator=g), "cond": torch.randn(8, 4, generator=g)} for _ in range(n)]


def _hand_rolled(steps, clip):
    ref = _Toy()
    opt = torch.optim.Adam(ref.parameters(), lr=ref.lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=100)
    norms = []
    for b in steps:
        opt.zero_grad()
        (10.0 * (ref.net(b["signal"]) - b["cond"]) ** 2).mean().backward()
        norms.append(clip(list(ref.parameters())))
        opt.step()
        sched.step()
    return ref, norms


def test_trainer_rejects_an_unknown_clip_algorithm_and_a_negative_value():
    from tqdne_amd.trainer import DataParallelTrainer
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        DataParallelTrainer(_Toy(), fused_optimizer=False, gradient_clip_val=1.0, gradient_clip_algorithm="l2")
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        DataParallelTrainer(_Toy(), fused_optimizer=False, gradient_clip_algorithm="Norm")
    with pytest.raises(ValueError, match="gradient_clip_val"):
        DataParallelTrainer(_Toy(), fused_optimizer=False, gradient_clip_val=-1.0)
    tr = DataParallelTrainer(_Toy(), fused_optimizer=False)
    assert tr.gradient_clip_val is None and tr.gradient_clip_algorithm == "norm" and tr.last_grad_norm is None
    assert DataParallelTrainer(_Toy(), fused_optimizer=False, gradient_clip_val=0).gradient_clip_val is None   # 0: off, as in Lightning


def test_unfused_norm_clipping_bounds_the_gradient_and_follows_torch():
    from tqdne_amd.trainer import DataParallelTrainer
    steps, c = _batches(4), 0.5
    m = _Toy()
    tr = DataParallelTrainer(m, fused_optimizer=False, gradient_clip_val=c)
    seen = []
    for b in steps:
        tr.train_step(b)
        total = torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in m.parameters()]).double())
        assert float(total) <= c * (1 + 1e-6)
        seen.append(float(tr.last_grad_norm))
    ref, norms = _hand_rolled(steps, lambda ps: float(torch.nn.utils.clip_grad_norm_(ps, c)))
    assert seen == norms and min(norms) > c, "every step must have clipped"
    for (n, p), q in zip(m.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), n


def test_unfused_value_clipping_and_tracking_follow_torch():
    from tqdne_amd.trainer import DataParallelTrainer
    steps, c = _batches(4), 0.05
    m = _Toy()
    tr = DataParallelTrainer(m, fused_optimizer=False, gradient_clip_val=c, gradient_clip_algorithm="value", track_grad_norm=True)
    seen = []
    for b in steps:
        tr.train_step(b)
        assert max(float(p.grad.abs().max()) for p in m.parameters()) == float(torch.tensor(c))   # (some entry was clamped)
        seen.append(float(tr.last_grad_norm))

    def clip(ps):
        n = float(torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in ps])))
        torch.nn.utils.clip_grad_value_(ps, c)
        return n

    ref, norms = _hand_rolled(steps, clip)
    assert seen == pytest.approx(norms, rel=1e-6)   # the norm BEFORE the clamp
    for (n, p), q in zip(m.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), n


def test_defaults_and_tracking_alone_leave_the_trajectory_as_it_was():
    from tqdne_amd.trainer import DataParallelTrainer
    steps = _batches(4)
    ref, norms = _hand_rolled(steps, lambda ps: float(torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in ps]))))
    for kw in ({}, {"track_grad_norm": True}):
        m = _Toy()
        tr = DataParallelTrainer(m, fused_optimizer=False, **kw)
        seen = []
        for b in steps:
            tr.train_step(b)
            seen.append(tr.last_grad_norm)
        for (n, p), q in zip(m.named_parameters(), ref.parameters()):
            assert torch.equal(p, q), n
        if kw:
            assert [float(x) for x in seen] == pytest.approx(norms, rel=1e-6)
        else:
            assert seen == [None] * 4


def test_fused_step_refuses_both_algorithms_at_once():
    """(checked in front of everything else: needs no device -- the optimizer object itself does)"""
    from tqdne_amd.optim import _FusedFlatOptimizer
    opt = object.__new__(_FusedFlatOptimizer)
    with pytest.raises(ValueError, match="alternatives"):
        _FusedFlatOptimizer.step(opt, max_grad_norm=1.0, clip_value=1.0)
    with pytest.raises(ValueError, match="positive"):
        _FusedFlatOptimizer.step(opt, max_grad_norm=0.0)
    with pytest.raises(ValueError, match="positive"):
        _FusedFlatOptimizer.step(opt, clip_value=-1.0)
