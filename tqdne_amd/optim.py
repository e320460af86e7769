"""Fused Adam / RAdam (+ EMA) for the training step: one HIP launch over the whole model (tq_adam_ema_step_guarded,
tq_radam_ema_step_guarded), optionally with gradient clipping / gradient-norm tracking decided on the device (tq_grad_sumsq,
tq_grad_clip_coef, tq_*_ema_step_clipped).

Semantics are ``torch.optim.Adam(params, lr)`` as configured by the reference (tqdne/edm.py:240-251: default betas / eps, no
weight decay) and, when ``ema_decay`` is given, the reference's EMA callback (tqdne/ema.py:24-28: ``ema.lerp_(p, 1 - decay)``
after every optimizer step).  The class is a ``torch.optim.Optimizer``: LR schedulers drive ``param_groups[0]["lr"]`` and
``state_dict()`` / ``load_state_dict()`` speak torch Adam's format, so the ``optimizer_states`` of a reference checkpoint load.
Moments (and the EMA copy) live in flat fp32 buffers; ``state[p]["exp_avg"]`` etc. are views of them.  ``swap_ema()`` exchanges
the parameters with that EMA copy in place (tq_ema_swap, one launch): the callback's other half, EMA weights for validation and
sampling (tqdne/ema.py:30-48), without a second copy of the model.

``FusedRAdamEMA`` is the same for ``torch.optim.RAdam(params, lr)``, the consistency model's optimizer (tqdne/consistency_model.py:
178-190); flat buffers, chunk table, EMA views, version bump and (de)serialisation are ``_FusedFlatOptimizer``'s, shared by both.
"""

from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from typing import Iterable, Optional, Tuple

import torch

from . import _lib
from ._lib import TQ_ADAM_CHUNK, TqAdamChunk, check


class _FusedFlatOptimizer(torch.optim.Optimizer):
    """What the one-launch optimizers share: flat moment / EMA buffers, the device chunk table, the step's bookkeeping and torch's
    state format (``step``, ``exp_avg``, ``exp_avg_sq``: Adam's and RAdam's alike), gradient clipping / norm tracking in front of
    the launch, and the choice between the guarded and the clipped entry point (``_launch``).  A subclass supplies ``_entry`` = (guarded
    entry point, clipped entry point, what ``check`` calls the launch) and ``_scalars(t, group, ema_w, grad_scale)``, the launch's
    scalars between the chunk count and the skip pointer."""

    def __init__(self, named_params: Iterable[Tuple[str, torch.nn.Parameter]], lr: float = 1e-3, betas=(0.9, 0.999),
                 eps: float = 1e-8, ema_decay: Optional[float] = None, weight_decay: float = 0.0):
        cls = type(self).__name__
        named = [(n, p) for n, p in named_params if p.requires_grad]
        if not named:
            raise ValueError("no trainable parameters")
        self._names = [n for n, _ in named]
        super().__init__([p for _, p in named], dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.ema_decay = ema_decay
        ps = self.param_groups[0]["params"]
        dev = ps[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"{cls} updates parameters on the GPU; move the module to cuda first")
        self._lib = _lib.load()  # raises when the HIP library is missing: there is no fallback update
        offs, total = [], 0
        for p in ps:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError(f"{cls} handles contiguous fp32 parameters on one device")
            offs.append(total)
            total += (p.numel() + 63) // 64 * 64  # every tensor starts 256-byte aligned
        self._offs = offs
        self._m = torch.zeros(total, device=dev)
        self._v = torch.zeros(total, device=dev)
        self._ema = None
        if ema_decay is not None:
            self._ema = torch.zeros(total, device=dev)
            for p, o in zip(ps, offs):
                self._ema[o:o + p.numel()].copy_(p.detach().reshape(-1))
        self._step = 0
        self._step_t = torch.tensor(0.0)  # one shared CPU scalar: state[p]["step"] of every parameter (torch Adam's format)
        for p, o in zip(ps, offs):
            n = p.numel()
            self.state[p] = dict(step=self._step_t, exp_avg=self._m[o:o + n].view_as(p),
                                 exp_avg_sq=self._v[o:o + n].view_as(p))
        self._table = None           # the step's table: rows of the parameters that have a gradient (``_build_table``)
        self._table_key = None
        self._n_chunks = 0
        self._updated = []           # the parameters of ``_table``: the ones whose versions a step bumps
        self._swap_table = None      # the swap's own table, made by the first ``swap_ema``
        self._swap_key = None
        self._swap_chunks = 0
        self._norm_buf = None        # (fp64 partials per chunk, [norm, coefficient]) of the current table, made on first use
        self.last_grad_norm = None   # device fp32 scalar once a step has formed the norm

    # ------------------------------------------------------------------ EMA
    ema_swapped = False   # True between two ``swap_ema()`` calls: the parameters hold the EMA weights, the EMA buffer the training weights

    def ema_state(self) -> "OrderedDict[str, torch.Tensor]":
        """name -> EMA tensor (views), the dict the reference's EMA callback stores under checkpoint['ema_state'].  Always the EMA of
        the training run: while ``ema_swapped`` the values live in the parameters, so the views are of the parameters (detached) and
        ``checkpoint.save_checkpoint(..., ema_state=optimizer.ema_state())`` keeps writing the EMA under ``ema_state``."""
        if self._ema is None:
            raise RuntimeError("constructed without ema_decay")
        ps = self.param_groups[0]["params"]
        if self.ema_swapped:
            return OrderedDict((n, p.detach()) for n, p in zip(self._names, ps))
        return OrderedDict((n, self._ema[o:o + p.numel()].view_as(p)) for n, p, o in zip(self._names, ps, self._offs))

    def load_ema_state(self, ema_state):
        """(while ``ema_swapped`` this writes the parameters: raw copies, so their versions are bumped like ``swap_ema`` does)"""
        for n, t in self.ema_state().items():
            t.copy_(ema_state[n])

    @torch.no_grad()
    def swap_ema(self):
        """Exchange every optimized parameter with its EMA in place: ONE launch (tq_ema_swap) on the current stream, no second copy of
        the model.  Toggles ``ema_swapped`` and bumps the parameters' autograd versions, as ``step`` does, so that the engines' packed
        weights follow.  While swapped ``step`` refuses to run (it would update the EMA as if it were the weights); ``ema_state()``
        keeps meaning the EMA of the run, and ``state_dict()`` is unaffected (moments and step count do not move).  The MODULE's
        ``state_dict()`` holds the EMA weights while swapped: write checkpoints after swapping back (DataParallelTrainer.save_checkpoint
        refuses inside ``ema_weights()``)."""
        if self._ema is None:
            raise RuntimeError("constructed without ema_decay")
        ps = self.param_groups[0]["params"]
        key = tuple(p.data_ptr() for p in ps)
        if key != self._swap_key:
            # (EVERY optimized parameter: unlike the step's table it does not depend on ``p.grad``, which may not exist yet)
            self._swap_table, self._swap_chunks = self._upload(self._rows(grads=False))
            self._swap_key = key
        stream = torch.cuda.current_stream(self._m.device).cuda_stream
        check(self._lib.tq_ema_swap(self._swap_table.data_ptr(), self._swap_chunks, stream), "ema swap")
        torch._C._increment_version(ps)
        self.ema_swapped = not self.ema_swapped

    # ------------------------------------------------------------------ chunk table
    def _rows(self, grads: bool):
        """(p, g, m, v, ema, n) addresses of every chunk of ``TQ_ADAM_CHUNK`` elements, 0 for null.  ``grads``: the step's rows, of the
        parameters that have a gradient; otherwise every parameter with g / m / v null (the swap's rows)."""
        def at(t, elem):
            return 0 if t is None else t.data_ptr() + 4 * elem
        for p, o in zip(self.param_groups[0]["params"], self._offs):
            g = m = v = None
            if grads:
                if p.grad is None:
                    continue  # like torch: parameters without a gradient are skipped
                g, m, v = p.grad, self._m, self._v
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise ValueError(f"{type(self).__name__} needs contiguous fp32 gradients")
            n = p.numel()
            for s in range(0, n, TQ_ADAM_CHUNK):
                yield at(p, s), at(g, s), at(m, o + s), at(v, o + s), at(self._ema, o + s), min(TQ_ADAM_CHUNK, n - s)

    def _upload(self, rows):
        """rows -> (the device table of ``TqAdamChunk``, their number)"""
        rows = list(rows)
        arr = (TqAdamChunk * len(rows))(*(TqAdamChunk(*r) for r in rows))
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self._m.device), len(rows)

    def _build_table(self):
        """the step's table, rebuilt when a parameter or its gradient has moved"""
        ps = self.param_groups[0]["params"]
        key = tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in ps)
        if key != self._table_key:
            self._table, self._n_chunks = self._upload(self._rows(grads=True))
            self._table_key = key
            self._norm_buf = None   # (sized by the table)
            self._updated = [p for p in ps if p.grad is not None]

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0, skip_flag: Optional[torch.Tensor] = None,
             max_grad_norm: Optional[float] = None, clip_value: Optional[float] = None, track_grad_norm: bool = False):
        """``skip_flag``: device int32 tensor; when it is non-zero at execution time the launch changes nothing (the range guard
        of the fp16-range forward scheme, see tq_adam_ema_step_guarded) -- decided on the device, no host synchronisation; the
        host-side step count advances all the same.

        ``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` on the scaled gradients ``grad_scale * g``,
        inside the launch: two small launches in front of it form the total 2-norm (fp64 partial sums per chunk, fixed order) and
        the coefficient ``min(1, max_grad_norm / (norm + 1e-6))`` on the device; the update multiplies it in.  ``p.grad`` itself is
        left as it was.  ``clip_value``: ``clip_grad_value_`` the same way (a clamp in the launch, no extra launch).  One of the
        two at most, like Lightning's ``gradient_clip_algorithm``.  ``track_grad_norm``: form the norm without clipping.
        Whenever the norm is formed, ``last_grad_norm`` is a device fp32 scalar holding it (of the scaled gradient, before
        clipping; a view of a buffer the next such step overwrites; never synchronised here).  ``skip_flag`` keeps its meaning: a
        raised flag drops the whole update, and the norm of such a step may be inf.  With none of the three given the step issues
        exactly the launch it always did."""
        self._check_step_args(max_grad_norm, clip_value)
        loss = closure() if closure is not None else None
        self._build_table()
        self._step += 1
        t = self._step
        if self._n_chunks:
            ema_w = 0.0 if self.ema_decay is None else 1.0 - self.ema_decay
            stream = torch.cuda.current_stream(self._m.device).cuda_stream
            clip = None   # (device pointer of the norm-clipping coefficient | None, clip_value | 0.0)
            if max_grad_norm is not None or track_grad_norm:
                clip = self._form_norm(grad_scale, max_grad_norm, stream)
            if clip_value is not None:
                clip = (None, float(clip_value))
            self._launch(t, self.param_groups[0], ema_w, grad_scale, None if skip_flag is None else skip_flag.data_ptr(), stream,
                         clip)
        # the kernel wrote the parameters through raw pointers: bump their autograd version counters so that everything keyed
        # on ``p._version`` (the engines' packed MFMA weight fragments, engine.py repack / repack_transposed) sees the update
        torch._C._increment_version(self._updated)
        self._step_t.fill_(float(t))
        return loss

    def _check_step_args(self, max_grad_norm, clip_value):
        """the refusals in front of everything else (they read no instance state: ``ema_swapped`` is a class attribute)"""
        if max_grad_norm is not None and clip_value is not None:
            raise ValueError("max_grad_norm and clip_value are alternatives (gradient_clip_algorithm 'norm' or 'value'): give one")
        for name, val in (("max_grad_norm", max_grad_norm), ("clip_value", clip_value)):
            if val is not None and not val > 0:
                raise ValueError(f"{name} must be positive, got {val!r}")
        if self.ema_swapped:
            raise RuntimeError("the parameters hold the EMA weights (swap_ema / DataParallelTrainer.ema_weights): a step now would "
                               "update the EMA as if it were the weights; swap back first")

    def _form_norm(self, grad_scale, max_grad_norm, stream):
        """The two small launches that form ``[norm, coefficient]`` of the current table's gradients; ``last_grad_norm`` becomes a
        view of the first.  Returns the launch's ``clip``: the second's address when ``max_grad_norm`` clips, None when it only tracks."""
        if self._norm_buf is None:
            self._norm_buf = (torch.empty(self._n_chunks, dtype=torch.float64, device=self._m.device),
                              torch.empty(2, dtype=torch.float32, device=self._m.device))
        partials, out = self._norm_buf
        check(self._lib.tq_grad_sumsq(self._table.data_ptr(), self._n_chunks, partials.data_ptr(), stream), "grad_sumsq")
        check(self._lib.tq_grad_clip_coef(partials.data_ptr(), self._n_chunks, grad_scale, max_grad_norm or 0.0,
                                          out.data_ptr(), stream), "grad_clip_coef")
        self.last_grad_norm = out[0]
        return (out.data_ptr() + 4, 0.0) if max_grad_norm is not None else None

    def _launch(self, t, g, ema_w, grad_scale, skip_ptr, stream, clip=None):
        guarded, clipped, what = self._entry
        args = (self._table.data_ptr(), self._n_chunks, *self._scalars(t, g, ema_w, grad_scale), skip_ptr)
        if clip is None:
            check(getattr(self._lib, guarded)(*args, stream), what)
        else:
            check(getattr(self._lib, clipped)(*args, clip[0], clip[1], stream), what + " (clipped)")

    # ------------------------------------------------------------------ (de)serialisation in torch Adam's format
    def state_dict(self):
        """torch's format, with a ``step`` tensor of its own per parameter: the one shared scalar kept here would stay shared through
        ``torch.save`` / ``deepcopy``, and torch's Adam, loading it, would then count every step once per parameter."""
        sd = super().state_dict()
        sd["state"] = {k: dict(st, step=st["step"].clone()) for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        ps = self.param_groups[0]["params"]
        st = state_dict["state"]
        steps = set()
        for i, p in enumerate(ps):
            if i in st:
                self.state[p]["exp_avg"].copy_(st[i]["exp_avg"])
                self.state[p]["exp_avg_sq"].copy_(st[i]["exp_avg_sq"])
                steps.add(int(float(st[i]["step"])))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ; the fused update keeps one")
        self._step = steps.pop() if steps else 0
        self._step_t.fill_(float(self._step))
        for k, v in state_dict["param_groups"][0].items():
            if k in ("lr", "betas", "eps", "initial_lr", "weight_decay"):
                self.param_groups[0][k] = v


class FusedAdamEMA(_FusedFlatOptimizer):
    """``weight_decay`` > 0 gives torch.optim.AdamW (decoupled decay), the autoencoder's optimizer (autoencoder.py:93-95)."""

    _entry = ("tq_adam_ema_step_guarded", "tq_adam_ema_step_clipped", "adam")

    def _scalars(self, t, g, ema_w, grad_scale):
        b1, b2 = g["betas"]
        step_size = g["lr"] / (1.0 - b1 ** t)
        ibc2 = 1.0 / math.sqrt(1.0 - b2 ** t)
        return step_size, b1, b2, g["eps"], ibc2, ema_w, grad_scale, 1.0 - g["lr"] * g["weight_decay"]


def radam_scalars(t: int, lr: float, b1: float, b2: float):
    """(step size lr / (1 - b1^t), rect) of torch.optim.RAdam's step ``t`` in double, as torch's single-tensor path forms them:
    rect = r_t * sqrt(1 - b2^t) where rho_t > 5, else 0 = the un-rectified update p -= step_size * m."""
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho_t = rho_inf - 2.0 * t * (b2 ** t) / bc2
    rect = 0.0
    if rho_t > 5.0:
        rect = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) * math.sqrt(bc2)
    return lr / bc1, rect


class FusedRAdamEMA(_FusedFlatOptimizer):
    """torch.optim.RAdam with its defaults (weight_decay=0, decoupled_weight_decay=False, maximize=False) + the EMA lerp."""

    def __init__(self, named_params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, ema_decay: Optional[float] = None,
                 weight_decay: float = 0.0):
        if weight_decay != 0:
            raise ValueError("FusedRAdamEMA implements torch.optim.RAdam without weight decay (the consistency model's optimizer)")
        super().__init__(named_params, lr=lr, betas=betas, eps=eps, ema_decay=ema_decay, weight_decay=0.0)

    _entry = ("tq_radam_ema_step_guarded", "tq_radam_ema_step_clipped", "radam")

    def _scalars(self, t, g, ema_w, grad_scale):
        b1, b2 = g["betas"]
        step_size, rect = radam_scalars(t, g["lr"], b1, b2)
        return step_size, b1, b2, g["eps"], rect, ema_w, grad_scale
