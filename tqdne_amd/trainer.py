"""Data-parallel training loop for the EDM module, the autoencoder and the consistency model: stands where Lightning's fit loop +
DDPStrategy stand in the reference (experiments/train_1d_edm.py:34-70): one process per GPU, identical replicas, the batch is
sharded by rank, gradients are summed with RCCL all-reduce over xGMI (torch.distributed backend "nccl") and divided
by the world size, then every rank applies the same Adam + per-step cosine LR update (edm.py:240-251) -- or, for the consistency
model, the same RAdam update without a scheduler (consistency_model.py:178-190).

The exchange is overlapped with the backward, the way torch's DDP reducer does it for the reference: the backward plan lays
the flat gradient buffer out in the order its reverse sweep finalises the gradients (head, output blocks, middle block,
input blocks, stem, embedding MLPs) and calls back as each contiguous bucket becomes final; the bucket's all-reduce is
issued right there (asynchronously: on RCCL's own stream, ordered behind the launches enqueued so far) and runs under the
rest of the sweep.  Only the optimizer launch waits for the exchange.  Every rank cuts and issues the buckets identically
(the cut depends on the model and ``bucket_bytes`` only), so the collectives match up by construction.

The rest of the fit loop: ``ema_weights()`` is the second half of the reference's EMA callback (tqdne/ema.py:30-48: EMA weights into the
module before every validation / test / predict pass, the training weights back afterwards), ``validate`` / ``evaluate`` run
``validation_step`` / ``evaluate`` under it, ``save_checkpoint`` / ``load_checkpoint`` write and resume the Lightning layout of
checkpoint.py, and ``fit`` is the thin loop over all of it with ModelCheckpoint's ``last.ckpt`` + best ``save_top_k`` (training.py:54-65).
"""

from __future__ import annotations

import contextlib
import inspect
import os

import torch
import torch.distributed as dist

from . import checkpoint, rng
from .engine import leave_fp16_range_scheme, reserve_side_streams, shared_range_flag


def init_process_group(backend: str = "nccl", device=None, **kw):
    """``torch.distributed.init_process_group`` with the one ordering rule this package has on ROCm: the sampler lanes and the
    backward's weight-gradient stream make their first submission BEFORE the RCCL communicator creates its streams.  ROCm binds a
    HIP stream to a hardware queue at its first submission; with the communicator in first, the backward's two streams share a
    queue and the training step of the paper UNet runs 22.1 -> 28.1 ms (measured with a forced one-rank exchange,
    ``profiles/r04_u_rccl_ab.txt``).  Extra keywords go to torch (``rank``, ``world_size``, ``timeout``, ``device_id`` ...)."""
    if device is not None and torch.device(device).type == "cuda":
        reserve_side_streams(torch.device(device))
    return dist.init_process_group(backend, **kw)


def _flats(flat) -> list:
    """a flat gradient buffer, or a list of them (the autoencoder step returns per-tensor gradients), as a list"""
    return list(flat) if isinstance(flat, (list, tuple)) else [flat]


def allreduce_mean_(flat, world_size: int, bucket_elems: int = 8 << 20, scale: bool = True):
    """In-place mean of ``flat`` over all ranks: a few large bucketed all-reduces (RCCL over xGMI on GPUs, gloo in the
    CPU tests), launched asynchronously and waited together, then one scale.  62 MB of gradients = 2 buckets of 32 MB."""
    if world_size <= 1:
        return flat
    flats = _flats(flat)
    works = []
    for f in flats:
        f1 = f.view(-1)
        works += [dist.all_reduce(f1[i:i + bucket_elems], op=dist.ReduceOp.SUM, async_op=True)
                  for i in range(0, f1.numel(), bucket_elems)]
    for w in works:
        w.wait()
    if scale:
        for f in flats:
            f.mul_(1.0 / world_size)
    return flat


def shard_batch(batch: dict, rank: int, world_size: int) -> dict:
    """Rank ``rank``'s slice of a global batch (what Lightning's DistributedSampler does for the reference)."""
    if world_size <= 1:
        return batch
    out = {}
    for k, v in batch.items():
        n = v.shape[0]
        assert n % world_size == 0, "global batch must divide evenly over the ranks"
        per = n // world_size
        out[k] = v[rank * per:(rank + 1) * per]
    return out


class _Done:
    """handle of a collective that has already completed (host-staged gloo exchange)"""

    def wait(self):
        return True


class _ForeachEMA:
    """The EMA of a run on a torch optimizer, behind the surface the one-launch optimizers have for theirs (optim.py: ``ema_state``,
    ``load_ema_state``, ``swap_ema``) plus the per-step ``lerp`` that those do inside their launch."""

    def __init__(self, module, decay: float):
        self.decay = decay
        self.params = [p for p in module.parameters() if p.requires_grad]
        self.ema = {n: p.detach().clone() for n, p in module.named_parameters() if p.requires_grad}
        self.saved = None   # the training weights while the module holds the EMA (between two ``swap_ema()`` calls)

    @torch.no_grad()
    def lerp(self):
        torch._foreach_lerp_(tuple(self.ema.values()), tuple(self.params), 1 - self.decay)

    def ema_state(self):
        return self.ema   # (``swap_ema`` copies it into the module and leaves the dict alone: always the EMA of the run)

    def load_ema_state(self, src):
        for n, t in self.ema.items():
            t.copy_(src[n])

    @torch.no_grad()
    def swap_ema(self):
        """EMA weights into the module, or the training weights back: ``torch._foreach_copy_`` through one list of clones"""
        if self.saved is None:
            self.saved = [p.detach().clone() for p in self.params]
            torch._foreach_copy_(self.params, list(self.ema.values()))
        else:
            torch._foreach_copy_(self.params, self.saved)
            self.saved = None


class DataParallelTrainer:
    def __init__(self, module, world_size: int = 1, bucket_bytes: int = 16 << 20, ema_decay=None, fused_optimizer=None,
                 overlap: bool = True, process_group=None, force_exchange: bool = False, max_steps=None,
                 gradient_clip_val=None, gradient_clip_algorithm: str = "norm", track_grad_norm: bool = False):
        """``gradient_clip_val`` / ``gradient_clip_algorithm``: ``pl.Trainer``'s two gradient options, which the reference passes
        through ``trainer_params``: ``"norm"`` = ``clip_grad_norm_(params, val)``, ``"value"`` = ``clip_grad_value_(params, val)``,
        applied to the mean gradient over the ranks (behind the exchange and its 1 / world_size), so every rank clips alike.  None
        or 0: no clipping.  Fused optimizer: decided on the device inside the optimizer launch (optim.py), no host synchronisation;
        ``p.grad`` keeps the unclipped sum.  Otherwise torch's functions on the optimizer's parameters.
        ``track_grad_norm``: form the total gradient norm without clipping.  Whenever the norm is formed (``"norm"`` clipping or
        tracking) ``last_grad_norm`` holds it after ``train_step``: the norm of the mean gradient BEFORE clipping, identical on every
        rank; a device fp32 scalar on the fused path (read it when you log: reading synchronises), torch's returned norm otherwise.
        The range guard keeps its meaning: a step whose flag is raised is dropped whole, clipped or not, and its ``last_grad_norm``
        may be inf.
        ``max_steps``: length of the run for modules whose training step depends on its progress (the consistency model's iCT
        schedule, which under Lightning reads ``trainer.max_steps`` / ``global_step``): when given, ``module._dp_progress =
        (steps done so far, max_steps)`` is set before every ``step_and_backward``.  None: nothing is published.
        ``force_exchange``: issue the collectives with ONE rank too (a sum over one rank is the identity: the self-test of the
        RCCL path on a 1-GPU box -- communicator, RCCL's stream behind the sweep's launches, the waits in front of the optimizer).
        ``ema_decay``: keep the EMA weights of the reference's EMA callback (tqdne/ema.py; 0.999 in the reference's runs).
        ``fused_optimizer``: one-launch Adam / AdamW / RAdam (+ EMA) instead of torch's; default: on GPUs.  An optimizer of any
        other class is kept as the module configured it (with the foreach-lerp EMA).
        ``overlap``: issue each gradient bucket's all-reduce from inside the backward sweep (default) instead of after it.
        ``bucket_bytes``: 16 MB = 4 buckets over the paper UNet's 62 MB of gradients (xGMI rings are per-link bound: few,
        large messages; the first bucket leaves after the output blocks' half of the sweep)."""
        self.module = module
        self.world = world_size
        self.group = process_group
        self.overlap = overlap
        self.exchange = world_size > 1 or force_exchange
        cfg = module.configure_optimizers()
        if isinstance(cfg, torch.optim.Optimizer):   # a bare optimizer (the consistency model's RAdam): no LR scheduler
            self.optimizer, self.scheduler = cfg, None
        else:
            self.optimizer = cfg["optimizer"]
            self.scheduler = cfg["lr_scheduler"]["scheduler"]
        on_gpu = next(module.parameters()).device.type == "cuda"
        self.fused = on_gpu if fused_optimizer is None else fused_optimizer
        self.ema_decay = ema_decay
        self.max_steps = max_steps
        self.steps_done = 0
        if gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm={gradient_clip_algorithm!r}: expected 'norm' or 'value'")
        if gradient_clip_val is not None and not gradient_clip_val >= 0:
            raise ValueError(f"gradient_clip_val must be None or >= 0, got {gradient_clip_val!r}")
        self.gradient_clip_val = float(gradient_clip_val) if gradient_clip_val else None
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self.track_grad_norm = bool(track_grad_norm)
        self.last_grad_norm = None
        # (exact classes: a subclass may change the update)
        kind = type(self.optimizer)
        if self.fused and kind not in (torch.optim.Adam, torch.optim.AdamW, torch.optim.RAdam):
            self.fused = False
        if self.fused:
            from .optim import FusedAdamEMA, FusedRAdamEMA
            g = self.optimizer.param_groups[0]
            self.optimizer = (FusedRAdamEMA if kind is torch.optim.RAdam else FusedAdamEMA)(
                self._named_optimized(g["params"]), lr=g["lr"], betas=g["betas"], eps=g["eps"], ema_decay=ema_decay,
                weight_decay=0.0 if kind is torch.optim.Adam else g.get("weight_decay", 0.0))
            if self.scheduler is not None:
                op = module.optimizer_params
                self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=op["max_steps"],
                                                                            eta_min=op["eta_min"])
        # the keeper of the EMA weights: the fused optimizer (its launch updates them), a _ForeachEMA beside a torch optimizer, or None
        self._ema = None if ema_decay is None else self.optimizer if self.fused else _ForeachEMA(module, ema_decay)
        self.bucket_elems = max(1, bucket_bytes // 4)
        sig = inspect.signature(module.step_and_backward).parameters
        self._hooked = "on_bucket" in sig
        self._tailed = "tail_fill" in sig   # the module lets a few words of ours ride at the end of the last gradient bucket
        self.last_bucket_sizes = []   # elements of each bucket exchanged by the last step, in issue order (diagnostics / tests)
        if self.exchange:
            self._broadcast_parameters()

    def _named_optimized(self, params):
        """(name, parameter) of the module's parameters, in the module's order; the configured optimizer must hold them all (both
        EDM's ``self.parameters()`` and the consistency model's ``self.net.parameters()`` do)."""
        named = list(self.module.named_parameters())
        held = {id(p) for p in params}
        missing = [n for n, p in named if p.requires_grad and id(p) not in held]
        if missing:
            raise ValueError(f"the module's optimizer leaves out trainable parameters ({missing[0]}, ...): not a case the fused "
                             "optimizer handles; pass fused_optimizer=False")
        return named

    def _network(self):
        """the module's 1-D network, whose range-guard flag the optimizer launch is predicated on: ``unet`` (EDM) or ``net`` (the
        consistency model); None for modules without one (autoencoder) and for dims=2 networks"""
        for name in ("unet", "net"):
            net = getattr(self.module, name, None)
            if net is not None:
                return net if getattr(net, "dims", 1) == 1 else None
        return None

    # ------------------------------------------------------------------ exchange
    def _broadcast_parameters(self):
        """Replicas start identical (DDP's initial broadcast): rank 0's parameters go out as ONE flat buffer per dtype
        (round 4 issued one collective per tensor: 311 for the paper UNet) and are copied back in place on the parameters themselves
        (not p.data), so that their version counters move and the packed weights follow."""
        with torch.no_grad():
            by_dtype = {}
            for p in self.module.parameters():
                by_dtype.setdefault(p.dtype, []).append(p)
            for ps in by_dtype.values():
                flat = torch.cat([p.detach().reshape(-1) for p in ps])
                if self._host_staged(flat):
                    h = flat.cpu()
                    dist.broadcast(h, src=0, group=self.group)
                    flat.copy_(h)
                else:
                    dist.broadcast(flat, src=0, group=self.group)
                torch._foreach_copy_(ps, [v.view_as(p) for v, p in zip(flat.split([p.numel() for p in ps]), ps)])

    def _host_staged(self, t: torch.Tensor) -> bool:
        """device tensors over the gloo backend (the dry-run configuration of bench.py / the 1-GPU tests: ranks sharing a device) go
        through host memory: the product backend for GPUs is "nccl" = RCCL, which takes device tensors as they are"""
        return t.is_cuda and dist.get_backend(self.group) == "gloo"

    def _allreduce_async(self, t: torch.Tensor):
        """start the sum all-reduce of ``t`` (in place); returns a handle with ``wait()``.  NCCL/RCCL: the collective is
        enqueued on the process group's own stream behind everything the current stream holds so far."""
        if self._host_staged(t):
            h = t.cpu()   # (synchronises: the slice is final on the current stream at this point)
            dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
            t.copy_(h)
            return _Done()
        return dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True, group=self.group)

    def train_step(self, batch):
        """loss, backward (HIP) with the gradient exchange riding under it, Adam, cosine LR.  Returns the local loss (a device
        scalar; no host sync here -- the reference's ``loss.item()`` logging, edm.py:138, belongs to the caller)."""
        if self._ema_active:
            raise RuntimeError("train_step inside ema_weights(): the module holds the EMA weights; leave the context first")
        works = []
        self.last_bucket_sizes = []
        self.last_tail_words = 0      # words of ours that rode at the end of the last gradient bucket (the range-guard pair: 2)

        def issue(sl):
            self.last_bucket_sizes.append(sl.numel())
            works.append(self._allreduce_async(sl))
        hook = issue if self.exchange and self.overlap and self._hooked else None
        kw = dict(on_bucket=hook, bucket_elems=self.bucket_elems) if self._hooked else {}   # (what the module's signature takes)
        tail = None
        if hook is not None and self._tailed and not self._skip_done and self._local_range_flag()[0] is not None:
            # the range-guard pair of this step rides at the end of the last gradient bucket (no collective of its own)
            tail = []

            def tail_fill(words):
                self._skip_fill(words, *self._local_range_flag())
                tail.append(words)
                self.last_tail_words = words.numel()
            kw["tail_fill"] = tail_fill
        self._publish_progress()
        loss, flat = self.module.step_and_backward(batch, **kw)
        if self.exchange and hook is None:
            for f in _flats(flat):
                f1 = f.view(-1)
                for i in range(0, f1.numel(), self.bucket_elems):
                    issue(f1[i:i + self.bucket_elems])
        reduced = tail[0] if tail else None
        if reduced is None:
            skip = self._range_skip_flag()
        for w in works:   # (NCCL: makes the current stream wait for the exchange; the host does not block)
            w.wait()
        if reduced is not None:
            skip = self._range_skip_flag(reduced)   # (after the waits: every AGREE_EVERY steps the host reads the reduced pair)
        self.last_skip = skip
        if self.fused:
            # the 1 / world_size of the gradient mean rides in the optimizer launch
            clip = self._clip_kwargs()
            self.optimizer.step(grad_scale=1.0 / self.world, skip_flag=skip, **clip)
            if clip:
                self.last_grad_norm = self.optimizer.last_grad_norm
        else:
            if self.world > 1:
                for f in _flats(flat):
                    f.mul_(1.0 / self.world)
            self._clip_unfused()
            self.optimizer.step()
            if self._ema is not None:   # (the fused launch does this lerp itself)
                self._ema.lerp()
        if self.scheduler is not None:
            self.scheduler.step()
        self.steps_done += 1
        return loss

    def _publish_progress(self):
        """``module._dp_progress`` for modules whose step depends on the run's progress (``max_steps`` in ``__init__``)"""
        if self.max_steps is not None:
            self.module._dp_progress = (self.steps_done, self.max_steps)

    def _clip_kwargs(self) -> dict:
        """the clipping / tracking arguments of the fused optimizer's step; empty with the defaults: the same call and the same launches as without these options"""
        kw = {}
        if self.gradient_clip_val is not None:
            kw["max_grad_norm" if self.gradient_clip_algorithm == "norm" else "clip_value"] = self.gradient_clip_val
        if self.track_grad_norm:
            kw["track_grad_norm"] = True
        return kw

    def _clip_unfused(self):
        """torch's optimizer: torch's clipping functions on the gradients it is about to consume (the mean over the ranks)"""
        val, norm_alg = self.gradient_clip_val, self.gradient_clip_algorithm == "norm"
        if val is None and not self.track_grad_norm:
            return
        ps = [p for g in self.optimizer.param_groups for p in g["params"] if p.grad is not None]
        if val is not None and norm_alg:
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(ps, val)
            return
        if self.track_grad_norm:   # (before the clamp, like the fused path)
            with torch.no_grad():
                self.last_grad_norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in ps]))
        if val is not None:
            torch.nn.utils.clip_grad_value_(ps, val)

    AGREE_EVERY = 64   # steps between the (host-synchronous) checks whether every rank has left the fp16-range scheme
    _skip, _skip_steps, _skip_done = None, 0, False   # the exchange's state: the pair's buffer, steps so far, all ranks agreed to stop

    def _local_range_flag(self):
        """(device int32[1] range-guard flag of this rank's model | None, is this rank still on the fp16-range scheme?)"""
        unet = self._network()
        if not self.fused or unet is None:
            return None, False
        dev = next(self.module.parameters()).device
        return shared_range_flag(unet, dev), getattr(unet, "_conv_scheme", "auto") == "auto"

    def _range_skip_flag(self, reduced=None):
        """Device predicate of the optimizer launch (fused optimizer only): the range-guard flag of the fp16-range forward scheme.
        The host learns of a raised flag one or more steps late (engine._range_poll does not synchronise), so the step whose
        forward raised it -- activations within a factor two of the fp16 range, possibly inf / NaN gradients -- is dropped ON
        THE DEVICE, and so is every later step until the host has moved the plans to bf16x3.  With several ranks the flag is
        summed over the ranks first (a rank that skipped alone would leave the replicas different); a rank already on bf16x3
        contributes 0 (its kernels still raise the flag for large activations, which that scheme handles).

        Bookkeeping of a dropped step: only the device-side update is skipped.  The host-side counters move on -- Adam's step count
        (bias corrections), the cosine schedule, the parameters' version counters (one redundant re-pack) -- exactly as if the step had
        produced a zero update; at most a handful of steps per run are affected (the host switches the plans to bf16x3 within a
        step or two of the flag).

        The exchange ends by agreement: the second word of the exchanged pair counts the ranks that are off the fp16-range scheme;
        every ``AGREE_EVERY`` steps all ranks read it (the same step on every rank, so they stop together) and, once it equals the
        world size, no rank issues the collective any more.

        ``reduced`` (round 5): the pair already summed over the ranks -- it rode at the end of the step's last gradient bucket
        (``tail_fill`` of BackwardPlan.run), so the step has no collective of its own for it; None: the pair is exchanged here (modules
        without the bucket hook, ``overlap=False``)."""
        if reduced is None:
            flag, auto = self._local_range_flag()   # (read behind the step's forward, where a rank leaves the fp16-range scheme)
            if flag is None:
                return None
            if not self.exchange:
                return flag if auto else None
            if self._skip_done:
                return None
            # (summed as floats through the same exchange path as the gradients; the kernel tests word 0 for "non-zero", and a sum
            # of 0 / 1 flags has a non-zero bit pattern exactly when some rank raised its flag)
            if self._skip is None:
                self._skip = torch.zeros(2, dtype=torch.float32, device=flag.device)
            self._skip_fill(self._skip, flag, auto)
            self._allreduce_async(self._skip).wait()
            reduced = self._skip
        self._skip_steps += 1
        if self._skip_steps % self.AGREE_EVERY == 0 and float(reduced[1].item()) >= self.world:
            self._skip_done = True
        return reduced

    def _skip_fill(self, words, flag, auto):
        """this rank's pair into ``words`` (2 floats): [its range-guard flag while it is on the fp16-range scheme, 1 once it left it]"""
        if auto:
            words[0:1].copy_(flag)
            words[1:2].zero_()
        else:
            words[0:1].zero_()
            words[1:2].fill_(1.0)

    def ema_state(self):
        """name -> EMA weights, as the reference's EMA callback stores them in a checkpoint (tqdne/ema.py:50-51).  Always the EMA of
        the training run, also inside ``ema_weights()`` (fused path: views of the parameters then, where the swap put the values)."""
        if self._ema is None:
            raise RuntimeError("constructed without ema_decay")
        return self._ema.ema_state()

    # ------------------------------------------------------------------ validation / prediction on the EMA weights
    _ema_active = False   # inside ``ema_weights()``

    @contextlib.contextmanager
    def ema_weights(self):
        """The second half of the reference's EMA callback (tqdne/ema.py:30-48): inside the context the module holds the EMA weights,
        afterwards -- also when the body raises -- the training weights again; parameters and EMA are then bit for bit what they were.
        Fused optimizer: ``optimizer.swap_ema()`` twice, one small launch each, nothing copied or allocated (tq_ema_swap).  Otherwise
        ``torch._foreach_copy_`` through one temporary list.  Only the optimized / trainable parameters change (frozen parameters and
        buffers stay, like the reference's ``load_state_dict(ema_state, strict=False)``); the parameters' versions move, so the packed
        weights follow.  Not re-entrant; ``train_step``, ``save_checkpoint`` and ``load_checkpoint`` refuse to run inside it."""
        if self.ema_decay is None:
            raise RuntimeError("constructed without ema_decay")
        if self._ema_active:
            raise RuntimeError("ema_weights() is already active: the module holds the EMA weights (the context does not nest)")
        self._ema.swap_ema()
        self._ema_active = True
        try:
            yield self.module
        finally:
            self._ema_active = False
            self._ema.swap_ema()

    @contextlib.contextmanager
    def _eval_pass(self):
        """what Lightning sets up around a validation / predict pass: EMA weights when the trainer keeps an EMA, ``module.eval()``,
        ``torch.no_grad()``; every submodule's mode is put back afterwards (a frozen autoencoder stays in eval mode)"""
        modes = [(m, m.training) for m in self.module.modules()]
        weights = self.ema_weights() if self.ema_decay is not None else contextlib.nullcontext()
        try:
            with weights, torch.no_grad():
                self.module.eval()
                yield
        finally:
            for m, mode in modes:
                m.training = mode

    def validate(self, batches, limit_batches=None):
        """One validation pass (Lightning's validation loop + the EMA callback): ``module.validation_step(batch, i)`` for every batch
        (the first ``limit_batches`` if given) on the EMA weights when the trainer keeps an EMA, in eval mode, without gradients.
        Returns sum(loss_i * B_i) / sum(B_i) with B_i = batch["signal"].shape[0] as a device scalar; with several ranks both sums go
        over the ranks in ONE collective of two words -- for equally sized batches Lightning's ``sync_dist=True`` epoch mean, the value
        the reference's ModelCheckpoint monitors (training.py:54-65).  Every rank returns the same value."""
        dev = next(self.module.parameters()).device
        acc = torch.zeros(2, dtype=torch.float64, device=dev)   # [sum of loss * B, sum of B]
        with self._eval_pass():
            for i, batch in enumerate(batches):
                if limit_batches is not None and i >= limit_batches:
                    break
                self._publish_progress()
                loss = self.module.validation_step(batch, i)
                B = batch["signal"].shape[0]
                acc[0] += loss.detach().to(torch.float64) * B
                acc[1] += B
        if self.world > 1:
            self._allreduce_async(acc).wait()
        return (acc[0] / acc[1]).float()

    def evaluate(self, batch):
        """``module.evaluate(batch)`` -- the samples the reference's predict loop and LogCallback draw -- under the conditions of
        ``validate``: EMA weights when there are any, eval mode, no gradients."""
        with self._eval_pass():
            return self.module.evaluate(batch)

    # ------------------------------------------------------------------ checkpoints, resuming
    EXTRA_KEY = "tqdne_amd_trainer"   # our one top-level key in a checkpoint; a reference loader ignores it

    def save_checkpoint(self, path, epoch: int = 0):
        """``checkpoint.save_checkpoint`` (the Lightning layout: a reference loader reads it) of the module, the EMA, the optimizer in
        torch's format, the scheduler and ``global_step = steps_done``, plus what only this trainer needs to continue exactly where it
        stopped, under ``EXTRA_KEY``: the dropout call counter, the conv scheme of the module's 1-D network and ``steps_done``."""
        if self._ema_active:
            raise RuntimeError("save_checkpoint inside ema_weights(): the module holds the EMA weights; leave the context first")
        net = self._network()
        extra = {self.EXTRA_KEY: {"dropout_counter": rng.dropout_counter(), "steps_done": self.steps_done,
                                  "conv_scheme": None if net is None else getattr(net, "_conv_scheme", "auto")}}
        checkpoint.save_checkpoint(self.module, path, ema_state=self.ema_state() if self.ema_decay is not None else None,
                                   optimizer=self.optimizer, lr_scheduler=self.scheduler, epoch=epoch, global_step=self.steps_done, extra=extra)

    def load_checkpoint(self, path):
        """Put module, optimizer, EMA, scheduler and step count back where ``save_checkpoint`` -- or the reference's ModelCheckpoint --
        left them (``trainer.fit(..., ckpt_path=...)``).  The weights are copied in place, so the parameters' versions move and the
        packed weights follow.  A checkpoint without ``ema_state`` starts the EMA from the loaded weights (the callback's
        ``on_fit_start``); one without our key (written by the reference) continues at ``steps_done = global_step``.  Returns the
        checkpoint dict."""
        if self._ema_active:
            raise RuntimeError("load_checkpoint inside ema_weights(): leave the context first")
        ckpt = checkpoint.load_checkpoint(path, map_location="cpu")
        self.module.load_state_dict(ckpt["state_dict"])
        if ckpt.get("optimizer_states"):
            self.optimizer.load_state_dict(ckpt["optimizer_states"][0])
        if self.ema_decay is not None:
            with torch.no_grad():
                self._ema.load_ema_state(ckpt.get("ema_state") or dict(self.module.named_parameters()))
        if self.scheduler is not None and ckpt.get("lr_schedulers"):
            self.scheduler.load_state_dict(ckpt["lr_schedulers"][0])
        ours = ckpt.get(self.EXTRA_KEY) or {}
        self.steps_done = int(ours.get("steps_done", ckpt.get("global_step", 0)))
        if "dropout_counter" in ours:
            rng.reset_dropout_counter(ours["dropout_counter"])
        net = self._network()
        if net is not None and ours.get("conv_scheme") == "bf16x3" and getattr(net, "_conv_scheme", "auto") == "auto":
            leave_fp16_range_scheme(net)   # (the run had left it: the plans that exist move, plans built from now on start there)
        return ckpt

    def fit(self, train_batches, val_batches=None, *, max_steps, val_check_interval=None, limit_val_batches=None, dirpath=None,
            save_top_k: int = 3, ckpt_path=None):
        """The loop ``pl.Trainer.fit`` runs for the reference (experiments/train_1d_edm.py; no logger, no callbacks): resume from
        ``ckpt_path`` if given, then ``train_step`` over ``train_batches`` (a re-iterable of this rank's batches, gone through as many
        times as it takes) until ``steps_done == max_steps``.  Every ``val_check_interval`` steps: ``validate(val_batches,
        limit_val_batches)`` and, with ``dirpath``, rank 0 writes ``last.ckpt`` and keeps the ``save_top_k`` checkpoints of lowest
        validation loss (ModelCheckpoint(monitor="validation/loss", mode="min", save_top_k=3, save_last=True), training.py:54-65),
        deleting the ones that drop out.  The host reads the validation loss there and nowhere else.  Returns the validation losses
        as [(steps_done, loss), ...]."""
        if ckpt_path is not None:
            self.load_checkpoint(ckpt_path)
        writer = dirpath is not None and (self.world <= 1 or dist.get_rank(self.group) == 0)
        if writer:
            os.makedirs(dirpath, exist_ok=True)
        kept, history, epoch = [], [], 0   # kept: (loss, path) of the top-k files, best first
        it = iter(train_batches)
        while self.steps_done < max_steps:
            try:
                batch = next(it)
            except StopIteration:
                epoch += 1
                it = iter(train_batches)
                batch = next(it)
            self.train_step(batch)
            if not val_check_interval or self.steps_done % val_check_interval:
                continue
            val = float(self.validate(val_batches, limit_val_batches)) if val_batches is not None else None
            history.append((self.steps_done, val))
            if not writer:
                continue
            self.save_checkpoint(os.path.join(dirpath, "last.ckpt"), epoch=epoch)
            if val is not None and save_top_k > 0 and (len(kept) < save_top_k or val < kept[-1][0]):
                path = os.path.join(dirpath, f"step={self.steps_done}-val_loss={val:.2e}.ckpt")
                self.save_checkpoint(path, epoch=epoch)
                kept = sorted(kept + [(val, path)], key=lambda lp: lp[0])
                for _, old in kept[save_top_k:]:
                    os.remove(old)
                kept = kept[:save_top_k]
        return history
