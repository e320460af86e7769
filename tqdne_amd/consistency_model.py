"""Consistency model: drop-in for ``tqdne.consistency_model`` (reference tqdne/consistency_model.py:63-190): forward / sample
(63-106) and the iCT training step (115-176: teacher at sigma_t without gradient, student at sigma_{t+1}, weighted pseudo-Huber
distance).  The network is a ``tqdne_amd.UNetModel``; the consistency skip/out scalings are folded into the head-conv epilogue,
and the raw sigma is the network's timestep (line 77).  Both UNet passes of the training step and its backward are HIP;
``step_and_backward`` is the form ``DataParallelTrainer`` drives (flat gradient buffer, bucket hooks, one-launch RAdam + EMA)."""

from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib, engine, rng
from ._lib import _p, check
from ._cache import scratch_cache
from .autograd import loss_backward
from .edm import network_input, retry_on_range
from .lightning_compat import LightningModule


def ict_loss_forward(module, sample, sigmas, timesteps, epsilon, cond, cond_sample, lane=0):
    """loss = mean(w_t * (sqrt((f(x + s_{t+1} eps, s_{t+1}) - sg[f(x + s_t eps, s_t)])^2 + c^2) - c)),  c = 0.00054 sqrt(dim)
    (consistency_model.py:140-176) on the plan and buffers of ``lane``.  Returns (loss, the plan that holds the student's activations,
    d loss / d pred).  The teacher runs first on the same plan: the student's forward overwrites what it left, so only the student
    has a backward."""
    engine.require_device(sample)
    B = sample.shape[0]
    seed = rng.next_dropout_seed()  # one seed: teacher = student masks
    train = module.training
    lib = _lib.load()
    dev = sample.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    t_sig, s_sig = sigmas[timesteps].float().contiguous(), sigmas[timesteps + 1].float().contiguous()
    per = sample[0].numel()
    key = ("ict", tuple(sample.shape), str(dev), lane)
    bufs = module._scal.get(key)
    if bufs is None:
        bufs = dict(xt=torch.empty_like(sample), xs=torch.empty_like(sample), target=torch.empty_like(sample),
                    dpred=torch.empty_like(sample), loss=torch.empty(1, device=dev))
        module._scal[key] = bufs
    epsilon = epsilon.contiguous()
    # the two noised copies (consistency_model.py:150-160), teacher first (no gradient, same dropout masks as the student)
    check(lib.tq_axpy_sigma(_p(sample), _p(epsilon), _p(t_sig), _p(bufs["xt"]), B, per, stream), "noise (teacher)")
    check(lib.tq_axpy_sigma(_p(sample), _p(epsilon), _p(s_sig), _p(bufs["xs"]), B, per, stream), "noise (student)")
    # (a conditioning signal is concatenated behind both noised copies, consistency_model.py:63-66,111-118; it gets no gradient)
    bufs["target"].copy_(module._forward_static(bufs["xt"], t_sig, cond, lane=lane, train=train, dropout_seed=seed,
                                                cond_sample=cond_sample))
    eng = module.net._engine(B, sample.shape[2], dev, lane)
    with eng.hold_range_poll():   # (the range guard treats the step as one: a flag the teacher raised is acted on before the next step)
        pred = module._forward_static(bufs["xs"], s_sig, cond, lane=lane, train=train, dropout_seed=seed, cond_sample=cond_sample)
    c = 0.00054 * float(np.sqrt(np.prod(sample.shape[2:])))
    w = (1 / (sigmas[1:] - sigmas[:-1]))[timesteps].float().contiguous()   # (B,) weights: indexing glue, as the schedule
    check(lib.tq_pseudo_huber_loss(_p(pred), _p(bufs["target"]), _p(w), c, _p(bufs["loss"]), _p(bufs["dpred"]), B, per, stream),
          "pseudo-Huber loss")
    # (the plan stays with the caller: a later look-up could find a NEW plan if the bounded cache evicted this one in between)
    return bufs["loss"][0].clone(), eng, bufs["dpred"]


class _ICTLossFn(torch.autograd.Function):
    """``ict_loss_forward`` on lane 0 under autograd."""

    @staticmethod
    def forward(ctx, module, sample, sigmas, timesteps, epsilon, cond, cond_sample, *params):
        loss, ctx.eng, ctx.dpred = ict_loss_forward(module, sample, sigmas, timesteps, epsilon, cond, cond_sample)
        ctx.fwd_id = ctx.eng._fwd_count
        return loss

    @staticmethod
    def backward(ctx, gloss):
        return loss_backward(ctx, gloss, 7)


class LithningConsistencyModel(LightningModule):  # (sic) the reference's class name
    def __init__(self, net, sigma_min=0.002, sigma_max=80.0, rho=7.0, sigma_data=0.5, initial_timesteps=10,
                 final_timesteps=1280, lognormal_mean=-1.1, lognormal_std=2.0, lr=1e-4):
        super().__init__()
        if getattr(net, "dims", 1) != 1:
            raise NotImplementedError("the consistency model runs on the 1-D HIP path (every reference config that uses it is 1-D)")
        self.net = net
        self.sigma_min, self.sigma_max, self.rho, self.sigma_data = sigma_min, sigma_max, rho, sigma_data
        self.initial_timesteps, self.final_timesteps = initial_timesteps, final_timesteps
        self.lognormal_mean, self.lognormal_std, self.lr = lognormal_mean, lognormal_std, lr
        self._scal = scratch_cache()

    def _forward_static(self, sample, sigma, cond, lane=0, train=False, dropout_seed=0, infer=False, cond_sample=None):
        """``cond_sample``: conditioning signal concatenated on the channel axis behind the sample (consistency_model.py:63-66): the
        network sees the concatenation, the skip term the sample alone."""
        lib = _lib.load()
        B, _, T = sample.shape
        dev = sample.device
        key = (B, str(dev), lane)
        sc = self._scal.get(key)
        if sc is None:
            sc = torch.empty(2, B, device=dev)
            self._scal[key] = sc
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib.tq_cm_scalars(_p(sigma), 1, float(self.sigma_data), float(self.sigma_min), _p(sc[0]), _p(sc[1]), B, stream),
              "cm scalars")
        eng = self.net._engine(B, T, dev, lane)
        x_in, _, cond_x = network_input(eng, self._scal, lane, sample, None, cond_sample)
        return eng.forward(x_in, sigma, cond, in_scale=None, c_out=sc[0], c_skip=sc[1], skip_src=sample, train=train,
                           dropout_seed=dropout_seed, infer=infer, cond_x=cond_x)

    def forward(self, sample, sigma, cond_sample=None, cond=None, _check_range=True):
        """consistency_model.py:63-79."""
        engine.require_device(sample)
        sample, sigma = sample.contiguous(), sigma.contiguous().float()
        if cond_sample is not None:
            cond_sample = cond_sample.contiguous().float()
        B = sample.shape[0]
        lanes = 1  # one forward cannot amortise 4x the launches (measured 8.3 vs 6.5 ms at B = 64); kept for TQDNE experiments
        if os.environ.get("TQDNE_CM_LANES"):
            lanes = int(os.environ["TQDNE_CM_LANES"])
        if lanes > 1 and (B % lanes or torch.is_grad_enabled()):
            lanes = 1
        if lanes < 2:
            infer = not torch.is_grad_enabled()
            eng = self.net._engine(B, sample.shape[2], sample.device) if infer and _check_range else None   # (None: no flag read)
            return retry_on_range(eng, lambda: self._forward_static(sample, sigma, cond, infer=infer, cond_sample=cond_sample).clone())
        # independent samples: sub-batches on separate HIP streams run out of phase (see LightningEDM.sample_deterministically)
        out = torch.empty_like(sample[:, : self.net.out_channels])
        with engine.lane_fanout(sample.device, B, lanes) as fan:
            for i, st in enumerate(fan.streams):
                with torch.cuda.stream(st):
                    y = self._forward_static(fan.cut(sample, i), fan.cut(sigma, i), fan.cut(cond, i), lane=engine.CONCURRENT_LANE0 + i,
                                             infer=True, cond_sample=fan.cut(cond_sample, i))
                    out[fan.rows(i)].copy_(y)
        return out

    @torch.no_grad()
    def sample(self, shape, sigmas=[1.0], cond_sample=None, cond=None):
        """consistency_model.py:81-106 (the refinement noise is uniform, ``rand_like``, as in the reference)."""
        epsilon = torch.randn(shape, device=self.device)
        return self.sample_from(epsilon, sigmas, [torch.rand_like(epsilon) for _ in sigmas], cond_sample, cond)

    @torch.no_grad()
    def sample_from(self, epsilon, sigmas, uniform_noises, cond_sample=None, cond=None):
        def run():
            ones = torch.ones(epsilon.shape[0], device=epsilon.device)
            sample = self(epsilon, ones * self.sigma_max, cond_sample, cond, _check_range=False)
            for sigma, u in zip(sigmas, uniform_noises):
                sample = sample + u * sigma
                sample = self(sample, ones * sigma, cond_sample, cond, _check_range=False)
            return sample
        # range guard: ONE flag read per sample call (as the EDM samplers do), not one per network evaluation
        return retry_on_range(lambda: self.net._engine(epsilon.shape[0], epsilon.shape[2], epsilon.device), run)

    # ------------------------------------------------------------------ iCT training (consistency_model.py:115-190)
    def _schedule(self):
        """consistency_model.py:121-138.  Progress comes, in this order, from ``self._dp_progress = (global_step, max_steps)``, which
        ``DataParallelTrainer(max_steps=...)`` sets before every step (training without Lightning); from Lightning's
        ``trainer.max_steps`` / ``global_step``; without a trainer from the attributes ``max_steps`` / ``global_step`` of the module."""
        progress = getattr(self, "_dp_progress", None)
        if progress is not None:
            global_step, max_steps = progress
        else:
            tr = getattr(self, "trainer", None)
            max_steps = tr.max_steps if tr is not None else getattr(self, "max_steps", 1)
            global_step = getattr(self, "global_step", 0)
        prime = np.floor(max_steps / (np.log2(np.floor(self.final_timesteps / self.initial_timesteps)) + 1))
        num = self.initial_timesteps * 2 ** np.floor(global_step / prime)
        num = min(num, self.final_timesteps) + 1
        rho_inv = 1.0 / self.rho
        steps = torch.arange(num, device=self.device) / (num - 1)
        sig = self.sigma_min**rho_inv + steps * (self.sigma_max**rho_inv - self.sigma_min**rho_inv)
        return sig**self.rho

    def step(self, batch):
        """A single step of training or validation (consistency_model.py:115-176): teacher at sigma_t (no gradient, same
        dropout masks as the student), student at sigma_{t+1}, weighted pseudo-Huber distance.  Both UNet passes and the
        backward are HIP; the schedule, the (B,)-sized draws and the loss on the (B, C, T) outputs are torch glue."""
        sample, sigmas, pdf, timesteps, epsilon, cond, cond_sample = self._step_inputs(batch)
        return _ICTLossFn.apply(self, sample, sigmas, timesteps, epsilon, cond, cond_sample, *self.net.parameters())

    def _step_inputs(self, batch):
        """(sample, sigmas, pdf, timesteps, epsilon, cond, cond_sample) of one training step: the schedule and the two draws of
        consistency_model.py:121-148, in the reference's order.  The caller holds on to all of them, ``pdf`` included, until the step's
        launches are enqueued and lets them go in this order, as ``step`` always has: the caching allocator then hands the small
        temporaries of this and of later calls the same blocks as before, which keeps the launch listings of tools/plan_listing.py
        comparable line by line."""
        sample = batch["signal"]
        cond_sample, cond = batch.get("cond_signal"), batch.get("cond")
        if cond_sample is not None:
            cond_sample = cond_sample.detach().contiguous().float()
        sigmas = self._schedule()
        z = lambda s_: torch.erf((torch.log(s_) - self.lognormal_mean) / (self.lognormal_std * np.sqrt(2)))
        pdf = z(sigmas[1:]) - z(sigmas[:-1])
        pdf = pdf / pdf.sum()
        timesteps = torch.multinomial(pdf, sample.shape[0], replacement=True)
        epsilon = torch.randn_like(sample)
        return sample.contiguous(), sigmas, pdf, timesteps, epsilon, cond, cond_sample

    def step_and_backward(self, batch, on_bucket=None, bucket_elems: int = 4 << 20, tail_fill=None):
        """``step`` + backward in one call, without the autograd round trip: gradients are left in ``p.grad`` of the network's
        parameters, views of the student plan's flat buffer, which is returned as well: (loss, flat).  One lane.
        ``on_bucket``: gradient-exchange hook, called as buckets of the flat buffer become final (BackwardPlan.run);
        ``tail_fill``: extra words of the caller that ride at the end of the last bucket (BackwardPlan.run)."""
        params = list(self.net.parameters())
        with torch.no_grad():
            sample, sigmas, pdf, timesteps, epsilon, cond, cond_sample = self._step_inputs(batch)
            loss, eng, dpred = ict_loss_forward(self, sample, sigmas, timesteps, epsilon, cond, cond_sample)
            one = torch.ones((), device=dpred.device)
            grads = eng.backward(dpred, one, clone=False, on_bucket=on_bucket, bucket_elems=bucket_elems, tail_fill=tail_fill)
            for p, g in zip(params, grads):
                if g is not None and (p.grad is None or p.grad.data_ptr() != g.data_ptr()):
                    p.grad = g
        return loss, eng._bwd.flat

    def training_step(self, batch, batch_idx: int):
        loss = self.step(batch)
        self.log("train_loss", loss.item(), prog_bar=True)
        return loss

    def validation_step(self, batch, batch_idx: int):
        loss = self.step(batch)
        self.log("val_loss", loss.item())
        return loss

    def configure_optimizers(self):
        return torch.optim.RAdam(self.net.parameters(), lr=self.lr)

    def evaluate(self, batch, sigmas=[1]):
        sample = batch["signal"]
        return self.sample(sample.shape, sigmas, batch.get("cond_signal"), batch.get("cond"))
