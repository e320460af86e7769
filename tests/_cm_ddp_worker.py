"""Worker of tests/test_cm_trainer_gpu.py::test_two_rank_consistency_training (one process per rank; launched with RANK / WORLD_SIZE /
MASTER_* / TQ_TEST_BACKEND set, as tests/_ddp_worker.py is).

Real model, real kernels: every rank trains the micro consistency model on its shard of a fixed global batch of 4 x 3 x 256 with the
step's two draws (per-sample timesteps, epsilon) injected; after the exchange the gradients must equal the one-rank full-batch
gradients, with and without the overlap of the exchange with the backward sweep, and after 7 steps of the fused RAdam (across the
switch to the rectified update at t = 6, and across the growth of the iCT schedule) all replicas must hold identical weights.
With fewer GPUs than ranks the ranks share cuda:0 and the exchange goes over gloo, which the trainer stages through host memory."""

import json

import torch
import torch.distributed as dist

from _ddp_launch import gather, init_rank


def main():
    rank, world, dev, backend = init_rank()

    from conftest import cfg_of, load_golden, rel_err
    from tqdne_amd import UNetModel, rng
    from tqdne_amd.consistency_model import LithningConsistencyModel
    from tqdne_amd.optim import FusedRAdamEMA
    from tqdne_amd.trainer import DataParallelTrainer, shard_batch

    sd, d = load_golden("micro_unet.npz")
    cfg = dict(cfg_of(d), dropout=0.0)  # masks are indexed by the position in the LOCAL batch: equivalence needs p = 0
    Bg, T, per = 4, 256, 4 // world
    g = torch.Generator().manual_seed(11)
    batch = {"signal": 0.5 * torch.randn(Bg, 3, T, generator=g), "cond": torch.randn(Bg, 5, generator=g)}
    ts_g = torch.randint(0, 10, (Bg,), generator=g)   # (valid for every length of the schedule: 11, 21, 41 points)
    eps_g = torch.randn(Bg, 3, T, generator=g)

    # the step's two draws (consistency_model.py:141-148), injected as tests/test_hip_unet.py injects them
    inject = {}
    torch.multinomial = lambda pdf, n, replacement=True: inject["timesteps"]
    torch.randn_like = lambda t, **k: inject["eps"]

    def make():
        net = UNetModel(**cfg)
        net.load_state_dict(sd)
        return LithningConsistencyModel(net, initial_timesteps=10, final_timesteps=40, lr=1e-3).to(dev).train()

    rng.seed_rank(0, rank)
    res = {}
    # reference: the full global batch on this rank alone, at the progress the trainer publishes for its first step
    full = make()
    full._dp_progress = (0, 6)
    inject.update(timesteps=ts_g.to(dev), eps=eps_g.to(dev))
    loss_full, flat_full = full.step_and_backward({k: v.to(dev) for k, v in batch.items()})
    bwd_full = full.net._engine(Bg, T, dev)._bwd
    g_full = flat_full[:bwd_full.n_grad].clone()
    offs_full = bwd_full.offs

    for overlap in (True, False):
        m = make()
        local = {k: v.to(dev) for k, v in shard_batch(batch, rank, world).items()}
        inject.update(timesteps=ts_g[rank * per:(rank + 1) * per].to(dev), eps=eps_g[rank * per:(rank + 1) * per].contiguous().to(dev))
        tr = DataParallelTrainer(m, world_size=world, bucket_bytes=64 << 10, overlap=overlap, fused_optimizer=True, max_steps=6,
                                 ema_decay=0.9)
        assert isinstance(tr.optimizer, FusedRAdamEMA) and tr.scheduler is None
        # first step: capture the reduced gradients in front of the optimizer launch
        opt_step = tr.optimizer.step
        grabbed = {}

        def hold(grad_scale=1.0, skip_flag=None, _m=m):
            bwd = _m.net._engine(per, T, dev)._bwd
            grabbed["g"] = (bwd.flat[:bwd.n_grad] * grad_scale).clone()
            grabbed["offs"] = dict((id(p), bwd.offs[id(p)]) for p in _m.net.parameters())
            return opt_step(grad_scale=grad_scale, skip_flag=skip_flag)

        tr.optimizer.step = hold
        loss = tr.train_step(local)
        torch.cuda.synchronize()
        tr.optimizer.step = opt_step
        buckets, tail_words = list(tr.last_bucket_sizes), tr.last_tail_words
        # the two plans (B = 4 and B = 2) lay their gradients out identically (the layout depends on the model only)
        assert [grabbed["offs"][id(p)] for p in m.net.parameters()] == [offs_full[id(p)] for p in full.net.parameters()]
        err = rel_err(grabbed["g"].cpu(), g_full.cpu())
        # per tensor, relative to that tensor's own scale; tensors whose true gradient is zero (a conv bias in front of a
        # one-channel-per-group GroupNorm: the micro net has 32 channels) hold rounding noise only, hence the floor
        worst, floor = 0.0, 1e-4 * float(g_full.abs().max())
        for p_l, p_f in zip(m.net.parameters(), full.net.parameters()):
            if not p_l.requires_grad:
                continue
            o = offs_full[id(p_f)]
            a, b = grabbed["g"][o:o + p_l.numel()], g_full[o:o + p_l.numel()]
            worst = max(worst, float((a - b).abs().max()) / max(float(b.abs().max()), floor))
        losses = gather(torch.tensor([float(loss)], dtype=torch.float64))
        # six more steps: t = 7, the rectified update from t = 6, the schedule at 11, 21 and 41 points
        for _ in range(6):
            tr.train_step(local)
        torch.cuda.synchronize()
        params = gather(torch.cat([p.detach().reshape(-1) for p in m.net.parameters()]))
        emas = gather(torch.cat([e.reshape(-1) for e in tr.ema_state().values()]))
        start = torch.cat([v.reshape(-1) for v in (sd[k] for k, _ in m.net.named_parameters())])
        res["overlap" if overlap else "after"] = dict(
            err_flat=err, err_worst_tensor=worst, buckets=buckets, tail_words=tail_words,
            replicas_equal=bool(all(torch.equal(t, params[0]) for t in params) and all(torch.equal(t, emas[0]) for t in emas)),
            moved=float((params[0] - start).abs().max()), steps=int(tr.optimizer._step),
            finite=bool(torch.isfinite(params[0]).all()),
            loss_mean=float(sum(l.item() for l in losses) / world), loss_full=float(loss_full))
    if rank == 0:
        print("DDP_RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
