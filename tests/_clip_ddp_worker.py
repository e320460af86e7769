"""Worker of tests/test_grad_clip_gpu.py::test_two_rank_clipped_training_reproduces_the_full_batch_run (one process per rank; launched
with RANK / WORLD_SIZE / MASTER_* / TQ_TEST_BACKEND set, as tests/_ddp_worker.py is).

Real model, real kernels: the micro EDM UNet on a fixed global batch of 8 x 3 x 256 with the step's two draws injected.  One rank
trains two steps on the full batch with ``gradient_clip_val`` on; then the ranks train two steps on their halves.  The norm the fused
optimizer forms is that of the MEAN gradient (behind the exchange, with the 1 / world_size of the launch folded in), so both runs see
the same norm, clip by the same coefficient and end at the same parameters.  The learning rate is the reference's (1e-4, every script
under its experiments/): Adam moves an element whose gradient is summation noise -- the B = 4 and B = 8 plans round differently, and the
column sums use atomics -- by up to the learning rate per step whatever the noise's size, so the parameter comparison scales with it; at
1e-3 two runs of this worker measured 6.5e-6 and 9.5e-6 over the flat vector against the bar of 1e-5, with clipping playing no part in
the spread (the norms agreed to 6e-7).  With fewer GPUs than ranks the ranks share cuda:0 and the
exchange goes over gloo, which the trainer stages through host memory."""

import json

import torch
import torch.distributed as dist

from _ddp_launch import gather, init_rank

CLIP = 0.05   # below the gradient norm of both steps (asserted by the test from the norms reported here)


def main():
    rank, world, dev, backend = init_rank()

    from conftest import cfg_of, load_golden, rel_err
    from tqdne_amd import LightningEDM, rng
    from tqdne_amd.autograd import edm_loss_and_grads
    from tqdne_amd.trainer import DataParallelTrainer, shard_batch

    sd, d = load_golden("micro_unet.npz")
    cfg = dict(cfg_of(d), dropout=0.0)  # masks are indexed by the position in the LOCAL batch: equivalence needs p = 0
    Bg, T, per = 8, 256, 8 // world
    g = torch.Generator().manual_seed(11)
    batch = {"signal": 0.5 * torch.randn(Bg, 3, T, generator=g), "cond": torch.randn(Bg, 5, generator=g)}
    eps_g, noise_g = torch.randn(Bg, generator=g), torch.randn(Bg, 3, T, generator=g)

    class InjectedEDM(LightningEDM):
        """step_and_backward with the two random draws of edm.py:126,128 taken from the fixed global draws"""
        inject = None

        def step_and_backward(self, batch, on_bucket=None, bucket_elems=4 << 20):
            eps, noise = self.inject
            return edm_loss_and_grads(self, batch["signal"].contiguous(), eps, noise, batch.get("cond"), on_bucket=on_bucket,
                                      bucket_elems=bucket_elems)

    def make():
        m = InjectedEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0})
        m.unet.load_state_dict(sd)
        return m.to(dev).train()

    def train(m, tr, local):
        norms = []
        for _ in range(2):
            tr.train_step(local)
            norms.append(tr.last_grad_norm.clone())   # (the scalar is a view of a buffer the next step overwrites)
        torch.cuda.synchronize()
        return torch.stack(norms).double().cpu()

    rng.seed_rank(0, rank)
    # reference: the full global batch on this rank alone
    full = make()
    full.inject = (eps_g.to(dev), noise_g.to(dev))
    tr_full = DataParallelTrainer(full, world_size=1, fused_optimizer=True, ema_decay=0.999, gradient_clip_val=CLIP)
    norms_full = train(full, tr_full, {k: v.to(dev) for k, v in batch.items()})

    m = make()
    m.inject = (eps_g[rank * per:(rank + 1) * per].to(dev), noise_g[rank * per:(rank + 1) * per].contiguous().to(dev))
    tr = DataParallelTrainer(m, world_size=world, bucket_bytes=64 << 10, overlap=True, fused_optimizer=True, ema_decay=0.999,
                             gradient_clip_val=CLIP)
    norms = train(m, tr, {k: v.to(dev) for k, v in shard_batch(batch, rank, world).items()})

    flat = lambda mod: torch.cat([p.detach().reshape(-1) for p in mod.unet.parameters()]).cpu()
    a, b = flat(m), flat(full)
    err = rel_err(a, b)
    worst, wname = 0.0, ""
    for (n, p_l), p_f in zip(m.unet.named_parameters(), full.unet.parameters()):   # per tensor, relative to that tensor's own scale
        e = float((p_l.detach() - p_f.detach()).abs().max()) / max(float(p_f.detach().abs().max()), 1e-30)
        if e > worst:
            worst, wname = e, n
    params, all_norms = gather(a), gather(norms)
    start = torch.cat([sd[k].reshape(-1) for k, _ in m.unet.named_parameters()])
    res = dict(clip=CLIP, norms=norms.tolist(), norms_full=norms_full.tolist(), err_flat=err, err_worst_tensor=worst,
               worst_tensor=wname, replicas_equal=bool(all(torch.equal(t, params[0]) for t in params)),
               norms_equal_across_ranks=bool(all(torch.equal(t, all_norms[0]) for t in all_norms)),
               moved=float((a - start).abs().max()), steps=int(tr.optimizer._step), buckets=list(tr.last_bucket_sizes))
    if rank == 0:
        print("DDP_RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
