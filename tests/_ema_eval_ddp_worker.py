"""Worker of tests/test_ema_eval_gpu.py::test_two_ranks_validate_to_the_same_value_on_equal_ema_weights (one process per rank; launched
with RANK / WORLD_SIZE / MASTER_* / TQ_TEST_BACKEND set, as tests/_clip_ddp_worker.py is).

Real model, real kernels: the micro EDM UNet.  The ranks train two steps on their halves of a global batch (own noise draws per rank,
gradients exchanged: the replicas and their EMAs stay equal), then ``validate`` on DIFFERENT batches -- other sizes, another number of
them -- with their own draws.  Reported: the value of every rank; the same sum formed by hand (every rank repeats its own validation
steps on a fresh module holding the EMA, with the same seed, and the (sum of loss * B, sum of B) pairs are gathered); the parameters of
the ranks inside and after ``ema_weights()``.  With fewer GPUs than ranks the ranks share cuda:0 and the exchange goes over gloo, which
the trainer stages through host memory."""

import json

import torch
import torch.distributed as dist

from _ddp_launch import gather, init_rank


def main():
    rank, world, dev, backend = init_rank()

    from conftest import cfg_of, load_golden
    from tqdne_amd import LightningEDM, rng
    from tqdne_amd.trainer import DataParallelTrainer, shard_batch

    sd, d = load_golden("micro_unet.npz")
    cfg = dict(cfg_of(d), dropout=0.0)

    def make():
        m = LightningEDM(cfg, {"learning_rate": 2e-3, "max_steps": 10, "eta_min": 0.0})
        m.unet.load_state_dict(sd)
        return m.to(dev).train()

    def batch_of(B, seed):
        g = torch.Generator().manual_seed(seed)
        return {"signal": (0.5 * torch.randn(B, 3, 256, generator=g)).to(dev), "cond": torch.randn(B, 5, generator=g).to(dev)}

    def same_on_all_ranks(t):
        ts = gather(t)
        return bool(all(torch.equal(x.view(torch.int32), ts[0].view(torch.int32)) for x in ts))

    flat = lambda mod: torch.cat([p.detach().reshape(-1) for p in mod.parameters() if p.requires_grad])

    rng.seed_rank(0, rank)
    m = make()
    tr = DataParallelTrainer(m, world_size=world, bucket_bytes=64 << 10, fused_optimizer=True, ema_decay=0.9)
    local = shard_batch(batch_of(4 * world, 11), rank, world)
    for _ in range(2):
        tr.train_step(local)
    w0 = flat(m).clone()
    ema0 = {k: v.detach().clone() for k, v in tr.ema_state().items()}
    ema_flat = torch.cat([ema0[n].reshape(-1) for n, p in m.named_parameters() if p.requires_grad])

    mine = [batch_of(2, 40), batch_of(3, 41)] if rank == 0 else [batch_of(4, 42), batch_of(2, 43), batch_of(3, 44)]
    torch.manual_seed(50 + rank)
    value = tr.validate(mine)
    values = gather(value.reshape(1).double())

    fresh = make()
    fresh.load_state_dict(m.state_dict())
    fresh.load_state_dict(ema0, strict=False)
    fresh.eval()
    torch.manual_seed(50 + rank)
    with torch.no_grad():
        pair = torch.tensor([sum(float(fresh.validation_step(b, i)) * b["signal"].shape[0] for i, b in enumerate(mine)),
                             float(sum(b["signal"].shape[0] for b in mine))], dtype=torch.float64)
    total = sum(gather(pair))

    with tr.ema_weights():
        inside = flat(m).clone()
        inside_equal = same_on_all_ranks(inside)
    after = flat(m).clone()
    res = dict(value=float(value), values_equal=bool(all(torch.equal(v, values[0]) for v in values)),
               by_hand=float(total[0] / total[1]), batches_seen=float(total[1]),
               inside_equal=inside_equal, inside_is_ema=bool(torch.equal(inside, ema_flat)), after_equal=same_on_all_ranks(after),
               restored=bool(torch.equal(after.view(torch.int32), w0.view(torch.int32))),
               ema_differs=not bool(torch.equal(ema_flat, w0)), steps=int(tr.optimizer._step), training=bool(m.training))
    if rank == 0:
        print("DDP_RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
