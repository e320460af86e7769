"""Consistency-model training on the fused path, the part that needs no GPU: the one-launch RAdam entry point is declared, exported
and bound; FusedRAdamEMA's refusals; DataParallelTrainer with a module whose ``configure_optimizers`` returns a BARE
optimizer (the reference's consistency model returns ``torch.optim.RAdam(...)``, consistency_model.py:178-190): no scheduler, torch
RAdam's exact trajectory, ``max_steps=`` published to the module; two gloo ranks against one-rank full-batch training."""

import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_radam_entry_point_is_declared_exported_and_bound():
    from tqdne_amd import _build, _lib
    _build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tqdne_hip.h")).read()
    assert re.search(r"\bint\s+tq_radam_ema_step_guarded\s*\(\s*const TqAdamChunk\*", header)
    assert "tq_radam_ema_step_guarded" in _lib.exported_symbols() and hasattr(lib, "tq_radam_ema_step_guarded")
    assert lib.tq_abi_version() == _lib.ABI_VERSION
    # a null table / an empty one is refused before the device is touched (this box has none)
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 1.0, None, None)
    assert lib.tq_radam_ema_step_guarded(None, 4, *args) == -1   # TQ_ERR_ARG
    table = (_lib.TqAdamChunk * 1)()
    import ctypes as C
    assert lib.tq_radam_ema_step_guarded(C.cast(table, C.c_void_p), 0, *args) == -1
    assert lib.tq_radam_ema_step_guarded(C.cast(table, C.c_void_p), -3, *args) == -1


def test_fused_radam_refuses_cpu_parameters_and_weight_decay():
    from tqdne_amd.optim import FusedAdamEMA, FusedRAdamEMA, _FusedFlatOptimizer
    assert issubclass(FusedRAdamEMA, _FusedFlatOptimizer) and issubclass(FusedAdamEMA, _FusedFlatOptimizer)
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(RuntimeError, match="GPU"):
        FusedRAdamEMA([("p", p)], lr=1e-3)
    with pytest.raises(ValueError, match="weight decay"):
        FusedRAdamEMA([("p", p)], lr=1e-3, weight_decay=1e-4)


def test_radam_scalars_follow_torch_branch():
    """the host-side scalars: un-rectified (rect = 0) through t = 5, rectified from t = 6 with the default betas (rho_5 = 4.996, rho_6 =
    5.994); with betas (0.8, 0.9), rho_inf = 19"""
    from tqdne_amd.optim import radam_scalars
    rect = [radam_scalars(t, 1e-3, 0.9, 0.999)[1] for t in range(1, 10)]
    assert all(r == 0.0 for r in rect[:5]) and all(r > 0.0 for r in rect[5:])
    step, _ = radam_scalars(3, 1e-3, 0.9, 0.999)
    assert step == pytest.approx(1e-3 / (1 - 0.9 ** 3), rel=1e-15)
    t, b2 = 7, 0.9
    rho_inf = 2 / (1 - b2) - 1
    assert rho_inf == pytest.approx(19.0)
    rho_t = rho_inf - 2 * t * b2 ** t / (1 - b2 ** t)
    want = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5 * (1 - b2 ** t) ** 0.5
    assert radam_scalars(t, 1e-3, 0.8, b2)[1] == pytest.approx(want, rel=1e-14)


class _StubCM(torch.nn.Module):
    """CPU stand-in for the consistency model as the trainer sees it: network under ``net``, ``configure_optimizers`` returns a bare
    torch.optim.RAdam, flat gradient buffer laid out in reverse parameter order, buckets released from inside the "backward" like
    BackwardPlan.run.  Records the progress the trainer publishes."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.SiLU(), torch.nn.Linear(32, 32), torch.nn.SiLU(),
                                       torch.nn.Linear(32, 4))
        self.lr = 1e-2
        ps = list(self.parameters())[::-1]
        self._offs, total = {}, 0
        for p in ps:
            self._offs[id(p)] = total
            total += p.numel()
        self.n_grad = total
        self.flat = torch.zeros(total + 2)   # (+ the two tail words of BackwardPlan's layout, engine_bwd.TAIL_WORDS)
        self.progress_seen = []

    def configure_optimizers(self):
        return torch.optim.RAdam(self.net.parameters(), lr=self.lr)

    def step_and_backward(self, batch, on_bucket=None, bucket_elems=1 << 20, tail_fill=None):
        self.progress_seen.append(getattr(self, "_dp_progress", None))
        self.flat.zero_()
        loss = ((self.net(batch["signal"]) - batch["cond"]) ** 2).mean()
        grads = torch.autograd.grad(loss, list(self.parameters()))
        for p, g in zip(self.parameters(), grads):
            o = self._offs[id(p)]
            self.flat[o:o + p.numel()].copy_(g.reshape(-1))
            p.grad = self.flat[o:o + p.numel()].view_as(p)
        if on_bucket is not None:
            n = self.n_grad
            for lo in range(0, n, bucket_elems):
                hi = min(lo + bucket_elems, n)
                if hi == n and tail_fill is not None:
                    tail_fill(self.flat[n:n + 2])
                    hi = n + 2
                on_bucket(self.flat[lo:hi])
        return loss.detach(), self.flat[:self.n_grad]


def _batches(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [{"signal": torch.randn(8, 16, generator=g), "cond": torch.randn(8, 4, generator=g)} for _ in range(n)]


def test_trainer_takes_a_bare_radam_and_follows_torch_radam_exactly():
    from tqdne_amd.trainer import DataParallelTrainer
    steps = _batches(8)
    m = _StubCM()
    tr = DataParallelTrainer(m, world_size=1, fused_optimizer=False)
    assert tr.scheduler is None and type(tr.optimizer) is torch.optim.RAdam
    for b in steps:
        tr.train_step(b)
    assert m.progress_seen == [None] * 8   # (no max_steps: nothing is published)
    assert tr.optimizer.param_groups[0]["lr"] == m.lr   # no scheduler moved it
    # the hand-rolled loop: loss, autograd, torch RAdam
    ref = _StubCM()
    opt = torch.optim.RAdam(ref.net.parameters(), lr=ref.lr)
    for b in steps:
        opt.zero_grad()
        ((ref.net(b["signal"]) - b["cond"]) ** 2).mean().backward()
        opt.step()
    for (n, p), q in zip(m.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), n
    assert int(next(iter(tr.optimizer.state.values()))["step"]) == 8   # across the rectification switch (t = 6)


def test_trainer_publishes_progress_for_the_ict_schedule():
    from tqdne_amd.trainer import DataParallelTrainer
    m = _StubCM()
    tr = DataParallelTrainer(m, world_size=1, fused_optimizer=False, max_steps=6)
    for b in _batches(8):
        tr.train_step(b)
    assert m.progress_seen == [(k, 6) for k in range(8)]
    assert tr.steps_done == 8


def test_ict_schedule_reads_the_published_progress_first():
    """``_dp_progress`` wins over the module's own ``max_steps`` / ``global_step`` attributes; without it the old lookup holds"""
    from tqdne_amd import UNetModel, tiny_1d_unet_config
    from tqdne_amd.consistency_model import LithningConsistencyModel
    cm = LithningConsistencyModel(UNetModel(**tiny_1d_unet_config()), initial_timesteps=10, final_timesteps=40)
    cm.max_steps, cm.global_step = 6, 0
    assert cm._schedule().numel() == 11
    cm.global_step = 2
    assert cm._schedule().numel() == 21
    for k, want in zip(range(8), (11, 11, 21, 21, 41, 41, 41, 41)):
        cm._dp_progress = (k, 6)
        assert cm._schedule().numel() == want, k
    del cm._dp_progress
    assert cm._schedule().numel() == 21


def test_trainer_keeps_other_optimizers_unfused():
    """fused path requested, but the module configures neither Adam(W) nor RAdam: the optimizer stays as configured"""
    from tqdne_amd.trainer import DataParallelTrainer

    class SGDStub(_StubCM):
        def configure_optimizers(self):
            return torch.optim.SGD(self.net.parameters(), lr=0.1)

    m = SGDStub()
    tr = DataParallelTrainer(m, world_size=1, fused_optimizer=True, ema_decay=0.5)
    assert not tr.fused and type(tr.optimizer) is torch.optim.SGD
    before = [p.detach().clone() for p in m.parameters()]
    tr.train_step(_batches(1)[0])
    for (n, e), p, b in zip(tr.ema_state().items(), m.parameters(), before):
        assert torch.allclose(e, b + 0.5 * (p.detach() - b)), n


def _gloo_worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tqdne_amd.trainer import DataParallelTrainer, shard_batch

    steps = _batches(8)

    def run(world_size, **kw):
        m = _StubCM()
        if world_size > 1 and rank != 0:  # replicas that start different must be overwritten by rank 0's broadcast
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(1.0)
        tr = DataParallelTrainer(m, world_size=world_size, fused_optimizer=False, max_steps=6, **kw)
        sizes = []
        for b in steps:
            tr.train_step(shard_batch(b, rank, world_size) if world_size > 1 else b)
            sizes.append(list(tr.last_bucket_sizes))
        return torch.cat([p.detach().reshape(-1) for p in m.parameters()]), sizes

    ref, _ = run(1)                                             # full batch, one rank, torch RAdam
    a, sizes_a = run(world, bucket_bytes=4 * 300, overlap=True)   # many small buckets, issued from inside the backward
    b, sizes_b = run(world, bucket_bytes=4 * 300, overlap=False)  # same buckets, issued after the backward
    c, sizes_c = run(world, bucket_bytes=1 << 20, overlap=True)   # one bucket
    gathered = [torch.zeros_like(a) for _ in range(world)]
    dist.all_gather(gathered, a)
    ok = (torch.allclose(a, ref, atol=1e-6) and torch.equal(a, b) and torch.allclose(c, ref, atol=1e-6)
          and len(sizes_a[0]) > 3 and len(sizes_c[0]) == 1 and sum(sizes_a[0]) == sum(sizes_c[0])
          and all(torch.equal(t, gathered[0]) for t in gathered))
    ret[rank] = bool(ok)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_gloo_world2_bare_radam_matches_full_batch_training():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_gloo_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert all(ret[r] for r in range(world))
