"""Consistency-model training on the fused path (micro UNet of micro_unet.npz, B = 2, T = 256): ``step_and_backward`` against the
reference's own step (micro_cm_step.npz) and against ``step()`` + ``backward()``; the bucket hooks of its backward sweep;
DataParallelTrainer with the one-launch RAdam + EMA against torch.optim.RAdam applied to the trainer's own gradients, the iCT schedule
fed by ``max_steps=``; the range guard; two ranks."""

import os

import numpy as np
import pytest
import torch

from _ddp_launch import run_ranks
from conftest import GOLDEN, ROOT, cfg_of, load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3   # tests/test_hip_unet.py's bar for test_consistency_training_step_vs_reference


def dev():
    return torch.device("cuda:0")


def _model(dropout=None, **kw):
    from tqdne_amd import UNetModel
    from tqdne_amd.consistency_model import LithningConsistencyModel
    sd, d = load_golden("micro_unet.npz")
    cfg = cfg_of(d)
    if dropout is not None:   # (the golden net was taken without dropout)
        cfg = dict(cfg, dropout=dropout)
    net = UNetModel(**cfg)
    net.load_state_dict(sd)
    return LithningConsistencyModel(net, **kw).to(dev())


def _batch(seed=2, B=2, T=256):
    g = torch.Generator().manual_seed(seed)
    return {"signal": (0.5 * torch.randn(B, 3, T, generator=g)).to(dev()), "cond": torch.randn(B, 5, generator=g).to(dev())}


def test_step_and_backward_vs_reference_step():
    """loss and gradients of ``step_and_backward`` vs the reference's own iCT step (micro_cm_step.npz), its multinomial / randn_like
    draws injected, in eval mode as the golden was taken: the bounds of test_consistency_training_step_vs_reference.  ``p.grad`` of every
    parameter is a view into the returned flat buffer."""
    s = np.load(os.path.join(GOLDEN, "micro_cm_step.npz"))
    cm = _model().eval()
    net = cm.net
    cm.max_steps, cm.global_step = int(s["max_steps"]), int(s["global_step"])
    o_m, o_r = torch.multinomial, torch.randn_like
    seen = {}

    def mult(pdf, n, replacement=True):
        seen["pdf"] = pdf
        return torch.from_numpy(s["timesteps"]).to(dev())

    torch.multinomial, torch.randn_like = mult, (lambda t, **k: torch.from_numpy(s["eps"]).to(dev()))
    try:
        loss, flat = cm.step_and_backward({"signal": torch.from_numpy(s["sample"]).to(dev()), "cond": torch.from_numpy(s["cond"]).to(dev())})
    finally:
        torch.multinomial, torch.randn_like = o_m, o_r
    assert rel_err(seen["pdf"].cpu(), s["pdf"]) < 1e-5
    assert not loss.requires_grad and rel_err(loss.detach().cpu(), s["loss"]) < TOL
    grads = dict(net.named_parameters())
    gmax = float(s["gnorm"].max())
    for n, gn, gp in zip(s["gnames"], s["gnorm"], s["gproj"]):
        g = grads[str(n)].grad.reshape(-1).double().cpu()
        pat = torch.cos(torch.arange(g.numel(), dtype=torch.float64) * 0.37 + 0.1)
        assert abs(float(g.norm()) - gn) < 1e-3 * max(gn, 1e-3 * gmax), n
        assert abs(float((g * pat).sum()) - gp) < 1e-3 * max(gn, 1e-3 * gmax), n
    for k in s.files:
        if k.startswith("g:"):
            ref = torch.from_numpy(s[k])
            e = float((grads[k[2:]].grad.cpu() - ref).abs().max() / max(float(ref.abs().max()), 1e-3 * gmax))
            assert e < TOL, (k, e)
    # gradients live in the student plan's flat buffer
    B, T = s["sample"].shape[0], s["sample"].shape[2]
    bwd = net._engine(B, T, dev())._bwd
    assert flat.data_ptr() == bwd.flat.data_ptr()
    lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * bwd.n_grad
    spans = []
    for n, p in net.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, n
            continue
        assert p.grad is not None and p.grad.is_contiguous() and p.grad.shape == p.shape, n
        assert p.grad.data_ptr() == lo + 4 * bwd.offs[id(p)] and p.grad.data_ptr() + 4 * p.numel() <= hi, n
        spans.append((p.grad.data_ptr(), p.numel()))
    spans.sort()
    assert all(a + 4 * n <= b for (a, n), (b, _) in zip(spans, spans[1:])), "views overlap"


def test_step_and_backward_equals_step_plus_backward_in_training_mode():
    """same seed, dropout on: the loss of ``step()`` + ``backward()`` (rel 1e-6) and its gradients (1e-5: the column sums are summed by
    atomics, see test_bucket_callbacks_tile_the_buffer_and_fire_when_final)"""
    from tqdne_amd import rng
    cm = _model(dropout=0.1).train()
    assert cm.net.dropout > 0
    cm.max_steps, cm.global_step = 100, 0   # (no trainer: the schedule's progress comes from these attributes)
    batch = _batch()
    torch.manual_seed(3)
    rng.seed_rank(5, 0)
    loss = cm.step(batch)
    loss.backward()
    ref = {n: p.grad.clone() for n, p in cm.net.named_parameters() if p.grad is not None}
    for p in cm.net.parameters():
        p.grad = None
    torch.manual_seed(3)
    rng.seed_rank(5, 0)
    loss2, flat = cm.step_and_backward(batch)
    torch.cuda.synchronize()
    assert float(loss2) == pytest.approx(float(loss.detach()), rel=1e-6) and float(loss2) > 0
    assert len(ref) > 20
    bwd = cm.net._engine(2, 256, dev())._bwd
    flat_ref = torch.zeros_like(flat[:bwd.n_grad])
    for n, p in cm.net.named_parameters():
        if n in ref:
            o = bwd.offs[id(p)]
            flat_ref[o:o + p.numel()].copy_(ref[n].reshape(-1))
    assert rel_err(flat[:bwd.n_grad].cpu(), flat_ref.cpu()) < 1e-5


def test_bucket_callbacks_of_the_consistency_step():
    from tqdne_amd import rng
    cm = _model(dropout=0.1).train()
    cm.max_steps, cm.global_step = 100, 0
    batch = _batch()
    snaps = []

    def hook(sl):
        # a copy enqueued right behind the finalising launch: any later write to the slice would make it differ from the end state
        snaps.append((sl.data_ptr(), sl.numel(), sl.clone()))

    torch.manual_seed(3)
    rng.seed_rank(5, 0)
    loss, flat = cm.step_and_backward(batch, on_bucket=hook, bucket_elems=8192)
    torch.cuda.synchronize()
    bwd = cm.net._engine(2, 256, dev())._bwd
    assert len(snaps) >= 4
    pos = flat.data_ptr()
    for ptr, n, snap in snaps:  # contiguous, in order, covering [0, n_grad)
        assert ptr == pos
        off = (ptr - flat.data_ptr()) // 4
        assert torch.equal(snap, flat[off:off + n]), "bucket was modified after its callback"
        pos += 4 * n
    assert (pos - flat.data_ptr()) // 4 == bwd.n_grad
    # buckets of the output blocks' half leave before the sweep ends
    fire, late = bwd._fire_points(8192)
    assert len(fire) >= 3 and min(fire) < len(bwd.ops) // 2


def test_trainer_fused_radam_ema_and_ict_schedule():
    """8 fused train steps with max_steps=6, initial_timesteps=10, final_timesteps=40: the schedule has 11, 21, 41 points at steps 0-1,
    2-3, 4+.  After every step one torch.optim.RAdam step on the CPU with the trainer's own gradients: the device parameters track
    that copy to 1e-6 per tensor (optimizer parity; gradient parity is the tests above), the EMA the lerp recurrence over it."""
    from tqdne_amd import rng
    from tqdne_amd.optim import FusedRAdamEMA
    from tqdne_amd.trainer import DataParallelTrainer
    cm = _model(dropout=0.1, initial_timesteps=10, final_timesteps=40, lr=1e-3).train()
    tr = DataParallelTrainer(cm, world_size=1, fused_optimizer=True, ema_decay=0.9, max_steps=6)
    assert isinstance(tr.optimizer, FusedRAdamEMA) and tr.scheduler is None
    named = [(n, p) for n, p in cm.named_parameters() if p.requires_grad]
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for _, p in named]
    opt = torch.optim.RAdam(cpu, lr=1e-3)
    ema = [p.detach().clone() for p in cpu]
    lengths = []
    schedule = cm._schedule

    def recording():
        sig = schedule()
        lengths.append(int(sig.numel()))
        return sig

    cm._schedule = recording
    torch.manual_seed(1)
    rng.seed_rank(7, 0)
    batch = _batch(9)
    for step in range(8):
        loss = tr.train_step(batch)
        assert torch.isfinite(loss)
        for c, (n, p) in zip(cpu, named):
            c.grad = p.grad.detach().cpu().clone()
        opt.step()
        torch._foreach_lerp_(tuple(ema), tuple(c.detach() for c in cpu), 1 - 0.9)
        for c, (n, p) in zip(cpu, named):
            assert rel_err(p.detach().cpu(), c.detach()) < 1e-6, (step, n)
    assert lengths == [11, 11, 21, 21, 41, 41, 41, 41]
    assert tr.optimizer._step == 8 and tr.optimizer.param_groups[0]["lr"] == 1e-3
    state = tr.ema_state()
    assert list(state) == [n for n, _ in named]
    for (n, e), er in zip(state.items(), ema):
        assert rel_err(e.cpu(), er) < 1e-6, n
    start, _ = load_golden("micro_unet.npz")
    assert any(not torch.equal(p.detach().cpu(), start[n[len("net."):]]) for n, p in named)


def test_raised_range_flag_drops_the_step_on_the_device():
    """the trainer finds the consistency model's network under ``net``: with the model's range-guard flag raised (plainly: no kernel is
    provoked) the optimizer launch leaves parameters, moments and EMA as they were"""
    from tqdne_amd import rng
    from tqdne_amd.engine import shared_range_flag
    from tqdne_amd.trainer import DataParallelTrainer
    cm = _model(dropout=0.1, initial_timesteps=10, final_timesteps=40, lr=1e-3).train()
    tr = DataParallelTrainer(cm, world_size=1, fused_optimizer=True, ema_decay=0.9, max_steps=6)
    rng.seed_rank(7, 0)
    batch = _batch(9)
    for _ in range(2):
        tr.train_step(batch)
    torch.cuda.synchronize()
    flag = shared_range_flag(cm.net, dev())
    assert int(flag.item()) == 0 and tr.last_skip is flag
    opt = tr.optimizer
    snap = lambda: [p.detach().clone() for p in cm.parameters()] + [opt._m.clone(), opt._v.clone(), opt._ema.clone()]
    before = snap()
    flag.fill_(1)
    tr.train_step(batch)
    torch.cuda.synchronize()
    assert tr.last_skip is flag
    for a, b in zip(snap(), before):
        assert torch.equal(a, b)
    assert opt._step == 3 and tr.steps_done == 3   # the host-side bookkeeping moves on


@pytest.mark.timeout(600)
def test_two_rank_consistency_training():
    """two ranks on a global batch of 4 x 3 x 256 (tests/_cm_ddp_worker.py): the reduced gradients are the one-rank full-batch gradients
    (tests/test_ddp_gpu.py's bars), and after 7 fused RAdam steps the replicas are bit-equal"""
    res = run_ranks("_cm_ddp_worker.py", timeout=400)
    for mode in ("overlap", "after"):
        r = res[mode]
        assert r["err_flat"] < 1e-5 and r["err_worst_tensor"] < 5e-4, (mode, r)  # (B = 2 and B = 4 plans round differently)
        assert r["replicas_equal"] and r["finite"] and r["steps"] == 7 and r["moved"] > 0, (mode, r)
        assert abs(r["loss_mean"] - r["loss_full"]) < 1e-5 * abs(r["loss_full"]), (mode, r)
    assert len(res["overlap"]["buckets"]) >= 3 and res["overlap"]["tail_words"] == 2   # the range-guard pair rides in the last bucket
    assert len(res["after"]["buckets"]) >= 1 and res["after"]["tail_words"] == 0
