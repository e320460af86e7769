"""Fused RAdam + EMA launch (tq_radam_ema_step_guarded) against torch.optim.RAdam + torch._foreach_lerp_ on the CPU: the update the
reference's consistency model configures (tqdne/consistency_model.py:178-190).  Tolerance 1e-6 relative, the bar tests/test_optim.py
sets for the Adam launch: the same fp32 recurrences, scalars formed on the host in double.  9 steps cross the switch from the
un-rectified to the rectified form (default betas: rho_5 = 4.996, rho_6 = 5.994)."""

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 5), (3,), (32,), (256, 768), (5, 7, 3), (4097,), (1,), (130, 33)]   # tests/test_optim.py's


def _make(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * 0.3 for s in SHAPES]


def _named(ps):
    return [(f"p{i}", p) for i, p in enumerate(ps)]


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.9)])
def test_fused_radam_matches_torch_radam_and_ema_lerp(betas):
    from tqdne_amd.optim import FusedRAdamEMA, radam_scalars

    dev = torch.device("cuda:0")
    ref = [torch.nn.Parameter(t.clone()) for t in _make()]
    hip = [torch.nn.Parameter(t.clone().to(dev)) for t in _make()]
    opt_ref = torch.optim.RAdam(ref, lr=3e-3, betas=betas)
    opt = FusedRAdamEMA(_named(hip), lr=3e-3, betas=betas, ema_decay=0.9)
    ema_ref = [p.detach().clone() for p in ref]
    g = torch.Generator().manual_seed(7)
    rectified = []
    for step in range(9):
        for pr, ph in zip(ref, hip):
            gr = torch.randn(pr.shape, generator=g) * (10.0 ** (step % 5 - 2))   # gradients over several decades
            pr.grad = gr.clone()
            ph.grad = (gr * 4.0).to(dev)  # the launch folds the 1 / world_size of the gradient mean
        opt_ref.step()
        torch._foreach_lerp_(tuple(ema_ref), tuple(p.detach() for p in ref), 1 - 0.9)
        opt.step(grad_scale=0.25)
        rectified.append(radam_scalars(step + 1, 3e-3, *betas)[1] != 0.0)
        # every step, so that an error on one side of the switch cannot hide behind later steps
        for i, (pr, ph) in enumerate(zip(ref, hip)):
            assert rel_err(ph.detach().cpu(), pr.detach()) < 1e-6, (step, i)
    assert rectified[0] is False and rectified[-1] is True, "both forms of the update must have run"
    if betas == (0.9, 0.999):
        assert rectified == [False] * 5 + [True] * 4
    for i, (pr, ph) in enumerate(zip(ref, hip)):
        assert rel_err(opt.state[ph]["exp_avg"].cpu(), opt_ref.state[pr]["exp_avg"]) < 1e-6, i
        assert rel_err(opt.state[ph]["exp_avg_sq"].cpu(), opt_ref.state[pr]["exp_avg_sq"]) < 1e-6, i
    for (name, e), er in zip(opt.ema_state().items(), ema_ref):
        assert rel_err(e.cpu(), er) < 1e-6, name


def test_fused_radam_resumes_from_torch_radam_state():
    """a torch RAdam state taken at t = 4 continues identically through t = 8 (across the switch at t = 6); torch's format comes out"""
    from tqdne_amd.optim import FusedRAdamEMA

    dev = torch.device("cuda:0")
    ref = [torch.nn.Parameter(t.clone()) for t in _make(1)]
    opt_ref = torch.optim.RAdam(ref, lr=1e-3)
    g = torch.Generator().manual_seed(3)
    grads = [[torch.randn(p.shape, generator=g) for p in ref] for _ in range(8)]
    for step in range(4):
        for p, gr in zip(ref, grads[step]):
            p.grad = gr.clone()
        opt_ref.step()
    hip = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ref]
    opt = FusedRAdamEMA(_named(hip), lr=1e-3)
    opt.load_state_dict(opt_ref.state_dict())
    for step in range(4, 8):
        for pr, ph, gr in zip(ref, hip, grads[step]):
            pr.grad = gr.clone()
            ph.grad = gr.to(dev)
        opt_ref.step()
        opt.step()
    for pr, ph in zip(ref, hip):
        assert rel_err(ph.detach().cpu(), pr.detach()) < 1e-6
    sd, sd_ref = opt.state_dict(), opt_ref.state_dict()
    assert set(sd["state"][0]) == set(sd_ref["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert float(sd["state"][0]["step"]) == 8.0 and sd["state"][0]["exp_avg"].shape == ref[0].shape
    for i in range(len(ref)):
        assert rel_err(sd["state"][i]["exp_avg_sq"].cpu(), sd_ref["state"][i]["exp_avg_sq"]) < 1e-6


def test_raised_skip_flag_leaves_everything_untouched_but_the_host_step_count():
    from tqdne_amd.optim import FusedRAdamEMA

    dev = torch.device("cuda:0")
    hip = [torch.nn.Parameter(t.clone().to(dev)) for t in _make(2)]
    opt = FusedRAdamEMA(_named(hip), lr=1e-2, ema_decay=0.9)
    g = torch.Generator().manual_seed(5)

    def grads():
        for p in hip:
            p.grad = torch.randn(p.shape, generator=g).to(dev)

    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(2):   # (moments and EMA away from their initial values; a lowered flag lets the update through)
        grads()
        opt.step(skip_flag=flag)
    snap = lambda: [t.clone() for t in hip] + [opt._m.clone(), opt._v.clone(), opt._ema.clone()]
    first = [t.clone().to(dev) for t in _make(2)]
    assert not any(torch.equal(a.detach(), b) for a, b in zip(hip, first))
    before = snap()
    flag.fill_(1)
    for _ in range(5):   # (t = 3 ... 7: both forms of the update)
        grads()
        opt.step(skip_flag=flag)
    torch.cuda.synchronize()
    for a, b in zip(snap(), before):
        assert torch.equal(a, b)
    assert opt._step == 7 and float(opt.state[hip[0]]["step"]) == 7.0
