"""Gradient clipping and gradient-norm tracking inside the one-launch optimizers (tq_grad_sumsq, tq_grad_clip_coef,
tq_adam_ema_step_clipped, tq_radam_ema_step_clipped) and through DataParallelTrainer.

Expected values come from torch's own functions applied to FLOAT64 copies of the gradients (``clip_grad_norm_`` / ``clip_grad_value_`` on
double tensors): the norm both sides approximate.  (torch's fp32 ``clip_grad_norm_`` is itself off from that norm by up to 1.3e-6 relative on
these shapes and by 6e-4 on one 15.6 M-element tensor; the kernel's fp64 partial sums are the more accurate side.)  The coefficient is
rounded to fp32, multiplied into the fp32 gradients, and torch.optim.Adam / AdamW / RAdam + ``_foreach_lerp_`` run on the CPU as in
tests/test_radam_gpu.py.  Bar: 1e-6 relative, that file's and tests/test_optim.py's."""

import os

import pytest
import torch

from _ddp_launch import run_ranks
from conftest import ROOT, cfg_of, load_golden, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 5), (3,), (32,), (256, 768), (5, 7, 3), (4097,), (1,), (130, 33)]   # tests/test_radam_gpu.py's
TOL = 1e-6
LR, EMA = 3e-3, 0.9
OPTIMIZERS = ["adam", "adamw", "radam"]


def dev():
    return torch.device("cuda:0")


def _make(seed=0, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * 0.3 for s in shapes]


def _named(ps):
    return [(f"p{i}", p) for i, p in enumerate(ps)]


def _pair(kind, seed=0, shapes=SHAPES, ema=EMA):
    """(CPU parameters, torch's optimizer, device parameters, the fused optimizer) from the same start"""
    from tqdne_amd.optim import FusedAdamEMA, FusedRAdamEMA
    ref = [torch.nn.Parameter(t.clone()) for t in _make(seed, shapes)]
    hip = [torch.nn.Parameter(t.clone().to(dev())) for t in _make(seed, shapes)]
    if kind == "radam":
        return ref, torch.optim.RAdam(ref, lr=LR), hip, FusedRAdamEMA(_named(hip), lr=LR, ema_decay=ema)
    if kind == "adamw":
        return (ref, torch.optim.AdamW(ref, lr=LR, weight_decay=1e-2), hip,
                FusedAdamEMA(_named(hip), lr=LR, ema_decay=ema, weight_decay=1e-2))
    return ref, torch.optim.Adam(ref, lr=LR), hip, FusedAdamEMA(_named(hip), lr=LR, ema_decay=ema)


def norm64_and_coef(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ on float64 copies of ``grads``: (the norm as a float, the coefficient it applied rounded to fp32)"""
    d = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads]
    for p, g in zip(d, grads):
        p.grad = g.detach().double().cpu()
    norm = torch.nn.utils.clip_grad_norm_(d, max_norm)
    assert norm.dtype == torch.float64
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)   # clip_grad_norm_'s own expression, in double
    big = max(range(len(grads)), key=lambda i: grads[i].numel())
    assert torch.allclose(d[big].grad, grads[big].detach().double().cpu() * coef, rtol=1e-14, atol=0)   # (it is what torch applied)
    return float(norm), coef.float()


def _check_state(step, ref, opt_ref, ema_ref, hip, opt):
    for i, (pr, ph) in enumerate(zip(ref, hip)):
        assert rel_err(ph.detach().cpu(), pr.detach()) < TOL, ("p", step, i)
        assert rel_err(opt.state[ph]["exp_avg"].cpu(), opt_ref.state[pr]["exp_avg"]) < TOL, ("exp_avg", step, i)
        assert rel_err(opt.state[ph]["exp_avg_sq"].cpu(), opt_ref.state[pr]["exp_avg_sq"]) < TOL, ("exp_avg_sq", step, i)
    for (name, e), er in zip(opt.ema_state().items(), ema_ref):
        assert rel_err(e.cpu(), er) < TOL, ("ema", step, name)


@pytest.mark.parametrize("kind", OPTIMIZERS)
def test_norm_clipping_matches_torch_on_float64_gradients(kind):
    """nine steps, gradients over five decades, max_grad_norm = 50: norms of about 475, 4.7e3, 4.7e4 are clipped, 4.8 and 47 are not.
    Parameters, BOTH moments (Adam's first update does not depend on the gradient's scale; the moments do), EMA and the norm itself after
    every step.  The 1 / world_size rides in the launch: gradients pre-multiplied by 4, grad_scale = 0.25."""
    from tqdne_amd.optim import radam_scalars
    ref, opt_ref, hip, opt = _pair(kind)
    ema_ref = [p.detach().clone() for p in ref]
    g = torch.Generator().manual_seed(7)
    clipped, rectified = [], []
    for step in range(9):
        grads = [torch.randn(p.shape, generator=g) * (10.0 ** (step % 5 - 2)) for p in ref]
        norm, coef = norm64_and_coef(grads, 50.0)
        clipped.append(float(coef) < 1.0)
        for pr, ph, gr in zip(ref, hip, grads):
            pr.grad = gr * coef
            ph.grad = (gr * 4.0).to(dev())
        opt_ref.step()
        torch._foreach_lerp_(tuple(ema_ref), tuple(p.detach() for p in ref), 1 - EMA)
        opt.step(grad_scale=0.25, max_grad_norm=50.0)
        rectified.append(radam_scalars(step + 1, LR, 0.9, 0.999)[1] != 0.0)
        got = float(opt.last_grad_norm)
        print(f"{kind} step {step}: norm {got!r} vs float64 {norm!r} (rel {abs(got - norm) / norm:.2e}), coefficient {float(coef)!r}")
        assert opt.last_grad_norm.dtype == torch.float32 and opt.last_grad_norm.is_cuda and opt.last_grad_norm.dim() == 0
        assert abs(got - norm) < TOL * norm, step
        _check_state(step, ref, opt_ref, ema_ref, hip, opt)
    assert clipped == [False, False, True, True, True, False, False, True, True], "both kinds of step must have occurred"
    if kind == "radam":
        assert rectified == [False] * 5 + [True] * 4, "both forms of the RAdam update must have run"


@pytest.mark.parametrize("kind", OPTIMIZERS)
def test_value_clipping_matches_clip_grad_value(kind):
    """clip_value = 0.5 against torch.nn.utils.clip_grad_value_ on float64 copies (the clamp is exact in either precision), three steps
    with gradients of scale 0.1, 1 and 10: nearly all, about 38 % and about 4 % of the entries keep their value"""
    ref, opt_ref, hip, opt = _pair(kind)
    ema_ref = [p.detach().clone() for p in ref]
    g = torch.Generator().manual_seed(7)
    kept = []
    for step in range(3):
        grads = [torch.randn(p.shape, generator=g) * (10.0 ** (step - 1)) for p in ref]
        d = [torch.nn.Parameter(torch.zeros(gr.shape, dtype=torch.float64)) for gr in grads]
        for p, gr in zip(d, grads):
            p.grad = gr.double()
        torch.nn.utils.clip_grad_value_(d, 0.5)
        kept.append(sum(int((p.grad == gr.double()).sum()) for p, gr in zip(d, grads)) / sum(gr.numel() for gr in grads))
        for pr, ph, p, gr in zip(ref, hip, d, grads):
            pr.grad = p.grad.float()
            ph.grad = (gr * 4.0).to(dev())
        opt_ref.step()
        torch._foreach_lerp_(tuple(ema_ref), tuple(p.detach() for p in ref), 1 - EMA)
        opt.step(grad_scale=0.25, clip_value=0.5)
        _check_state(step, ref, opt_ref, ema_ref, hip, opt)
    assert opt.last_grad_norm is None   # no norm was asked for: none was formed
    assert kept[0] > 0.99 and 0.2 < kept[1] < 0.8 and kept[2] < 0.1, kept


def test_more_chunks_than_the_reducing_workgroup_has_threads():
    """1025 + 1 chunks against the 256 threads of tq_grad_clip_coef's workgroup; a tail of 5 after 1024 full chunks, a tensor of 7"""
    shapes = [(1024 * 4096 + 5,), (7,)]
    ref, opt_ref, hip, opt = _pair("adam", shapes=shapes, ema=None)
    assert opt._step == 0
    g = torch.Generator().manual_seed(4)
    grads = [torch.randn(s, generator=g) for s in shapes]
    norm, coef = norm64_and_coef(grads, 100.0)
    assert float(coef) < 0.1   # (the norm is about 2048)
    for pr, ph, gr in zip(ref, hip, grads):
        pr.grad = gr * coef
        ph.grad = gr.to(dev())
    opt_ref.step()
    opt.step(max_grad_norm=100.0)
    assert opt._n_chunks == 1026
    got = float(opt.last_grad_norm)
    print(f"norm {got!r} vs float64 {norm!r}: rel {abs(got - norm) / norm:.2e}")
    assert abs(got - norm) < TOL * norm
    for pr, ph in zip(ref, hip):
        assert rel_err(ph.detach().cpu(), pr.detach()) < TOL
        assert rel_err(opt.state[ph]["exp_avg"].cpu(), opt_ref.state[pr]["exp_avg"]) < TOL
        assert rel_err(opt.state[ph]["exp_avg_sq"].cpu(), opt_ref.state[pr]["exp_avg_sq"]) < TOL
    # tracking only: the same norm, no clipping (a second optimizer on the same gradients)
    _, _, hip2, opt2 = _pair("adam", shapes=shapes, ema=None)
    for ph, gr in zip(hip2, grads):
        ph.grad = gr.to(dev())
    opt2.step(track_grad_norm=True)
    assert torch.equal(opt2.last_grad_norm, opt.last_grad_norm) and float(opt2._norm_buf[1][1]) == 1.0
    m_ref = (gr * 0.1 for gr in grads)
    for ph, mr in zip(hip2, m_ref):
        assert rel_err(opt2.state[ph]["exp_avg"].cpu(), mr) < TOL   # (1 - beta1) * g: unclipped


def test_same_gradients_give_the_same_bits():
    outs = []
    for _ in range(2):
        _, _, hip, opt = _pair("radam")
        g = torch.Generator().manual_seed(9)
        seen = []
        for step in range(2):
            for ph in hip:
                ph.grad = (torch.randn(ph.shape, generator=g) * 3.0).to(dev())
            opt.step(max_grad_norm=50.0)
            seen += [opt.last_grad_norm.clone(), opt._norm_buf[1].clone(), opt._norm_buf[0].clone()]
        outs.append(seen + [p.detach().clone() for p in hip] + [opt._m.clone(), opt._v.clone(), opt._ema.clone()])
    assert float(outs[0][1][1]) < 1.0   # clipped
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", OPTIMIZERS)
def test_off_means_off(kind):
    """no clip argument: bit-identical to the call as it was before the arguments existed, nothing allocated, no norm.  Also: a
    coefficient of exactly 1 (norm far below max_grad_norm) changes no bit either -- the clipped kernel has the same update body."""
    runs = []
    for call in (lambda o: o.step(grad_scale=0.25),
                 lambda o: o.step(grad_scale=0.25, skip_flag=None, max_grad_norm=None, clip_value=None, track_grad_norm=False),
                 lambda o: o.step(grad_scale=0.25, max_grad_norm=1e30),
                 lambda o: o.step(grad_scale=0.25, clip_value=1e30)):
        _, _, hip, opt = _pair(kind)
        g = torch.Generator().manual_seed(7)
        for step in range(3):
            for ph in hip:
                ph.grad = (torch.randn(ph.shape, generator=g) * 4.0).to(dev())
            call(opt)
        runs.append((opt, [p.detach().clone() for p in hip] + [opt._m.clone(), opt._v.clone(), opt._ema.clone()]))
    for opt, _ in runs[:2]:
        assert opt.last_grad_norm is None and opt._norm_buf is None
    assert float(runs[2][0]._norm_buf[1][1]) == 1.0
    for _, state in runs[1:]:
        for a, b in zip(state, runs[0][1]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["adam", "radam"])
def test_raised_skip_flag_with_clipping_on_leaves_everything_untouched(kind):
    _, _, hip, opt = _pair(kind, seed=2)
    g = torch.Generator().manual_seed(5)

    def grads():
        for p in hip:
            p.grad = (torch.randn(p.shape, generator=g) * 3.0).to(dev())

    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    for _ in range(2):   # (moments and EMA away from their initial values; a lowered flag lets the clipped update through)
        grads()
        opt.step(skip_flag=flag, max_grad_norm=50.0)
    snap = lambda: [t.detach().clone() for t in hip] + [opt._m.clone(), opt._v.clone(), opt._ema.clone()]
    first = [t.to(dev()) for t in _make(2)]
    assert not any(torch.equal(a.detach(), b) for a, b in zip(hip, first))
    before = snap()
    flag.fill_(1)
    for kw in (dict(max_grad_norm=50.0), dict(clip_value=0.5), dict(max_grad_norm=50.0), dict(track_grad_norm=True)):
        grads()
        opt.step(skip_flag=flag, **kw)
    torch.cuda.synchronize()
    for a, b in zip(snap(), before):
        assert torch.equal(a, b)
    assert opt._step == 6 and float(opt.last_grad_norm) > 50.0   # the host-side count moves on; the norm is still formed


def test_both_algorithms_at_once_are_refused():
    _, _, hip, opt = _pair("adam")
    for ph in hip:
        ph.grad = torch.zeros_like(ph)
    with pytest.raises(ValueError, match="alternatives"):
        opt.step(max_grad_norm=1.0, clip_value=1.0)
    assert opt._step == 0


# ------------------------------------------------------------------------------------------------ trainer, one rank
def _edm():
    from tqdne_amd import LightningEDM
    sd, d = load_golden("micro_unet.npz")
    edm = LightningEDM(dict(cfg_of(d), dropout=0.0), {"learning_rate": 1e-3, "max_steps": 10, "eta_min": 0.0})
    edm.unet.load_state_dict(sd)
    g = torch.Generator().manual_seed(2)
    batch = {"signal": (0.5 * torch.randn(2, 3, 256, generator=g)).to(dev()), "cond": torch.randn(2, 5, generator=g).to(dev())}
    return edm.to(dev()).train(), batch, {}


def _cm():
    from tqdne_amd import UNetModel
    from tqdne_amd.consistency_model import LithningConsistencyModel
    sd, d = load_golden("micro_unet.npz")
    net = UNetModel(**cfg_of(d))
    net.load_state_dict(sd)
    cm = LithningConsistencyModel(net, initial_timesteps=10, final_timesteps=40, lr=1e-3).to(dev()).train()
    cm.max_steps, cm.global_step = 6, 0   # (the look-ahead step below runs without a trainer; the trainer publishes the same progress)
    g = torch.Generator().manual_seed(9)
    batch = {"signal": (0.5 * torch.randn(2, 3, 256, generator=g)).to(dev()), "cond": torch.randn(2, 5, generator=g).to(dev())}
    return cm, batch, {"max_steps": 6}


def _ae():
    import numpy as np
    from conftest import GOLDEN
    from tqdne_amd import LightningAutoencoder
    sd, d = load_golden("micro_ae.npz")
    s = np.load(os.path.join(GOLDEN, "micro_ae_step.npz"))
    ae = LightningAutoencoder(cfg_of(d, "enc_cfg"), cfg_of(d, "dec_cfg"), {"learning_rate": 2e-3, "max_steps": 50, "eta_min": 0})
    ae.load_state_dict(sd)
    return ae.to(dev()).train(), {"signal": torch.from_numpy(s["x"]).to(dev())}, {}


def _norm64(grads):
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))


@pytest.mark.parametrize("which", ["edm", "cm", "ae"])
def test_trainer_clips_by_norm_inside_the_optimizer_launch(which):
    """first fused train step with gradient_clip_val below the gradient norm (half of the norm of a look-ahead ``step_and_backward`` with
    the same seeds): ``last_grad_norm`` is the float64 norm of the gradients read back, and -- the moments start at zero -- exp_avg =
    (1 - beta1) * coef * g, exp_avg_sq = (1 - beta2) * (coef * g)^2, formed on the host in fp32.  EDM: Adam; consistency model: RAdam;
    autoencoder: AdamW over two flat gradient buffers."""
    from tqdne_amd import rng
    from tqdne_amd.optim import FusedAdamEMA, FusedRAdamEMA
    from tqdne_amd.trainer import DataParallelTrainer
    module, batch, kw = {"edm": _edm, "cm": _cm, "ae": _ae}[which]()
    named = [(n, p) for n, p in module.named_parameters() if p.requires_grad]

    def seed():
        torch.manual_seed(1)
        rng.seed_rank(7, 0)

    seed()
    module.step_and_backward(batch)
    c = 0.5 * _norm64([p.grad for _, p in named])
    assert c > 0
    tr = DataParallelTrainer(module, world_size=1, ema_decay=0.999, gradient_clip_val=c, **kw)
    assert isinstance(tr.optimizer, FusedRAdamEMA if which == "cm" else FusedAdamEMA) and tr.last_grad_norm is None
    if which == "ae":
        assert tr.optimizer.param_groups[0]["weight_decay"] > 0
    seed()
    loss = tr.train_step(batch)
    assert torch.isfinite(loss)
    grads = [p.grad.detach().cpu() for _, p in named]
    norm = _norm64(grads)
    assert norm > c, "the step must have been clipped"
    got = tr.last_grad_norm
    assert got is tr.optimizer.last_grad_norm and got.is_cuda and got.dtype == torch.float32
    print(f"{which}: clip {c!r}, norm {float(got)!r} vs float64 {norm!r} (rel {abs(float(got) - norm) / norm:.2e})")
    assert abs(float(got) - norm) < TOL * norm
    coef = torch.tensor(min(1.0, c / (norm + 1e-6)), dtype=torch.float64).float()
    b1, b2 = tr.optimizer.param_groups[0]["betas"]
    omb1, omb2 = torch.tensor(1.0 - b1).float(), torch.tensor(1.0 - b2).float()
    for (n, p), g in zip(named, grads):
        gc = g * coef
        st = tr.optimizer.state[p]
        if float(g.abs().max()) == 0.0:
            assert not st["exp_avg"].any() and not st["exp_avg_sq"].any(), n
            continue
        assert rel_err(st["exp_avg"].cpu(), gc * omb1) < TOL, n
        assert rel_err(st["exp_avg_sq"].cpu(), gc * gc * omb2) < TOL, n
    assert tr.optimizer._step == 1 and tr.steps_done == 1


def test_trainer_defaults_form_no_norm():
    from tqdne_amd.trainer import DataParallelTrainer
    module, batch, _ = _edm()
    tr = DataParallelTrainer(module, world_size=1, ema_decay=0.999)
    tr.train_step(batch)
    assert tr.last_grad_norm is None and tr.optimizer.last_grad_norm is None and tr.optimizer._norm_buf is None


# ------------------------------------------------------------------------------------------------ trainer, two ranks
@pytest.mark.timeout(600)
def test_two_rank_clipped_training_reproduces_the_full_batch_run():
    """tests/_clip_ddp_worker.py: two ranks on halves of a fixed global batch of the micro EDM model, gradient_clip_val on, against one
    rank on the full batch: ``last_grad_norm`` of both steps and the parameters after two steps, at tests/test_ddp_gpu.py's bars for the
    unclipped gradients (1e-5 over the flat vector, 5e-4 for the worst tensor against its own scale)."""
    res = run_ranks("_clip_ddp_worker.py", timeout=400)
    assert all(n > res["clip"] for n in res["norms_full"]), "both steps must have been clipped"
    for a, b in zip(res["norms"], res["norms_full"]):
        assert abs(a - b) < 1e-5 * b, res
    assert res["norms_equal_across_ranks"] and res["replicas_equal"], res
    assert res["err_flat"] < 1e-5 and res["err_worst_tensor"] < 5e-4, res
    assert res["moved"] > 0 and res["steps"] == 2, res
