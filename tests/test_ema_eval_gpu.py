"""Validation and sampling on the EMA weights mid-training, checkpoints and resuming, on the GPU: the in-place exchange of the
parameters with their EMA (tq_ema_swap, one launch over a chunk table of every optimized parameter) under the one-launch optimizers,
and DataParallelTrainer's ``ema_weights`` / ``validate`` / ``evaluate`` / ``save_checkpoint`` / ``load_checkpoint`` / ``fit`` on the
micro EDM, consistency-model and autoencoder configurations.

Bars.  The exchange moves bit patterns: everything about it is compared through ``.view(torch.int32)`` and must be equal.  An inference
forward on the swapped-in weights runs the same kernels on the same weights as a fresh module loaded with the EMA: ``torch.equal``, as
tests/test_trainer_gpu.py::test_plans_share_one_packed_weight_store relies on.  ``validate`` against the same steps by hand: rel 1e-6,
that file's bar for two evaluations of one computation.  A resumed run against the run it was saved from: two correct runs of the same
steps differ in the last bits (the backward's GroupNorm-affine atomics), so the trajectories are held to
``test_fused_and_torch_adam_train_the_same_trajectory``'s bars: losses rel 2e-4, at least 90 % of the tensors within 2e-3, two named
conv weights within 2e-3 (the autoencoder has no tensors of those names: its first and last conv stand in)."""

import os

import pytest
import torch

from _ddp_launch import run_ranks
from conftest import ROOT, cfg_of, load_golden, rel_err

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 3]   # tail alone, body + tail, a full chunk, a ragged last chunk of three
EMA = 0.9
WHICH = ["edm", "cm", "ae"]


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.detach().reshape(-1).view(torch.int32).clone()


# ------------------------------------------------------------------------------------------------ the kernel under a bare optimizer
SPECIALS = [0x7FC00000, 0x7FC12345, -0x003EDCBB, 0x7F800000, -0x00800000, -0x80000000, 0x00000001, -0x7FFFFFFF, 0x007FFFFF]
# (quiet NaN, NaNs with payloads of either sign, +inf, -inf, -0.0, the smallest and the largest denormals)


def _patterns(n, seed, rot=0):
    """``n`` random 32-bit patterns -- NaNs of every payload, infinities and denormals occur among them by themselves -- with the
    named special values (rotated by ``rot``: parameters and EMA get different ones at the same index) in front where they fit"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    k = min(n, len(SPECIALS))
    w[:k] = torch.tensor((SPECIALS[rot:] + SPECIALS[:rot])[:k], dtype=torch.int64).to(torch.int32)
    return w


def _ema_raw(opt, params):
    """the optimizer's EMA buffer cut per parameter, whatever ``ema_swapped`` says"""
    return [opt._ema[o:o + p.numel()] for p, o in zip(params, opt._offs)]


def _bare(kind, ema=EMA):
    """parameters of SIZES + one that never gets a gradient + one frozen, all handed to the constructor"""
    from tqdne_amd.optim import FusedAdamEMA, FusedRAdamEMA
    g = torch.Generator().manual_seed(1)
    ps = [torch.nn.Parameter((torch.randn(n, generator=g) * 0.3).to(dev())) for n in SIZES]
    no_grad = torch.nn.Parameter(torch.randn(7, generator=g).to(dev()))
    frozen = torch.nn.Parameter(torch.randn(9, generator=g).to(dev()), requires_grad=False)
    named = [(f"p{i}", p) for i, p in enumerate(ps)] + [("no_grad", no_grad), ("frozen", frozen)]
    opt = (FusedRAdamEMA if kind == "radam" else FusedAdamEMA)(named, lr=1e-2, ema_decay=ema)
    return ps, no_grad, frozen, opt


def _give_grads(ps, seed=2):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(dev())


def _fill(tensors, seed, rot=0):
    with torch.no_grad():
        for i, t in enumerate(tensors):
            t.view(torch.int32).copy_(_patterns(t.numel(), seed + i, rot).to(dev()))


@pytest.mark.parametrize("kind", ["adam", "radam"])
def test_swap_exchanges_bit_patterns_and_two_swaps_restore_everything(kind):
    ps, no_grad, frozen, opt = _bare(kind)
    _give_grads(ps)
    opt.step()   # (moments away from zero; the step's own table exists and skips ``no_grad``)
    swapped = ps + [no_grad]
    ema = list(opt.ema_state().values())
    assert list(opt.ema_state()) == [f"p{i}" for i in range(len(SIZES))] + ["no_grad"]
    _fill([p.data for p in swapped], 100)
    _fill(ema, 200, rot=1)
    p0, e0, f0 = [bits(p) for p in swapped], [bits(e) for e in ema], bits(frozen)
    m0, v0 = bits(opt._m), bits(opt._v)
    assert any(bool(torch.isnan(p).any()) for p in swapped) and not any(torch.equal(a, b) for a, b in zip(p0, e0))
    versions = [p._version for p in swapped]
    opt.swap_ema()
    assert opt.ema_swapped
    for p, e, a, b in zip(swapped, _ema_raw(opt, swapped), p0, e0):
        assert torch.equal(bits(p), b) and torch.equal(bits(e), a), p.numel()
    for k, (n, t) in enumerate(opt.ema_state().items()):   # still the EMA of the run: it lives in the parameters now
        assert torch.equal(bits(t), e0[k]), n
    assert torch.equal(bits(frozen), f0) and torch.equal(bits(opt._m), m0) and torch.equal(bits(opt._v), v0)
    assert all(p._version > v for p, v in zip(swapped, versions))
    versions = [p._version for p in swapped]
    opt.swap_ema()
    assert not opt.ema_swapped
    for p, e, a, b in zip(swapped, _ema_raw(opt, swapped), p0, e0):
        assert torch.equal(bits(p), a) and torch.equal(bits(e), b), p.numel()
    assert torch.equal(bits(frozen), f0) and torch.equal(bits(opt._m), m0) and torch.equal(bits(opt._v), v0)
    assert all(p._version > v for p, v in zip(swapped, versions))
    # the padding between the tensors of the flat EMA buffer was never written
    used = torch.zeros_like(opt._ema, dtype=torch.bool)
    for p, o in zip(swapped, opt._offs):
        used[o:o + p.numel()] = True
    assert not opt._ema[~used].any()


@pytest.mark.parametrize("kind", ["adam", "radam"])
def test_swap_before_the_first_step_and_step_while_swapped(kind):
    ps, no_grad, frozen, opt = _bare(kind)
    swapped = ps + [no_grad]
    assert opt._table is None   # no step yet: the swap does not need the step's table
    with torch.no_grad():
        for p in swapped:
            p.mul_(1.5)          # (the EMA starts as a copy of the parameters: make them differ)
    p0, e0 = [bits(p) for p in swapped], [bits(e) for e in _ema_raw(opt, swapped)]
    opt.swap_ema()
    for p, e, a, b in zip(swapped, _ema_raw(opt, swapped), p0, e0):
        assert torch.equal(bits(p), b) and torch.equal(bits(e), a)
    _give_grads(ps)
    snap = lambda: [bits(p) for p in swapped] + [bits(opt._ema), bits(opt._m), bits(opt._v)]
    before, versions = snap(), [p._version for p in swapped]
    with pytest.raises(RuntimeError, match="EMA weights"):
        opt.step()
    torch.cuda.synchronize()
    assert opt._step == 0 and opt._table is None and [p._version for p in swapped] == versions
    for a, b in zip(snap(), before):
        assert torch.equal(a, b)
    opt.swap_ema()
    opt.step()   # back on the training weights: the step runs
    assert opt._step == 1 and not torch.equal(bits(ps[4]), p0[4])


def test_swap_without_an_ema_raises():
    _, _, _, opt = _bare("adam", ema=None)
    with pytest.raises(RuntimeError, match="constructed without ema_decay"):
        opt.swap_ema()
    assert not opt.ema_swapped


# ------------------------------------------------------------------------------------------------ the three modules
LR = 2e-3   # three Adam steps move every weight by about 6e-3; the EMA (decay 0.9) follows at about a quarter of that


def _edm(dropout=0.0):
    from tqdne_amd import LightningEDM
    sd, d = load_golden("micro_unet.npz")
    edm = LightningEDM(dict(cfg_of(d), dropout=dropout), {"learning_rate": LR, "max_steps": 20, "eta_min": 0.0}, num_sampling_steps=4)
    edm.unet.load_state_dict(sd)
    return edm.to(dev()).train(), {}


def _cm(dropout=0.0):
    from tqdne_amd import UNetModel
    from tqdne_amd.consistency_model import LithningConsistencyModel
    sd, d = load_golden("micro_unet.npz")
    net = UNetModel(**dict(cfg_of(d), dropout=dropout))
    net.load_state_dict(sd)
    return LithningConsistencyModel(net, initial_timesteps=10, final_timesteps=40, lr=LR).to(dev()).train(), {"max_steps": 12}


def _ae(dropout=0.0):
    from tqdne_amd import LightningAutoencoder
    sd, d = load_golden("micro_ae.npz")
    ae = LightningAutoencoder(cfg_of(d, "enc_cfg"), cfg_of(d, "dec_cfg"), {"learning_rate": LR, "max_steps": 50, "eta_min": 0})
    ae.load_state_dict(sd)
    return ae.to(dev()).train(), {}


MAKE = {"edm": _edm, "cm": _cm, "ae": _ae}
NAMED = {"edm": ("unet.input_blocks.1.0.in_layers.2.weight", "unet.out.2.weight"),
         "cm": ("net.input_blocks.1.0.in_layers.2.weight", "net.out.2.weight"),
         "ae": ("encoder.input_layer.weight", "decoder.output_layer.weight")}


def _batch(which, B=2, seed=2):
    g = torch.Generator().manual_seed(seed)
    if which == "ae":
        return {"signal": (0.5 * torch.randn(B, 3, 256, generator=g)).to(dev())}
    return {"signal": (0.5 * torch.randn(B, 3, 256, generator=g)).to(dev()), "cond": torch.randn(B, 5, generator=g).to(dev())}


def _trained(which, steps=3, dropout=0.0, **kw):
    from tqdne_amd import rng
    from tqdne_amd.trainer import DataParallelTrainer
    module, tkw = MAKE[which](dropout)
    rng.seed_rank(7, 0)
    tr = DataParallelTrainer(module, world_size=1, ema_decay=EMA, **dict(tkw, **kw))
    batch = _batch(which)
    losses = []
    for i in range(steps):
        torch.manual_seed(100 + i)
        losses.append(tr.train_step(batch))
    assert all(bool(torch.isfinite(l)) for l in losses)
    return module, tr, batch


def _fresh(which, trained, weights=None):
    """a fresh module holding ``trained``'s state and, over it, ``weights`` (an EMA snapshot), as the reference loads one"""
    module, _ = MAKE[which]()
    module.load_state_dict(trained.state_dict())
    if weights is not None:
        module.load_state_dict(weights, strict=False)
    return module


def _infer(which, module, batch):
    """one inference forward (no gradients) of the module's network(s)"""
    torch.manual_seed(5)   # (the autoencoder draws its latent)
    with torch.no_grad():
        if which == "ae":
            return module(batch["signal"])
        sigma = torch.full((batch["signal"].shape[0],), 0.7, device=dev())
        return module(batch["signal"], sigma, None, batch["cond"])


def _ema_snapshot(tr):
    return {k: v.detach().clone() for k, v in tr.ema_state().items()}


def _weights(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def _equal(a, b):
    return a.keys() == b.keys() and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("which", WHICH)
def test_ema_weights_context_holds_the_ema_and_restores_also_after_an_exception(which, fused):
    from tqdne_amd.optim import _FusedFlatOptimizer
    module, tr, batch = _trained(which, fused_optimizer=fused)
    assert isinstance(tr.optimizer, _FusedFlatOptimizer) == fused
    ema0, w0 = _ema_snapshot(tr), _weights(module)
    trainable = [n for n, p in module.named_parameters() if p.requires_grad]
    assert sorted(ema0) == sorted(trainable)
    # three steps separate the EMA from every weight that training moved (a tensor whose gradient is exactly zero -- the consistency
    # model has a few -- stays where it started, and so does its EMA)
    start = _weights(MAKE[which]()[0])
    moved = [n for n in trainable if not torch.equal(w0[n], start[n])]
    print(f"{which}: {len(moved)} of {len(trainable)} trainable tensors moved; at rest: {sorted(set(trainable) - set(moved))[:6]}")
    assert len(moved) >= 0.9 * len(trainable) and not any(torch.equal(ema0[n], w0[n]) for n in moved), "EMA and weights must differ"
    with tr.ema_weights():
        w1 = _weights(module)
        for n in trainable:
            assert torch.equal(w1[n], ema0[n]), n
        for n in set(w0) - set(trainable):   # frozen parameters and buffers are not the callback's business
            assert torch.equal(w1[n], w0[n]), n
        assert _equal(_ema_snapshot(tr), ema0)   # ema_state() means the EMA of the run, also in here
        with pytest.raises(RuntimeError, match="does not nest"):
            with tr.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="train_step inside ema_weights"):
            tr.train_step(batch)
        assert _equal(_weights(module), w1) and tr.steps_done == 3
    assert _equal(_weights(module), w0) and _equal(_ema_snapshot(tr), ema0)
    with pytest.raises(ZeroDivisionError):
        with tr.ema_weights():
            1 / 0
    assert _equal(_weights(module), w0) and _equal(_ema_snapshot(tr), ema0) and not tr._ema_active
    assert bool(torch.isfinite(tr.train_step(batch))) and tr.steps_done == 4


@pytest.mark.parametrize("which", WHICH)
def test_inference_forward_inside_the_context_is_the_ema_models_and_the_packed_weights_follow_both_swaps(which):
    module, tr, batch = _trained(which)
    ema0 = _ema_snapshot(tr)
    y_train = _infer(which, module, batch)
    with tr.ema_weights():
        y_ema = _infer(which, module, batch)
    y_back = _infer(which, module, batch)
    y_ref = _infer(which, _fresh(which, module, ema0), batch)
    assert torch.equal(y_ema, y_ref)
    assert not torch.equal(y_ema, y_train)
    assert torch.equal(y_back, y_train)


def test_evaluate_samples_from_the_ema_weights():
    module, tr, batch = _trained("edm")
    ema0 = _ema_snapshot(tr)
    torch.manual_seed(11)
    got = tr.evaluate(batch)
    assert module.training and got.shape == batch["signal"].shape and bool(torch.isfinite(got).all())
    fresh = _fresh("edm", module, ema0).eval()
    torch.manual_seed(11)
    want = fresh.evaluate(batch)
    assert torch.equal(got, want)
    torch.manual_seed(11)
    assert not torch.equal(module.eval().evaluate(batch), got), "the training weights sample something else"


def _by_hand(which, module, tr, batches, seed):
    module.eval()
    if tr.max_steps is not None:
        module._dp_progress = (tr.steps_done, tr.max_steps)
    torch.manual_seed(seed)
    with torch.no_grad():
        losses = [float(module.validation_step(b, i)) for i, b in enumerate(batches)]
    sizes = [b["signal"].shape[0] for b in batches]
    return sum(l * n for l, n in zip(losses, sizes)) / sum(sizes)


@pytest.mark.parametrize("which", WHICH)
def test_validate_is_the_batch_weighted_validation_loss_on_the_ema_weights(which):
    module, tr, _ = _trained(which)
    ema0, w0 = _ema_snapshot(tr), _weights(module)
    batches = [_batch(which, 2, seed=21), _batch(which, 3, seed=22)]
    torch.manual_seed(31)
    got = tr.validate(batches)
    assert got.is_cuda and got.dim() == 0
    fresh = _fresh(which, module, ema0)
    want = _by_hand(which, fresh, tr, batches, 31)
    print(f"{which}: validate {float(got)!r} vs by hand {want!r} (rel {abs(float(got) - want) / abs(want):.2e})")
    assert float(got) == pytest.approx(want, rel=1e-6)
    assert module.training and all(m.training for m in module.modules()) and _equal(_weights(module), w0)
    torch.manual_seed(31)
    assert float(tr.validate(batches, limit_batches=1)) == pytest.approx(_by_hand(which, fresh, tr, batches[:1], 31), rel=1e-6)


def test_validate_without_an_ema_runs_on_the_training_weights():
    from tqdne_amd.trainer import DataParallelTrainer
    module, _ = _edm()
    tr = DataParallelTrainer(module, world_size=1)
    batch = _batch("edm")
    for i in range(2):
        torch.manual_seed(100 + i)
        tr.train_step(batch)
    batches = [_batch("edm", 2, seed=21), _batch("edm", 3, seed=22)]
    torch.manual_seed(31)
    got = float(tr.validate(batches))
    assert got == pytest.approx(_by_hand("edm", _fresh("edm", module), tr, batches, 31), rel=1e-6) and module.training
    with pytest.raises(RuntimeError, match="constructed without ema_decay"):
        with tr.ema_weights():
            pass


def test_swap_allocates_no_second_copy_of_the_model():
    module, tr, _ = _trained("edm", steps=1)
    param_bytes = sum(p.numel() * 4 for p in module.parameters() if p.requires_grad)
    with tr.ema_weights():   # (the swap's chunk table exists from here on)
        pass
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with tr.ema_weights():
        inside = torch.cuda.memory_allocated()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"parameters {param_bytes} B; allocated {base} B before, {inside} B inside, peak {peak} B")
    assert peak - base < param_bytes // 2


# ------------------------------------------------------------------------------------------------ checkpoints, resuming
def _assert_same_state(which, a, tr_a, b, tr_b):
    assert _equal(_weights(a), _weights(b)) and _equal(_ema_snapshot(tr_a), _ema_snapshot(tr_b))
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        if p.requires_grad:
            sa, sb = tr_a.optimizer.state[p], tr_b.optimizer.state[q]
            assert torch.equal(bits(sa["exp_avg"]), bits(sb["exp_avg"])) and torch.equal(bits(sa["exp_avg_sq"]), bits(sb["exp_avg_sq"])), n
            assert float(sa["step"]) == float(sb["step"])
    assert tr_a.optimizer._step == tr_b.optimizer._step and tr_a.steps_done == tr_b.steps_done
    assert tr_a.optimizer.param_groups[0]["lr"] == tr_b.optimizer.param_groups[0]["lr"]
    if tr_a.scheduler is not None:
        assert tr_a.scheduler.last_epoch == tr_b.scheduler.last_epoch and tr_a.scheduler.get_last_lr() == tr_b.scheduler.get_last_lr()


@pytest.mark.parametrize("which", WHICH)
def test_a_resumed_run_continues_the_run_it_was_saved_from(which, tmp_path):
    from tqdne_amd import rng
    from tqdne_amd.checkpoint import _RemapPickle, load_checkpoint
    from tqdne_amd.trainer import DataParallelTrainer
    drop = 0.1 if which != "ae" else 0.0   # (masks of the continued steps depend on the restored call counter)
    a, tr_a, batch = _trained(which, dropout=drop)
    path = str(tmp_path / "n3.ckpt")
    tr_a.save_checkpoint(path)
    counter = rng.dropout_counter()
    assert counter > 0 and tr_a.steps_done == 3
    rng.reset_dropout_counter(0)
    b, tkw = MAKE[which](drop)
    tr_b = DataParallelTrainer(b, world_size=1, ema_decay=EMA, **tkw)
    versions = {n: p._version for n, p in b.named_parameters()}
    tr_b.load_checkpoint(path)
    assert rng.dropout_counter() == counter and all(p._version > versions[n] for n, p in b.named_parameters())
    _assert_same_state(which, a, tr_a, b, tr_b)
    if which != "cm":
        assert tr_b.optimizer.param_groups[0]["lr"] < LR   # three cosine steps in

    def go_on(tr):
        rng.reset_dropout_counter(counter)
        out = []
        for i in range(3):
            torch.manual_seed(1000 + i)
            out.append(float(tr.train_step(batch)))
        return out

    l_b, l_a = go_on(tr_b), go_on(tr_a)
    print(which, "losses resumed", l_b, "original", l_a)
    for x, y in zip(l_b, l_a):
        assert x == pytest.approx(y, rel=2e-4)
    w_a, w_b = _weights(a), _weights(b)
    errs = {k: rel_err(w_b[k], w_a[k], elem=False) for k in w_a if w_a[k].is_floating_point()}   # (two trajectories, counted below)
    close = sum(e < 2e-3 for e in errs.values())
    print("weights within 2e-3:", close, "of", len(errs), "; worst", max(errs.items(), key=lambda kv: kv[1]))
    assert close >= 0.9 * len(errs)
    assert all(errs[n] < 2e-3 for n in NAMED[which])
    assert tr_a.steps_done == tr_b.steps_done == 6 == tr_b.optimizer._step
    # a checkpoint as the reference writes it: without our key
    raw = load_checkpoint(path)
    del raw["tqdne_amd_trainer"]
    bare = str(tmp_path / "bare.ckpt")
    torch.save(raw, bare, pickle_module=_RemapPickle)
    c, tkw = MAKE[which]()
    tr_c = DataParallelTrainer(c, world_size=1, ema_decay=EMA, **tkw)
    tr_c.load_checkpoint(bare)
    assert tr_c.steps_done == 3 == tr_c.optimizer._step
    for n, t in raw["ema_state"].items():
        assert torch.equal(tr_c.ema_state()[n].cpu(), t), n


def test_a_run_that_left_the_fp16_range_scheme_resumes_on_bf16x3(tmp_path):
    """The range guard fires in the middle of a run (raised the way the range-guard test of tests/test_trainer_gpu.py raises it: a
    residual stream is blown up); the checkpoint written afterwards records the scheme.  A fresh trainer that already holds a plan on
    the fp16-range scheme must come out of ``load_checkpoint`` with model, existing plans and later plans on bf16x3, and its next step
    must be the saved run's next step (the bar of test_a_resumed_run_continues_the_run_it_was_saved_from)."""
    import warnings

    from tqdne_amd import rng
    from tqdne_amd.trainer import DataParallelTrainer
    a, tr_a, batch = _trained("edm", steps=2)
    assert a.unet._conv_scheme == "auto" and all(e.scheme == "auto" for e in a.unet._engine_cache.values())
    with torch.no_grad():   # blow up the residual stream behind the first ResBlock
        for n, p in a.unet.named_parameters():
            if n.startswith("input_blocks.1.0.out_layers.3."):
                p.mul_(3.0e5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # ("activations approach the fp16 range")
        for k in range(6):   # the first of these steps raises the flag; the host sees it at the start of one of the next forwards
            if a.unet._conv_scheme == "bf16x3":
                break
            torch.manual_seed(200 + k)
            tr_a.train_step(batch)
            torch.cuda.synchronize()
    assert a.unet._conv_scheme == "bf16x3" and all(e.scheme == "bf16x3" for e in a.unet._engine_cache.values())
    path = str(tmp_path / "bf16x3.ckpt")
    tr_a.save_checkpoint(path)
    counter = rng.dropout_counter()

    b, tkw = MAKE["edm"]()
    tr_b = DataParallelTrainer(b, world_size=1, ema_decay=EMA, **tkw)
    _infer("edm", b, batch)
    plans = list(b.unet._engine_cache.values())
    assert plans and all(e.scheme == "auto" for e in plans) and b.unet._conv_scheme == "auto"
    tr_b.load_checkpoint(path)
    assert b.unet._conv_scheme == "bf16x3"
    assert list(b.unet._engine_cache.values()) == plans and all(e.scheme == "bf16x3" for e in plans)
    assert b.unet._engine(3, 256, dev()).scheme == "bf16x3"   # a plan built afterwards starts there
    _assert_same_state("edm", a, tr_a, b, tr_b)

    losses = []
    for tr in (tr_b, tr_a):
        rng.reset_dropout_counter(counter)
        torch.manual_seed(1000)
        losses.append(float(tr.train_step(batch)))
    print("loss resumed", losses[0], "original", losses[1])
    assert losses[0] == pytest.approx(losses[1], rel=2e-4)
    w_a, w_b = _weights(a), _weights(b)
    errs = {k: rel_err(w_b[k], w_a[k], elem=False) for k in w_a if w_a[k].is_floating_point()}
    close = sum(e < 2e-3 for e in errs.values())
    print("weights within 2e-3:", close, "of", len(errs), "; worst", max(errs.items(), key=lambda kv: kv[1]))
    assert close >= 0.9 * len(errs)
    assert all(errs[n] < 2e-3 for n in NAMED["edm"])
    assert tr_a.steps_done == tr_b.steps_done == tr_b.optimizer._step


def test_fit_validates_keeps_the_best_checkpoints_and_resumes(tmp_path):
    from tqdne_amd.trainer import DataParallelTrainer
    train = [_batch("edm", 2, seed=40 + i) for i in range(2)]
    val = [_batch("edm", 2, seed=50), _batch("edm", 3, seed=51)]
    module, _ = _edm()
    tr = DataParallelTrainer(module, world_size=1, ema_decay=EMA)
    d = str(tmp_path / "run")
    torch.manual_seed(3)
    hist = tr.fit(train, val, max_steps=6, val_check_interval=2, dirpath=d, save_top_k=2)
    assert tr.steps_done == 6 and [s for s, _ in hist] == [2, 4, 6] and all(v == v and v > 0 for _, v in hist)
    files = sorted(os.listdir(d))
    assert "last.ckpt" in files and len(files) == 3, files
    best = sorted(hist, key=lambda sv: sv[1])[:2]
    assert {f for f in files if f != "last.ckpt"} == {f"step={s}-val_loss={v:.2e}.ckpt" for s, v in best}
    module2, _ = _edm()
    tr2 = DataParallelTrainer(module2, world_size=1, ema_decay=EMA)
    seen = []
    step = tr2.train_step
    tr2.train_step = lambda b: (seen.append(tr2.steps_done), step(b))[1]
    hist2 = tr2.fit(train, val, max_steps=8, val_check_interval=2, ckpt_path=os.path.join(d, "last.ckpt"))
    assert seen == [6, 7] and tr2.steps_done == 8 == tr2.optimizer._step and [s for s, _ in hist2] == [8]


# ------------------------------------------------------------------------------------------------ two ranks
@pytest.mark.timeout(600)
def test_two_ranks_validate_to_the_same_value_on_equal_ema_weights():
    """tests/_ema_eval_ddp_worker.py: two ranks train two steps of the micro EDM model on halves of a global batch, then validate on
    different batches: the same value on both ranks, equal parameters inside and after the context"""
    res = run_ranks("_ema_eval_ddp_worker.py", timeout=400)
    assert res["values_equal"] and res["value"] > 0 and res["value"] == pytest.approx(res["by_hand"], rel=1e-6), res
    assert res["inside_equal"] and res["after_equal"] and res["inside_is_ema"] and res["restored"], res
    assert res["ema_differs"] and res["steps"] == 2, res
