"""Validation and sampling on the EMA weights, checkpoints and resuming -- the part that needs no GPU: ``tq_ema_swap`` is declared,
exported and bound and refuses bad arguments before the device is touched;
DataParallelTrainer's ``ema_weights`` / ``validate`` / ``evaluate`` / ``save_checkpoint`` / ``load_checkpoint`` / ``fit`` on the unfused
path (torch's optimizer on a CPU stub module); ``validate`` over two gloo ranks."""

import ctypes as C
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

ERR_ARG = -1
EMA = 0.9


def test_ema_swap_is_declared_exported_and_bound():
    from tqdne_amd import _build, _lib
    _build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tqdne_hip.h")).read()
    assert re.search(r"\bint\s+tq_ema_swap\s*\(\s*const TqAdamChunk\*\s*chunks,\s*int n_chunks,\s*hipStream_t stream\)", header)
    assert "tq_ema_swap" in _lib.exported_symbols() and hasattr(lib, "tq_ema_swap")
    assert lib.tq_abi_version() == _lib.ABI_VERSION


def test_ema_swap_refuses_bad_arguments_before_the_device_is_touched():
    """(this box has no device: anything that got as far as a launch would not return these codes)"""
    from tqdne_amd import _build, _lib
    _build.build(verbose=False)
    lib = _lib.load()
    table = C.cast((_lib.TqAdamChunk * 2)(), C.c_void_p)
    assert lib.tq_ema_swap(None, 4, None) == ERR_ARG      # a null table with chunks to do
    assert lib.tq_ema_swap(table, -1, None) == ERR_ARG    # a negative count
    assert lib.tq_ema_swap(None, -1, None) == ERR_ARG
    assert lib.tq_ema_swap(table, 0, None) == 0           # nothing to do: no launch
    assert lib.tq_ema_swap(None, 0, None) == 0


def test_swap_ema_and_step_guards_need_no_device():
    """the checks in front of every launch, on an optimizer object that was never constructed (as tests/test_grad_clip_host.py does)"""
    from tqdne_amd.optim import _FusedFlatOptimizer
    opt = object.__new__(_FusedFlatOptimizer)
    assert opt.ema_swapped is False
    opt._ema = None
    with pytest.raises(RuntimeError, match="constructed without ema_decay"):
        opt.swap_ema()
    opt.ema_swapped = True
    with pytest.raises(RuntimeError, match="EMA weights"):
        _FusedFlatOptimizer.step(opt)


# ---------------------------------------------------------------------------------------------------- the trainer on a CPU stub module
class _Stub(torch.nn.Module):
    """what the trainer sees of a module: configure_optimizers (Lightning's dict form), step_and_backward, validation_step, evaluate.
    One frozen parameter and one buffer: neither is the EMA callback's business."""

    def __init__(self, lr=5e-2):
        super().__init__()
        torch.manual_seed(0)
        self.lin = torch.nn.Linear(6, 3)
        self.frozen = torch.nn.Parameter(torch.full((3,), 0.25), requires_grad=False)
        self.register_buffer("buf", torch.arange(3.0))
        self.drop = torch.nn.Dropout(0.5)
        self.lr = lr
        self.modes = []   # module.training as every validation_step saw it

    def configure_optimizers(self):
        opt = torch.optim.Adam([p for p in self.parameters() if p.requires_grad], lr=self.lr)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=50)}}

    def _loss(self, batch):
        return ((self.drop(self.lin(batch["signal"])) + self.frozen - batch["cond"]) ** 2).mean()

    def step_and_backward(self, batch):
        loss = self._loss(batch)
        ps = list(self.lin.parameters())
        for p, g in zip(ps, torch.autograd.grad(loss, ps)):
            p.grad = g
        return loss.detach(), [p.grad for p in ps]

    def validation_step(self, batch, batch_idx):
        assert not torch.is_grad_enabled()
        self.modes.append(self.training)
        return self._loss(batch)

    def evaluate(self, batch):
        assert not torch.is_grad_enabled() and not self.training
        return self.lin(batch["signal"])


def _batches(sizes, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [{"signal": torch.randn(b, 6, generator=g), "cond": torch.randn(b, 3, generator=g)} for b in sizes]


def _trained(steps=3, **kw):
    from tqdne_amd.trainer import DataParallelTrainer
    m = _Stub().train()
    tr = DataParallelTrainer(m, fused_optimizer=False, **kw)
    for b in _batches([8] * steps):
        m.drop.p = 0.0   # (train_step without dropout noise; validation runs in eval mode anyway)
        tr.train_step(b)
    return m, tr


def _snapshot(m, tr):
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ema = {k: v.detach().clone() for k, v in tr.ema_state().items()} if tr.ema_decay is not None else {}
    return sd, ema


def _same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def test_ema_weights_context_swaps_in_and_restores_bit_for_bit():
    m, tr = _trained(ema_decay=EMA)
    sd0, ema0 = _snapshot(m, tr)
    assert set(ema0) == {"lin.weight", "lin.bias"}
    assert not any(torch.equal(sd0[k], ema0[k]) for k in ema0), "three steps must separate the EMA from the weights"
    versions = {n: p._version for n, p in m.named_parameters()}
    with tr.ema_weights() as inside:
        assert inside is m
        sd1, ema1 = _snapshot(m, tr)
        for k in ema0:
            assert torch.equal(sd1[k], ema0[k]), k                       # the module holds the EMA ...
        assert torch.equal(sd1["frozen"], sd0["frozen"]) and torch.equal(sd1["buf"], sd0["buf"])   # ... and nothing else moved
        assert _same_bits(ema1, ema0)                                   # ema_state() still means the EMA of the run
        assert all(m.get_parameter(n)._version > versions[n] for n in ema0)
        with pytest.raises(RuntimeError, match="does not nest"):
            with tr.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="train_step inside ema_weights"):
            tr.train_step(_batches([8])[0])
        with pytest.raises(RuntimeError, match="save_checkpoint inside ema_weights"):
            tr.save_checkpoint(os.devnull)
        assert _same_bits(_snapshot(m, tr)[0], sd1) and tr.steps_done == 3   # the refused calls changed nothing
    sd2, ema2 = _snapshot(m, tr)
    assert _same_bits(sd2, sd0) and _same_bits(ema2, ema0)
    # the context is usable again, and an exception in the body restores as well
    with pytest.raises(ZeroDivisionError):
        with tr.ema_weights():
            assert torch.equal(m.lin.weight, ema0["lin.weight"])
            1 / 0
    sd3, ema3 = _snapshot(m, tr)
    assert _same_bits(sd3, sd0) and _same_bits(ema3, ema0) and not tr._ema_active
    tr.train_step(_batches([8])[0])   # and training goes on
    assert tr.steps_done == 4


def test_ema_weights_without_an_ema_raises():
    m, tr = _trained(steps=1)
    with pytest.raises(RuntimeError, match="constructed without ema_decay"):
        with tr.ema_weights():
            pass


def _by_hand(m, weights, batches):
    """batch-weighted mean of the validation loss of a fresh stub holding ``weights``, in eval mode"""
    ref = _Stub().eval()
    ref.load_state_dict(weights, strict=False)
    with torch.no_grad():
        return sum(float(ref._loss(b)) * b["signal"].shape[0] for b in batches) / sum(b["signal"].shape[0] for b in batches)


def test_validate_runs_on_the_ema_weights_in_eval_mode_and_weights_by_batch_size():
    m, tr = _trained(ema_decay=EMA)
    m.drop.p = 0.5       # (a pass left in training mode would show)
    sd0, ema0 = _snapshot(m, tr)
    val = _batches([5, 2, 7], seed=11)
    got = tr.validate(val)
    assert got.dim() == 0 and got.dtype == torch.float32
    assert float(got) == pytest.approx(_by_hand(m, ema0, val), rel=1e-6)
    assert float(got) != pytest.approx(_by_hand(m, sd0, val), rel=1e-3)   # not the training weights
    assert m.modes == [False] * 3 and m.training and m.drop.training
    assert _same_bits(_snapshot(m, tr)[0], sd0)
    assert float(tr.validate(val, limit_batches=2)) == pytest.approx(_by_hand(m, ema0, val[:2]), rel=1e-6)
    m.eval()
    tr.validate(val[:1])
    assert not m.training, "the mode is put back, whatever it was"
    # evaluate: the same conditions, the module's samples
    m.train()
    out = tr.evaluate(val[0])
    assert torch.equal(out, torch.nn.functional.linear(val[0]["signal"], ema0["lin.weight"], ema0["lin.bias"])) and m.training


def test_validate_without_an_ema_uses_the_training_weights():
    m, tr = _trained()
    sd0, _ = _snapshot(m, tr)
    val = _batches([4, 6], seed=11)
    assert float(tr.validate(val)) == pytest.approx(_by_hand(m, sd0, val), rel=1e-6)


def test_save_and_load_put_a_fresh_trainer_where_the_first_one_stopped(tmp_path):
    from tqdne_amd import rng
    from tqdne_amd.checkpoint import load_checkpoint
    from tqdne_amd.trainer import DataParallelTrainer
    rng.reset_dropout_counter(17)
    m, tr = _trained(ema_decay=EMA)
    path = str(tmp_path / "a.ckpt")
    tr.save_checkpoint(path, epoch=2)
    raw = load_checkpoint(path)
    assert raw["global_step"] == 3 and raw["epoch"] == 2 and set(raw["ema_state"]) == {"lin.weight", "lin.bias"}
    assert raw["tqdne_amd_trainer"] == {"dropout_counter": 17, "steps_done": 3, "conv_scheme": None}
    rng.reset_dropout_counter(0)
    m2 = _Stub().train()
    with torch.no_grad():
        for p in m2.lin.parameters():
            p.add_(1.0)
    tr2 = DataParallelTrainer(m2, fused_optimizer=False, ema_decay=EMA)
    versions = {n: p._version for n, p in m2.named_parameters()}
    tr2.load_checkpoint(path)
    assert _same_bits(*(s[0] for s in (_snapshot(m2, tr2), _snapshot(m, tr)))) and _same_bits(_snapshot(m2, tr2)[1], _snapshot(m, tr)[1])
    assert all(p._version > versions[n] for n, p in m2.named_parameters())
    for p, q in zip(m.lin.parameters(), m2.lin.parameters()):
        a, b = tr.optimizer.state[p], tr2.optimizer.state[q]
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"]) and float(a["step"]) == float(b["step"]) == 3
    assert tr2.steps_done == 3 and rng.dropout_counter() == 17
    assert tr2.scheduler.last_epoch == tr.scheduler.last_epoch == 3
    assert tr2.optimizer.param_groups[0]["lr"] == tr.optimizer.param_groups[0]["lr"] != m.lr
    for b in _batches([8, 8], seed=5):   # both go on alike, bit for bit (CPU, no dropout)
        m.drop.p = m2.drop.p = 0.0
        assert torch.equal(tr.train_step(b), tr2.train_step(b))
    assert _same_bits(_snapshot(m2, tr2)[0], _snapshot(m, tr)[0]) and _same_bits(_snapshot(m2, tr2)[1], _snapshot(m, tr)[1])
    rng.reset_dropout_counter(0)


def test_a_checkpoint_without_our_key_or_without_an_ema_loads(tmp_path):
    """what the reference's ModelCheckpoint writes: no ``tqdne_amd_trainer``; and a run without the EMA callback: no ``ema_state``"""
    from tqdne_amd.checkpoint import _RemapPickle, load_checkpoint
    from tqdne_amd.trainer import DataParallelTrainer
    m, tr = _trained(ema_decay=EMA)
    path = str(tmp_path / "a.ckpt")
    tr.save_checkpoint(path)
    raw = load_checkpoint(path)
    del raw["tqdne_amd_trainer"], raw["ema_state"]
    raw["global_step"] = 3
    torch.save(raw, path, pickle_module=_RemapPickle)
    m2 = _Stub().train()
    tr2 = DataParallelTrainer(m2, fused_optimizer=False, ema_decay=EMA)
    tr2.load_checkpoint(path)
    assert tr2.steps_done == 3
    sd2, ema2 = _snapshot(m2, tr2)
    assert _same_bits(sd2, _snapshot(m, tr)[0])
    for k in ema2:
        assert torch.equal(ema2[k], sd2[k]), "without ema_state the EMA starts from the loaded weights (the callback's on_fit_start)"


def test_fit_validates_checkpoints_keeps_the_best_and_resumes(tmp_path):
    from tqdne_amd.trainer import DataParallelTrainer
    train, val = _batches([8, 8, 8], seed=1), _batches([4, 2], seed=2)
    m = _Stub().train()
    m.drop.p = 0.0
    tr = DataParallelTrainer(m, fused_optimizer=False, ema_decay=EMA)
    d = str(tmp_path / "run")
    hist = tr.fit(train, val, max_steps=8, val_check_interval=2, dirpath=d, save_top_k=2)
    assert tr.steps_done == 8 and [s for s, _ in hist] == [2, 4, 6, 8]
    files = sorted(os.listdir(d))
    assert "last.ckpt" in files and len(files) == 3, files
    best2 = sorted(hist, key=lambda sv: sv[1])[:2]
    assert {f for f in files if f != "last.ckpt"} == {f"step={s}-val_loss={v:.2e}.ckpt" for s, v in best2}
    m2 = _Stub().train()
    m2.drop.p = 0.0
    tr2 = DataParallelTrainer(m2, fused_optimizer=False, ema_decay=EMA)
    hist2 = tr2.fit(train, val, max_steps=10, val_check_interval=2, ckpt_path=os.path.join(d, "last.ckpt"))
    assert tr2.steps_done == 10 and [s for s, _ in hist2] == [10]
    assert tr2.fit(train, max_steps=10) == [] and tr2.steps_done == 10   # nothing left to do


# ---------------------------------------------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _validate_worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tqdne_amd.trainer import DataParallelTrainer
    m = _Stub().train()
    tr = DataParallelTrainer(m, world_size=world, fused_optimizer=False, ema_decay=EMA)
    for b in _batches([8, 8], seed=20):
        m.drop.p = 0.0
        tr.train_step(b)   # (the same batch on both ranks: the replicas stay equal, which is all this test needs of training)
    calls = []
    orig = tr._allreduce_async
    tr._allreduce_async = lambda t: (calls.append(t.numel()), orig(t))[1]
    mine = _batches([3, 5] if rank == 0 else [2, 7, 4], seed=30 + rank)   # different batches, sizes and counts per rank
    got = float(tr.validate(mine))
    ema = {k: v.clone() for k, v in tr.ema_state().items()}
    both = _batches([3, 5], seed=30) + _batches([2, 7, 4], seed=31)
    ret[rank] = dict(got=got, want=_by_hand(m, ema, both), collectives=calls)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_gloo_world2_validate_is_the_batch_weighted_mean_over_both_ranks():
    world, port = 2, _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_validate_worker, args=(world, port, ret), nprocs=world, join=True)
    assert ret[0]["got"] == ret[1]["got"], "every rank returns the same value"
    for r in range(world):
        assert ret[r]["got"] == pytest.approx(ret[r]["want"], rel=1e-6)
        assert ret[r]["collectives"] == [2], "one collective of two words"
