"""Classifier on the HIP path (GPU): the three head entry points of csrc/classifier.hip called directly, the module against the
reference's fixture (tools/make_classifier_goldens.py), the training route, and FID / IS end to end.

Direct parity: each kernel is called through ctypes and held against the same formulas in float64 on the CPU, formed from the very
float32 inputs the kernel gets.  Outputs are slices out of NaN-filled device tensors with GUARD elements either side (the bands must
come back bit-unchanged), inputs must equal the clones taken before the call, and two successive calls must agree bit for bit.
Bars (none is a measurement): 1e-5 is tests/test_side_kernels_gpu.py's BAR_F32 for exact-fp32 kernels with a reduction or a
transcendental inside; 1e-3 is the suite's parity bar against the reference (conftest.rel_err / grad_err); the metrics are held to twice
the sensitivity the fixture tool measured on the reference's own values for embedding / logit noise of that 1e-3."""


import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import cfg_of, grad_err, load_golden, rel_err

pytestmark = pytest.mark.gpu

GUARD = 64
BAR_F32 = 1e-5
OPT = {"learning_rate": 1e-3, "max_steps": 10, "eta_min": 0.0}


def dev():
    return torch.device("cuda:0")


def lib():
    from tqdne_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()])


class Out:
    """n output elements in the middle of a NaN-filled device tensor"""

    def __init__(self, *shape):
        self.shape = shape
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), device=dev())
        self.view = self.buf[GUARD:GUARD + self.n]
        self.before = self.bands()

    def bands(self):
        v = bits(self.buf)
        return torch.cat([v[:GUARD], v[GUARD + self.n:]]).clone()

    def ptr(self):
        return self.view.data_ptr()

    def cpu(self):
        return self.view.cpu().reshape(self.shape)


class Case:
    """the device tensors of one call: inputs with their clones, outputs with their guard bands"""

    def __init__(self):
        self.ins, self.outs = [], []

    def inp(self, t):
        d = t.contiguous().to(dev())
        self.ins.append((d, d.clone()))
        return d

    def out(self, *shape):
        o = Out(*shape)
        self.outs.append(o)
        return o

    def verify(self):
        torch.cuda.synchronize()
        for i, (d, c) in enumerate(self.ins):
            assert torch.equal(bits(d), bits(c)), f"input {i} was written"
        for i, o in enumerate(self.outs):
            assert torch.equal(o.bands(), o.before), f"guard band of output {i} was written"
            assert not torch.isnan(o.view).any(), f"output {i} was not written everywhere"


def ok(rc):
    assert rc == 0, f"library call returned {rc}"


def p(t):
    return None if t is None else (t.ptr() if isinstance(t, Out) else t.data_ptr())


def c_max():
    return lib().tq_classifier_head_max_channels()


# (B, T, C, K); C_max is filled in at run time; the launchers have no grid cap (one workgroup per sample in grid.x): B = 130
HEAD_SHAPES = [(1, 1, 32, 2), (5, 37, 96, 7), (3, 130, 256, 36), (2, 5, "max", 3), (130, 3, 32, 7)]


def head_inputs(B, T, C, K, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    h = r(B, T, C) + 0.5 * r(B, 1, C)   # a per-sample mean that survives the pooling
    W1, W2, W3 = r(C, C) * (2.0 / C ** 0.5), r(C, C) * (2.0 / C ** 0.5), r(K, C) * (2.0 / C ** 0.5)
    b1, b2, b3 = 0.3 * r(C), 0.3 * r(C), 0.3 * r(K)
    return h, W1, b1, W2, b2, W3, b3


def head_ref(h, W1, b1, W2, b2, W3, b3):
    """the head in float64 from the float32 inputs: (pooled, a1, emb, logits)"""
    h, W1, b1, W2, b2, W3, b3 = (t.double() for t in (h, W1, b1, W2, b2, W3, b3))
    pooled = h.mean(1)
    a1 = F.linear(F.silu(pooled), W1, b1)
    emb = F.linear(F.silu(a1), W2, b2)
    return pooled, a1, emb, F.linear(emb, W3, b3)


def run_head_fwd(ins, with_logits=True):
    h = ins[0]
    B, T, C = h.shape
    K = ins[5].shape[0]
    case = Case()
    d = [case.inp(t) for t in ins]
    outs = [case.out(B, C), case.out(B, C), case.out(B, C)] + ([case.out(B, K)] if with_logits else [])
    ok(lib().tq_classifier_head_fwd(*[p(t) for t in d], p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]) if with_logits else None,
                                    B, T, C, K, stream()))
    case.verify()
    return [o.cpu() for o in outs], d


def shape_of(s):
    B, T, C, K = s
    return B, T, (c_max() if C == "max" else C), K


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=str)
def test_head_forward(shape):
    B, T, C, K = shape_of(shape)
    ins = head_inputs(B, T, C, K, B + T)
    ref = head_ref(*ins)
    got, _ = run_head_fwd(ins)
    for name, a, b in zip(("pooled", "a1", "emb", "logits"), got, ref):
        e = rel_err(a, b)
        print(f"head fwd {shape} {name}: {e:.2e}")
        assert e < BAR_F32, name
    again, _ = run_head_fwd(ins)
    for a, b in zip(got, again):
        assert torch.equal(bits(a), bits(b))   # fixed-order sums, no atomics
    emb_only, _ = run_head_fwd(ins, with_logits=False)   # logits = NULL: embed() only
    for a, b in zip(got[:3], emb_only):
        assert torch.equal(bits(a), bits(b))


def run_head_bwd(ins, saved, dl, embed_only=False):
    h, W1, b1, W2, b2, W3, b3 = ins
    B, T, C = h.shape
    K = W3.shape[0]
    case = Case()
    d_dl, d_pooled, d_a1, d_emb = (case.inp(t) for t in (dl, *saved))
    dW1, dW2, dW3 = case.inp(W1), case.inp(W2), case.inp(W3)
    names = ("dW3", "db3", "dW2", "db2", "dW1", "db1", "dh")
    outs = dict(dW3=case.out(K, C), db3=case.out(K), dW2=case.out(C, C), db2=case.out(C), dW1=case.out(C, C), db1=case.out(C),
                dh=case.out(B, T, C))
    nws = lib().tq_classifier_head_bwd_workspace(B, C)
    ws = case.out(nws // 4)
    if embed_only:   # never written: take them out of the "written everywhere" check
        case.outs = [o for o in case.outs if o is not outs["dW3"] and o is not outs["db3"]]
    case.outs.remove(ws)   # (scratch: its bands are checked below, its contents are the kernel's own)
    ok(lib().tq_classifier_head_bwd(p(d_dl), p(d_pooled), p(d_a1), p(d_emb), p(dW1), p(dW2), None if embed_only else p(dW3),
                                    None if embed_only else p(outs["dW3"]), None if embed_only else p(outs["db3"]), p(outs["dW2"]),
                                    p(outs["db2"]), p(outs["dW1"]), p(outs["db1"]), p(outs["dh"]), p(ws), nws, B, T, C, K, stream()))
    case.verify()
    assert torch.equal(ws.bands(), ws.before), "guard band of the workspace was written"
    return {n: outs[n].cpu() for n in names if not (embed_only and n in ("dW3", "db3"))}


def head_bwd_ref(ins, dl, embed_only=False):
    """float64 autograd of the same head, seeded with ``dl`` (d logits, or d emb for the embed-only form)"""
    leaves = [t.double().requires_grad_(True) for t in ins]
    _, _, emb, logits = head_ref(*leaves)
    ((emb if embed_only else logits) * dl.double()).sum().backward()
    h, W1, b1, W2, b2, W3, b3 = leaves
    g = dict(dW2=W2.grad, db2=b2.grad, dW1=W1.grad, db1=b1.grad, dh=h.grad)
    if not embed_only:
        g.update(dW3=W3.grad, db3=b3.grad)
    return g


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=str)
def test_head_backward(shape):
    B, T, C, K = shape_of(shape)
    ins = head_inputs(B, T, C, K, B + T + 1)
    dl = torch.randn(B, K, generator=torch.Generator().manual_seed(5)) / B
    (pooled, a1, emb, _), _ = run_head_fwd(ins)    # the backward reads what the forward kernel saved
    got = run_head_bwd(ins, (pooled, a1, emb), dl)
    ref = head_bwd_ref(ins, dl)
    for name, b in ref.items():
        e = rel_err(got[name], b)
        print(f"head bwd {shape} {name}: {e:.2e}")
        assert e < BAR_F32, name
    again = run_head_bwd(ins, (pooled, a1, emb), dl)
    for name in got:
        assert torch.equal(bits(got[name]), bits(again[name])), name
    if shape in (HEAD_SHAPES[1], HEAD_SHAPES[3]):   # W3 = NULL: the incoming gradient is d emb
        de = torch.randn(B, C, generator=torch.Generator().manual_seed(6)) / B
        got = run_head_bwd(ins, (pooled, a1, emb), de, embed_only=True)
        for name, b in head_bwd_ref(ins, de, embed_only=True).items():
            e = rel_err(got[name], b)
            print(f"head bwd (embed only) {shape} {name}: {e:.2e}")
            assert e < BAR_F32, name


def run_ce(logits, labels, weight, ignore_index, want_d=True):
    B, K = logits.shape
    case = Case()
    d_l, d_y = case.inp(logits), case.inp(labels)
    d_w = None if weight is None else case.inp(weight)
    loss, dlog = case.out(1), (case.out(B, K) if want_d else None)
    ok(lib().tq_cross_entropy(p(d_l), p(d_y), p(d_w), ignore_index, p(loss), p(dlog), B, K, stream()))
    case.verify()
    return loss.cpu(), (dlog.cpu() if want_d else None)


CE_CASES = [  # (B, K, class weights?, ignored labels, logit scale)
    (1, 2, False, 0, 1.0), (5, 7, True, 1, 1.0), (5, 7, False, 0, 1.0), (130, 36, True, 9, 3.0), (300, 36, False, 1, 1.0),
    (37, 7, True, 3, 100.0), (6, 1024, True, 2, 100.0)]


@pytest.mark.parametrize("case", CE_CASES, ids=str)
def test_cross_entropy(case):
    B, K, weighted, n_ignored, scale = case
    g = torch.Generator().manual_seed(B * 31 + K)
    logits = torch.randn(B, K, generator=g)
    logits = logits * (scale / logits.abs().max()) if scale == 100.0 else logits * scale   # +-100: exp overflows fp32 un-shifted
    labels = torch.randint(0, K, (B,), generator=g)
    ignore_index = -100 if B != 130 else 4   # (also an ignore_index that is a class)
    labels[labels == ignore_index] = 5
    labels[torch.randperm(B, generator=g)[:n_ignored]] = ignore_index
    weight = (0.2 + torch.rand(K, generator=g)) if weighted else None
    lg = logits.double().requires_grad_(True)
    ref = F.cross_entropy(lg, labels, None if weight is None else weight.double(), ignore_index=ignore_index, reduction="mean")
    ref.backward()
    loss, dlog = run_ce(logits, labels, weight, ignore_index)
    e_l, e_d = rel_err(loss.reshape(()), ref.detach()), rel_err(dlog, lg.grad)
    print(f"cross entropy {case}: loss {e_l:.2e} dlogits {e_d:.2e}")
    assert e_l < BAR_F32 and e_d < BAR_F32
    assert (dlog[labels == ignore_index] == 0).all()
    loss2, dlog2 = run_ce(logits, labels, weight, ignore_index)
    assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(dlog), bits(dlog2))
    loss3, _ = run_ce(logits, labels, weight, ignore_index, want_d=False)   # dlogits = NULL
    assert torch.equal(bits(loss), bits(loss3))


# ============================================================================================================================
# module parity against the reference
# ============================================================================================================================
def build(name, loss=None, K=None, **cfg_over):
    from tqdne_amd import LithningClassifier
    sd, d = load_golden(name)
    K = sd["output_layer.weight"].shape[0] if K is None else K
    if loss is None:
        loss = nn.CrossEntropyLoss(weight=sd["loss.weight"].clone())
    clf = LithningClassifier(dict(cfg_of(d), **cfg_over), K, loss, [], OPT)
    if K == sd["output_layer.weight"].shape[0]:
        clf.load_state_dict(sd, strict=isinstance(loss, nn.CrossEntropyLoss) and loss.weight is not None)
    return clf.to(dev()), d


def batch_of(d):
    return {"signal": torch.from_numpy(d["x"]).to(dev()), "label": torch.from_numpy(d["label"]).to(dev())}


@pytest.mark.parametrize("name", ["micro_classifier.npz", "micro_classifier_b.npz"])
def test_module_matches_the_reference(name):
    clf, d = build(name)
    batch = batch_of(d)
    clf.eval()
    with torch.no_grad():
        emb, logits = clf.embed(batch["signal"]), clf(batch["signal"])
        e1, e2 = rel_err(emb.cpu(), d["embed"]), rel_err(logits.cpu(), d["logits"])
        assert torch.allclose(clf.output_layer(emb), logits, rtol=1e-4, atol=1e-4 * float(logits.abs().max()))
    clf.train()
    loss = clf.training_step(batch, 0)
    loss.backward()
    e3 = rel_err(loss.detach().cpu(), d["loss"])
    print(f"{name}: embed {e1:.2e} logits {e2:.2e} loss {e3:.2e}")
    assert max(e1, e2, e3) < 1e-3
    gmax = max(float(np.abs(d[k]).max()) for k in d if k.startswith("grad:"))
    worst = 0.0
    for pname, prm in clf.named_parameters():
        assert prm.grad is not None, pname
        worst = max(worst, grad_err(prm.grad, d["grad:" + pname], gmax, pname))
    print(f"{name}: worst gradient error {worst:.2e}")
    assert worst < 1e-3


def flat_grads(clf):
    return torch.cat([q.grad.reshape(-1) for q in clf.parameters()]).clone()


@pytest.mark.parametrize("fused", [True, False], ids=["fused_ce", "label_smoothing"])
def test_step_and_backward_equals_the_autograd_route(fused):
    """The encoder kernels are the same on both routes; only the loss arithmetic differs: 1e-5 of the largest gradient.  Measured on the
    fixture (logits of +-30): 8.3e-6 with the fused cross-entropy -- torch's fp32 log_softmax backward carries |logp| 2^-24 in the
    exponent, tq_cross_entropy is at 2e-7 of float64 -- and 8.9e-8 with a torch loss on both sides."""
    _, d0 = load_golden("micro_classifier.npz")
    w = torch.from_numpy(d0["x"]).new_tensor([1.0, 0.5, 2.0, 1.5, 0.7, 1.2, 0.9])
    loss_mod = nn.CrossEntropyLoss(weight=w) if fused else nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)
    clf, d = build("micro_classifier.npz", loss=loss_mod)
    batch = batch_of(d)
    clf.train()
    assert clf._fused_loss(batch["label"]) == fused
    loss_a = clf.training_step(batch, 0)
    loss_a.backward()
    ga = flat_grads(clf)
    clf.zero_grad(set_to_none=True)
    loss_b, flats = clf.step_and_backward(batch)
    gb = flat_grads(clf)
    assert sum(f.numel() for f in flats) == gb.numel()
    e = float((ga - gb).abs().max() / ga.abs().max())
    el = abs(float(loss_a.detach()) - float(loss_b)) / abs(float(loss_a.detach()))
    print(f"step_and_backward vs autograd ({'fused' if fused else 'torch loss'}): gradients {e:.2e} loss {el:.2e}")
    assert e <= 1e-5 and el <= 1e-5


def test_embed_under_autograd_equals_forward_through_an_identity_output_layer():
    """the W3 = NULL form of the backward: with output_layer = identity, forward(x) is embed(x) and every other gradient must agree"""
    clf, d = build("micro_classifier.npz", K=32, loss=nn.CrossEntropyLoss())
    sd, _ = load_golden("micro_classifier.npz")
    clf.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("output_layer", "loss"))}, strict=False)
    with torch.no_grad():
        clf.output_layer.weight.copy_(torch.eye(32))
        clf.output_layer.bias.zero_()
    clf.train()
    x = torch.from_numpy(d["x"]).to(dev()).requires_grad_(True)
    G = torch.randn(6, 32, generator=torch.Generator().manual_seed(1)).to(dev())
    res = []
    for fn in (clf.forward, clf.embed):
        clf.zero_grad(set_to_none=True)
        x.grad = None
        out = fn(x)
        (out * G).sum().backward()
        res.append((out.detach().clone(), x.grad.clone(),
                    torch.cat([q.grad.reshape(-1) for n, q in clf.named_parameters() if not n.startswith("output_layer")])))
    assert clf.output_layer.weight.grad is None   # (embed: the output layer is not part of the graph)
    (o1, dx1, g1), (o2, dx2, g2) = res
    assert torch.equal(o1, o2)
    assert float(dx1.abs().max()) > 0
    e_g, e_x = float((g1 - g2).abs().max() / g1.abs().max()), float((dx1 - dx2).abs().max() / dx1.abs().max())
    print(f"embed vs identity forward: gradients {e_g:.2e} dx {e_x:.2e}")
    assert e_g <= 1e-5 and e_x <= 1e-5
    with pytest.raises(RuntimeError, match="another forward"):
        out = clf.embed(x)
        clf.embed(x)
        out.sum().backward()


def test_trainer_steps_validation_and_checkpoint(tmp_path):
    from tqdne_amd import LithningClassifier
    from tqdne_amd.trainer import DataParallelTrainer
    clf, d = build("micro_classifier.npz")
    batch = batch_of(d)
    clf.train()
    tr = DataParallelTrainer(clf, world_size=1, ema_decay=0.999)
    assert tr.fused
    before = {n: q.detach().clone() for n, q in clf.named_parameters()}
    losses = [float(tr.train_step(batch)) for _ in range(3)]
    print("trainer losses:", losses)
    assert losses[2] < losses[0]
    for n, q in clf.named_parameters():
        assert not torch.equal(q.detach(), before[n]), f"{n} did not move"
    # validate: batch-weighted mean of validation_step on the EMA weights, eval mode, no gradients
    small = {k: v[:4].contiguous() for k, v in batch.items()}
    val = float(tr.validate([batch, small]))
    with tr.ema_weights(), torch.no_grad():
        clf.eval()
        want = (6 * float(clf.validation_step(batch, 0)) + 4 * float(clf.validation_step(small, 1))) / 10
        clf.train()
    assert val == pytest.approx(want, rel=1e-6)
    path = tmp_path / "clf.ckpt"
    tr.save_checkpoint(path)
    back = LithningClassifier.load_from_checkpoint(path).to(dev())
    clf.eval(), back.eval()
    with torch.no_grad():
        assert torch.equal(bits(clf.embed(batch["signal"])), bits(back.embed(batch["signal"])))


@pytest.mark.parametrize("batch_size", [32, None])
def test_fid_and_is_end_to_end(batch_size):
    from tqdne_amd import FrechetInceptionDistance, InceptionScore
    from tqdne_amd.representation import Identity
    clf, d = build("micro_classifier.npz")
    pred, target = d["set:pred"], d["set:target"]
    fid = FrechetInceptionDistance(clf, Identity(), batch_size=batch_size)(pred, target)
    iscore = InceptionScore(clf, Identity(), batch_size=batch_size)(pred)
    e_f, e_i = abs(fid - float(d["set:fid"])) / float(d["set:fid"]), abs(iscore - float(d["set:is"])) / float(d["set:is"])
    print(f"batch_size={batch_size}: FID {fid:.6f} (reference {float(d['set:fid']):.6f}, off {e_f:.2e}, bar {2 * float(d['fid_sens']):.2e}); "
          f"IS {iscore:.6f} (reference {float(d['set:is']):.6f}, off {e_i:.2e}, bar {2 * float(d['is_sens']):.2e})")
    assert e_f <= 2 * float(d["fid_sens"])
    assert e_i <= 2 * float(d["is_sens"])
