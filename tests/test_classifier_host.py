"""Classifier and metrics without a GPU: the module's schema and refusals, the C ABI's additions and their argument checks, the host
statistics of tqdne_amd.metric against the values the reference computed from the same arrays (tools/make_classifier_goldens.py), and
the dims=2 classifier (stock-PyTorch family) against the reference on the CPU."""

import os
import warnings

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN, cfg_of, load_golden, rel_err

OPT = {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}
TQ_ERR_ARG, TQ_ERR_SHAPE = -1, -2


def build(name, K=None):
    from tqdne_amd import LithningClassifier
    sd, d = load_golden(name)
    K = sd["output_layer.weight"].shape[0] if K is None else K
    w = sd.get("loss.weight")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = LithningClassifier(cfg_of(d), K, nn.CrossEntropyLoss(weight=None if w is None else w.clone()), [], OPT)
    return clf, sd, d


@pytest.mark.parametrize("name", ["micro_classifier.npz", "micro_classifier_b.npz", "micro_classifier_2d.npz"])
def test_state_dict_keys_and_order_equal_the_reference(name):
    clf, sd, _ = build(name)
    assert list(clf.state_dict().keys()) == list(sd.keys())
    assert [k for k in sd if not k.startswith("encoder.")] == [
        "output_MLP.1.weight", "output_MLP.1.bias", "output_MLP.3.weight", "output_MLP.3.bias", "output_layer.weight",
        "output_layer.bias", "loss.weight"]
    clf.load_state_dict(sd)
    assert type(clf.output_layer) is nn.Linear and isinstance(clf.output_MLP, nn.Sequential)


def test_configure_optimizers_types():
    clf, _, _ = build("micro_classifier.npz")
    cfg = clf.configure_optimizers()
    assert type(cfg["optimizer"]) is torch.optim.Adam
    assert type(cfg["lr_scheduler"]["scheduler"]) is torch.optim.lr_scheduler.CosineAnnealingLR
    assert cfg["lr_scheduler"]["interval"] == "step"
    assert cfg["optimizer"].param_groups[0]["lr"] == OPT["learning_rate"]
    assert len(cfg["optimizer"].param_groups[0]["params"]) == len(list(clf.parameters()))


def test_unsupported_widths_are_refused_at_construction():
    from tqdne_amd import LithningClassifier, _lib
    _, _, d = build("micro_classifier.npz")
    limit = _lib.load().tq_classifier_head_max_channels()
    for oc in (8, 16, 48, 100, limit + 32):
        with pytest.raises(NotImplementedError, match=str(limit)):
            LithningClassifier(dict(cfg_of(d), out_channels=oc), 7, nn.CrossEntropyLoss(), [], OPT)
    with pytest.raises(NotImplementedError):
        LithningClassifier(cfg_of(d), _lib.load().tq_classifier_head_max_classes() + 1, nn.CrossEntropyLoss(), [], OPT)
    LithningClassifier(dict(cfg_of(d), out_channels=64), 3, nn.MSELoss(), [], OPT)   # metrics=[] and any loss module


def test_abi_and_limits_without_a_device():
    from tqdne_amd import _lib
    lib = _lib.load()
    assert lib.tq_abi_version() == _lib.ABI_VERSION
    new = {"tq_classifier_head_fwd", "tq_classifier_head_bwd", "tq_cross_entropy", "tq_classifier_head_max_channels",
           "tq_classifier_head_max_classes", "tq_classifier_head_bwd_workspace"}
    assert new <= set(_lib.exported_symbols())
    assert lib.tq_classifier_head_max_channels() >= 1024
    assert lib.tq_classifier_head_max_classes() >= 36
    assert lib.tq_classifier_head_bwd_workspace(3, 64) == 5 * 3 * 64 * 4
    assert lib.tq_classifier_head_bwd_workspace(0, 64) == 0


def test_argument_checks_before_the_device_is_touched():
    from tqdne_amd import _lib
    lib = _lib.load()
    f = 0x1000   # never dereferenced: every call below is rejected during validation
    cmax, kmax = lib.tq_classifier_head_max_channels(), lib.tq_classifier_head_max_classes()
    fwd = [f] * 11
    for i in range(11):
        if i in (5, 6, 10):
            continue   # W3, b3 and logits: the embed-only form
        a = list(fwd)
        a[i] = None
        assert lib.tq_classifier_head_fwd(*a, 2, 8, 32, 7, None) == TQ_ERR_ARG, i
    a = list(fwd)
    a[5] = None   # logits wanted, W3 missing
    assert lib.tq_classifier_head_fwd(*a, 2, 8, 32, 7, None) == TQ_ERR_ARG
    for B, T, C, K, rc in ((2, 8, 48, 7, TQ_ERR_SHAPE), (2, 8, cmax + 32, 7, TQ_ERR_SHAPE), (2, 8, 32, kmax + 1, TQ_ERR_SHAPE),
                           (2, 0, 32, 7, TQ_ERR_ARG), (0, 8, 32, 7, TQ_ERR_ARG), (2, 8, 0, 7, TQ_ERR_ARG), (2, 8, 32, 0, TQ_ERR_ARG),
                           (2, -3, 48, 7, TQ_ERR_ARG)):
        assert lib.tq_classifier_head_fwd(*fwd, B, T, C, K, None) == rc, (B, T, C, K)
        assert lib.tq_classifier_head_bwd(*([f] * 15), 1 << 30, B, T, C, K, None) == rc, (B, T, C, K)
    bwd = [f] * 15
    for i in range(15):
        if i in (6, 7, 8):
            continue   # W3, dW3, db3: the embed-only form
        a = list(bwd)
        a[i] = None
        assert lib.tq_classifier_head_bwd(*a, 1 << 30, 2, 8, 32, 7, None) == TQ_ERR_ARG, i
    a = list(bwd)
    a[7] = None   # W3 given, dW3 missing
    assert lib.tq_classifier_head_bwd(*a, 1 << 30, 2, 8, 32, 7, None) == TQ_ERR_ARG
    assert lib.tq_classifier_head_bwd(*bwd, 5 * 2 * 32 * 4 - 1, 2, 8, 32, 7, None) == TQ_ERR_ARG   # workspace one byte short
    for i in (0, 1, 4):   # logits, labels, loss_out; weight (2) and dlogits (5) are nullable
        a = [f, f, None, -100, f, None]
        a[i] = None
        assert lib.tq_cross_entropy(*a, 4, 7, None) == TQ_ERR_ARG, i
    assert lib.tq_cross_entropy(f, f, None, -100, f, None, 0, 7, None) == TQ_ERR_ARG
    assert lib.tq_cross_entropy(f, f, None, -100, f, None, 4, 0, None) == TQ_ERR_ARG
    assert lib.tq_cross_entropy(f, f, None, -100, f, None, 4, kmax + 1, None) == TQ_ERR_SHAPE


# ---------------------------------------------------------------------------------------------------------------- metrics
def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_host_statistics_equal_the_reference():
    """the same float64 numpy / scipy arithmetic on the very arrays the reference saw"""
    from tqdne_amd import metric
    _, d = load_golden("micro_classifier.npz")
    ep, et = d["set:emb_pred"], d["set:emb_target"]
    assert rel(metric.frechet_distance(ep, et), d["set:fid"]) <= 1e-9
    assert rel(metric.frechet_distance(ep, et, isotropic=True), d["set:fd_isotropic"]) <= 1e-9
    assert rel(metric.inception_score(d["set:prob_pred"]), d["set:is"]) <= 1e-9
    pred, target = torch.from_numpy(d["set:pred"]), torch.from_numpy(d["set:target"])
    fs = int(d["set:fs"])
    assert rel(metric.AmplitudeSpectralDensity(fs=fs, channel=0)(pred, target), d["set:asd"]) <= 1e-9
    assert rel(metric.AmplitudeSpectralDensity(fs=fs, channel=1, isotropic=False)(pred, target), d["set:asd_full"]) <= 1e-9
    assert rel(metric.MeanSquaredError(channel=0)(pred, target), d["set:mse"]) <= 1e-9
    assert rel(metric.MeanSquaredError(channel=None)(d["set:pred"], d["set:target"]), d["set:mse_all"]) <= 1e-9
    assert metric.MeanSquaredError(channel=2).name == "MeanSquaredError - Channel 2"


def test_fixture_conditions_hold():
    """what the golden tool asserted on the reference's values before writing: a fixture that can tell a wrong metric from a right one"""
    _, d = load_golden("micro_classifier.npz")
    K = d["set:prob_pred"].shape[1]
    assert 1.5 <= float(d["set:is"]) <= K - 0.5 and float(d["set:fid"]) >= 0.1
    assert float(d["fid_sens"]) <= 1e-2 and float(d["is_sens"]) <= 1e-2
    for e in (d["set:emb_pred"], d["set:emb_target"]):
        ev = np.linalg.eigvalsh(np.cov(e, rowvar=False))
        assert ev[0] >= 1e-6 * ev[-1]
    for name in ("micro_classifier.npz", "micro_classifier_b.npz", "micro_classifier_2d.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 1_000_000


def test_frechet_distance_singular_and_imaginary_paths(capsys):
    from tqdne_amd.metric import frechet_distance
    g = np.random.default_rng(3)
    x = g.standard_normal((40, 5))
    assert abs(frechet_distance(x, x)) < 1e-6
    assert frechet_distance(x, x + 2.0) == pytest.approx(20.0, rel=1e-6)   # equal covariances: |mu_x - mu_y|^2
    rank1 = np.outer(g.standard_normal(40), np.ones(5))   # singular covariances: finite, real result
    assert np.isfinite(frechet_distance(rank1, rank1 * 2.0))


def test_neural_metrics_are_instantiable_and_batch():
    """FID / IS can be built (the reference's cannot) and ``batch_size=None`` means everything at once"""
    from tqdne_amd import FrechetInceptionDistance, InceptionScore, metric
    from tqdne_amd.representation import Identity

    class Fake(nn.Module):   # a classifier whose embedding is the per-channel mean and std
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(6, 4)
            self.calls = []

        device, dtype = torch.device("cpu"), torch.float32

        def embed(self, x):
            self.calls.append(len(x))
            return torch.cat([x.mean(-1), x.std(-1)], dim=1)

        def forward(self, x):
            return self.lin(self.embed(x))

    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(50, 3, 40, generator=g).numpy(), (1.5 * torch.randn(50, 3, 40, generator=g) + 0.2).numpy()
    clf = Fake()
    vals = []
    for bs, calls in ((None, [50, 50]), (16, [16, 16, 16, 2] * 2), (50, [50, 50])):
        clf.calls.clear()
        m = FrechetInceptionDistance(clf, Identity(), batch_size=bs)
        vals.append(m(a, b))
        assert clf.calls == calls and m.name == "FrechetInceptionDistance"
    assert vals[0] == pytest.approx(vals[1], rel=1e-6) and vals[0] > 0
    with torch.no_grad():
        e = lambda s: clf.embed(torch.from_numpy(s)).numpy()
        p = torch.softmax(clf(torch.from_numpy(a)), -1).numpy()
    assert vals[0] == pytest.approx(metric.frechet_distance(e(a), e(b)), rel=1e-6)
    for bs in (None, 7):
        assert InceptionScore(clf, Identity(), batch_size=bs)(a) == pytest.approx(metric.inception_score(p), rel=1e-5)
    assert not clf.training


# ---------------------------------------------------------------------------------------------------------------- dims = 2
def test_dims2_classifier_matches_the_reference_on_the_cpu():
    """embed, logits, loss and every gradient of training_step through torch.autograd; bars of tests/test_family2d.py"""
    clf, sd, d = build("micro_classifier_2d.npz")
    clf.load_state_dict(sd)
    clf.eval()
    x, y = torch.from_numpy(d["x"]), torch.from_numpy(d["label"])
    with torch.no_grad():
        assert rel_err(clf.embed(x), d["embed"]) < 1e-4
        logits = clf(x)
        assert rel_err(logits, d["logits"]) < 1e-4
        assert torch.allclose(clf.output_layer(clf.embed(x)), logits)   # evaluate.py's classifier.output_layer(embedding)
    clf.train()
    loss = clf.training_step({"signal": x, "label": y}, 0)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(d["loss"]), rel=1e-5)
    assert clf._logged["training/loss"] == pytest.approx(float(d["loss"]), rel=1e-5)
    n = 0
    for name, p in clf.named_parameters():
        assert rel_err(p.grad, d["grad:" + name]) < 1e-4, name
        n += 1
    assert n == len([k for k in d if k.startswith("grad:")])
    with pytest.raises(NotImplementedError):
        clf.step_and_backward({"signal": x, "label": y})
    clf.eval()
    with torch.no_grad():
        val = clf.validation_step({"signal": x, "label": y}, 0)
    assert float(val) == pytest.approx(float(d["loss"]), rel=1e-5)


def test_checkpoint_round_trip_keeps_the_loss_module(tmp_path):
    from tqdne_amd import LithningClassifier, checkpoint
    clf, sd, _ = build("micro_classifier.npz")
    clf.load_state_dict(sd)
    path = tmp_path / "clf.ckpt"
    checkpoint.save_checkpoint(clf, path)
    back = LithningClassifier.load_from_checkpoint(path)
    assert type(back.loss) is nn.CrossEntropyLoss
    for (ka, a), (kb, b) in zip(clf.state_dict().items(), back.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka


def test_1d_classifier_has_no_cpu_fallback():
    clf, sd, d = build("micro_classifier.npz")
    with pytest.raises(RuntimeError, match="HIP"):
        clf.embed(torch.from_numpy(d["x"]))
