#!/usr/bin/env python3
"""Generate tests/golden/micro_classifier.npz, micro_classifier_b.npz and micro_classifier_2d.npz by running the reference's own
``LithningClassifier`` and ``tqdne.metric`` on the CPU.

Run:  python tools/make_classifier_goldens.py            (needs the reference checkout of tools/make_goldens.py; CPU only)

The reference is imported at run time, never copied.  ``pytorch_lightning``, ``pathos`` and ``PIL`` get the in-memory stand-ins of
tools/make_goldens.py / tools/make_envelope_golden.py; ``torchmetrics`` (not installed here either) gets one for the two names
classifier.py imports.  None contributes arithmetic.  The reference's ``NeuralMetric.__call__`` is decorated ``@abstractmethod``, so its
FID / IS classes cannot be instantiated: the tool subclasses them with a ``__call__`` that calls ``NeuralMetric.__call__``.

A fresh classifier gives embeddings with a covariance of about 1e-5 and an inception score of 1.0000002, which pins nothing: after
``perturb_`` the weights are rescaled (see the constants below) so that embeddings and class probabilities vary across the inputs.  The tool asserts, on the
reference's values alone, before it writes anything:
  * the inception score is finite and in [1.5, K - 0.5];
  * the smallest eigenvalue of each embedding covariance is at least 1e-6 of the largest;
  * FID >= 0.1;
  * ``fid_sens`` and ``is_sens`` -- the largest relative change of the reference's FID / IS over 8 draws of Gaussian noise of
    1e-3 * rms (the suite's element-wise parity bar) added to its embeddings / logits -- are at most 1e-2.  Both are stored.

Files (arrays only):
  micro_classifier.npz     configuration (a): 7 classes with random positive class weights, T = 72, B = 6, one label -100; weights, x,
                           labels, embed, logits, loss, every parameter gradient of training_step; two sets of N = 96 inputs with
                           per-sample log-normal amplitudes, the reference's embeddings / probabilities / FID / isotropic Frechet
                           distance / IS / ASD / MSE on them, and the two sensitivities.
  micro_classifier_b.npz   configuration (b): the same trunk with out_channels = 96, 36 classes, T = 200 (a file of its own: the two
                           together would pass the size limit of a committed file).
  micro_classifier_2d.npz  a small dims=2 classifier: the same quantities, for the stock-PyTorch family.
"""

from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402

TRUNK = dict(in_channels=3, model_channels=32, channel_mult=(1, 2), out_channels=32, num_res_blocks=1, attention_resolutions=(2,),
             num_heads=2, conv_kernel_size=3, dropout=0.0, dims=1, flash_attention=False)
CFG_2D = dict(in_channels=2, model_channels=32, channel_mult=(1, 1), out_channels=32, num_res_blocks=1, attention_resolutions=(2,),
              num_heads=2, conv_kernel_size=3, dropout=0.0, dims=2, flash_attention=False)
OPT = {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}
N_SET, FS = 96, 100
# Tuned until the reference alone meets the asserted conditions:
HEAD_GAIN = (2.0, 2.0)           # output_MLP.1 / .3 weights: a random orthogonal matrix times this (two default-initialised square
                                 # matrices in a row have a condition number of 1e4: an embedding covariance of rank 32 in name only)
OUT_SCALE = 16.0                 # output_layer weight
ENC_OUT_SCALE = 2.0              # the encoder's output conv
BRANCH_SCALE = 5.0               # the zero-initialised convs that end the residual branches, after perturb_'s N(0, 0.02^2): without
                                 # them the trunk is almost linear and the pooled features are the input's three channel means


def install_standins():
    mg.install_lightning_standin()
    for name in ("pathos", "pathos.multiprocessing"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.Pool = None
            sys.modules[name] = m
    try:
        import PIL  # noqa: F401
    except ImportError:
        sys.modules["PIL"] = types.ModuleType("PIL")
    if "torchmetrics" not in sys.modules:
        tm = types.ModuleType("torchmetrics")

        class Metric(nn.Module):
            pass

        class MetricCollection(nn.ModuleList):
            def forward(self, preds, target):
                return {type(m).__name__: m(preds, target) for m in self}

        tm.Metric, tm.MetricCollection = Metric, MetricCollection
        sys.modules["torchmetrics"] = tm


def make_classifier(cls, cfg, K, seed, weighted=True):
    torch.manual_seed(seed)
    w = (0.5 + torch.rand(K)) if weighted else None
    clf = cls(cfg, K, nn.CrossEntropyLoss(weight=w), [], OPT)
    mg.perturb_(clf, seed + 1)
    go = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        for name, p in clf.named_parameters():
            if name.endswith("out_layers.3.weight") or name.endswith("proj_out.weight"):
                p.mul_(BRANCH_SCALE)
        clf.encoder.output_layer.weight.mul_(ENC_OUT_SCALE)
        for lin, gain in zip((clf.output_MLP[1], clf.output_MLP[3]), HEAD_GAIN):
            q, _ = torch.linalg.qr(torch.randn(lin.weight.shape, generator=go))
            lin.weight.copy_(gain * q)
        clf.output_layer.weight.mul_(OUT_SCALE)
    return clf


def step_fixture(clf, x, y):
    """embed, logits, loss and every parameter gradient of training_step, as the reference computes them"""
    fx = {"w:" + k: v.detach().numpy().copy() for k, v in clf.state_dict().items()}
    clf.eval()
    with torch.no_grad():
        fx["embed"] = clf.embed(x).numpy()
        fx["logits"] = clf(x).numpy()
    clf.train()
    clf.zero_grad()
    loss = clf.training_step({"signal": x, "label": y}, 0)
    loss.backward()
    fx.update(x=x.numpy(), label=y.numpy(), loss=loss.detach().numpy())
    for name, p in clf.named_parameters():
        fx["grad:" + name] = p.grad.numpy().copy()
    clf.zero_grad()
    clf.eval()
    return fx


def signal_set(g, n, T, colour):
    """n three-channel signals: per channel, white noise through a one-pole filter (pole drawn around ``colour``) plus two tones, a
    channel gain and an offset; per-sample log-normal amplitudes on top"""
    w = torch.randn(n, 3, T + 32, generator=g)
    pole = (colour + 0.3 * torch.randn(n, 3, generator=g)).clamp(-0.9, 0.9)
    y = torch.zeros_like(w)
    for k in range(1, T + 32):
        y[:, :, k] = pole * y[:, :, k - 1] + w[:, :, k]
    y = y[:, :, 32:]
    y = y / y.std(dim=2, keepdim=True)
    tt = torch.arange(T)[None, None, :]
    tone = 0
    for _ in range(2):
        freq = 0.02 + 0.4 * torch.rand(n, 3, 1, generator=g)
        phase = 6.2831853 * torch.rand(n, 3, 1, generator=g)
        tone = tone + torch.sin(6.2831853 * freq * tt + phase) * (2.0 * torch.rand(n, 3, 1, generator=g))
    dc = 0.5 * torch.randn(n, 3, 1, generator=g)
    gain = torch.exp(0.5 * torch.randn(n, 3, 1, generator=g))
    amp = torch.exp(0.7 * torch.randn(n, 1, 1, generator=g))
    return (((y + tone) * gain + dc) * amp).float().contiguous()


def main():
    sys.path.insert(0, mg.REF)
    install_standins()
    torch.set_num_threads(8)
    from tqdne.classifier import LithningClassifier
    from tqdne import metric as rm
    from tqdne.representation import Identity

    class FID(rm.FrechetInceptionDistance):
        def __call__(self, pred, target=None):
            return rm.NeuralMetric.__call__(self, pred, target)

    class IS(rm.InceptionScore):
        def __call__(self, pred, target=None):
            return rm.NeuralMetric.__call__(self, pred, target)

    g = torch.Generator().manual_seed(20240)

    # ---------------------------------------------------------------- (a): 7 classes, T = 72, B = 6, and the metric sets
    K = 7
    clf = make_classifier(LithningClassifier, TRUNK, K, 5)
    x = signal_set(g, 6, 72, 0.3)
    y = torch.tensor([3, 0, 6, -100, 1, 3])
    pred, target = signal_set(g, N_SET, 72, 0.5), signal_set(g, N_SET, 72, -0.3)
    with torch.no_grad():   # centre the logits on the first set: an un-trained head puts every input into one class
        clf.eval()
        clf.output_layer.bias.sub_(clf(pred).mean(0))
    fx = step_fixture(clf, x, y)
    fx["cfg"] = np.array(repr(TRUNK))
    with torch.no_grad():   # (in the metrics' batches of 32: the CPU kernels' last bits depend on the batch)
        emb_p, emb_t = (np.concatenate([clf.embed(s[i:i + 32]).numpy() for i in range(0, N_SET, 32)]) for s in (pred, target))
        logit_p = np.concatenate([clf(pred[i:i + 32]).numpy() for i in range(0, N_SET, 32)])
    prob_p = torch.softmax(torch.from_numpy(logit_p), dim=-1).numpy()
    rep = Identity()
    fid = float(FID(clf, rep, batch_size=32)(pred.numpy(), target.numpy()))
    iscore = float(IS(clf, rep, batch_size=32)(pred.numpy()))
    fid_direct = float(rm.frechet_distance(emb_p, emb_t))
    assert fid == fid_direct, (fid, fid_direct)   # (the stored embeddings are the ones the reference's metric saw)
    fd_iso = float(rm.frechet_distance(emb_p, emb_t, isotropic=True))
    asd = float(rm.AmplitudeSpectralDensity(fs=FS, channel=0)(pred, target))
    asd_full = float(rm.AmplitudeSpectralDensity(fs=FS, channel=1, isotropic=False)(pred, target))
    mse = float(rm.MeanSquaredError(channel=0)(pred, target))
    mse_all = float(rm.MeanSquaredError(channel=None)(pred, target))

    def is_of(logits):
        return float(rm.InceptionScore.compute(_FixedProbs(logits), torch.zeros(len(logits))))

    class _FixedProbs:   # the reference's own IS arithmetic on given logits: a "classifier" that returns them
        batch_size = len(logit_p)

        def __init__(self, logits):
            self._logits = torch.from_numpy(np.asarray(logits, dtype=np.float32))

        def classifier(self, _):
            return self._logits

    assert is_of(logit_p) == iscore, (is_of(logit_p), iscore)
    rng_ = np.random.default_rng(77)
    fid_sens = is_sens = 0.0
    for _ in range(8):
        ep = emb_p + 1e-3 * np.sqrt((emb_p ** 2).mean()) * rng_.standard_normal(emb_p.shape)
        et = emb_t + 1e-3 * np.sqrt((emb_t ** 2).mean()) * rng_.standard_normal(emb_t.shape)
        fid_sens = max(fid_sens, abs(float(rm.frechet_distance(ep, et)) - fid_direct) / fid_direct)
        lg = logit_p + 1e-3 * np.sqrt((logit_p ** 2).mean()) * rng_.standard_normal(logit_p.shape)
        is_sens = max(is_sens, abs(is_of(lg) - iscore) / iscore)
    eig = [np.linalg.eigvalsh(np.cov(e, rowvar=False)) for e in (emb_p, emb_t)]
    print(f"(a) FID {fid:.6g}  isotropic {fd_iso:.6g}  IS {iscore:.6g}  ASD {asd:.6g} / {asd_full:.6g}  MSE {mse:.6g}  "
          f"fid_sens {fid_sens:.3e}  is_sens {is_sens:.3e}  eig min/max {[float(e[0] / e[-1]) for e in eig]}")
    assert np.isfinite(iscore) and 1.5 <= iscore <= K - 0.5, iscore
    assert all(e[0] >= 1e-6 * e[-1] for e in eig), [float(e[0] / e[-1]) for e in eig]
    assert fid >= 0.1, fid
    assert fid_sens <= 1e-2 and is_sens <= 1e-2, (fid_sens, is_sens)
    fx.update({"set:pred": pred.numpy(), "set:target": target.numpy(), "set:emb_pred": emb_p, "set:emb_target": emb_t,
               "set:prob_pred": prob_p, "set:fid": np.float64(fid), "set:fd_isotropic": np.float64(fd_iso), "set:is": np.float64(iscore),
               "set:asd": np.float64(asd), "set:asd_full": np.float64(asd_full), "set:mse": np.float64(mse),
               "set:mse_all": np.float64(mse_all), "set:fs": np.int64(FS), "fid_sens": np.float64(fid_sens),
               "is_sens": np.float64(is_sens)})
    save("micro_classifier.npz", fx)

    # ---------------------------------------------------------------- (b): out_channels = 96, 36 classes, T = 200
    cfg_b = dict(TRUNK, out_channels=96)
    clf = make_classifier(LithningClassifier, cfg_b, 36, 9)
    x = signal_set(g, 6, 200, 0.3)
    y = torch.randint(0, 36, (6,), generator=g)
    fx = step_fixture(clf, x, y)
    fx["cfg"] = np.array(repr(cfg_b))
    save("micro_classifier_b.npz", fx)

    # ---------------------------------------------------------------- dims = 2 (stock-PyTorch family)
    clf = make_classifier(LithningClassifier, CFG_2D, 5, 13)
    x = torch.randn(3, 2, 16, 12, generator=g)
    y = torch.tensor([4, -100, 2])
    fx = step_fixture(clf, x, y)
    fx["cfg"] = np.array(repr(CFG_2D))
    save("micro_classifier_2d.npz", fx)


def save(name, fx):
    path = os.path.join(mg.OUT, name)
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print(name, size // 1024, "KiB")
    assert size < 1_000_000, (name, size)


if __name__ == "__main__":
    main()
