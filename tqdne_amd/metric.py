"""Evaluation metrics (third stage of the reference's workflow; counterpart of ``tqdne.metric``, metric.py:13-173): mean squared
error and amplitude spectral density on the signals themselves (the latter on the GPU for GPU tensors), Frechet inception distance
and inception score through a trained ``LithningClassifier``.

The embeddings / class probabilities come from the classifier module (on the GPU: the HIP encoder plan and head kernels), in batches of
``batch_size``; the statistics are formed on the host in float64 with numpy / scipy by the reference's formulas.  Two departures from
the reference, both where it cannot run: ``batch_size=None`` means the whole input at once (the reference's ``range(0, n, None)``
raises), and ``NeuralMetric.__call__`` is concrete (the reference decorates it ``@abstractmethod``, so its FID / IS classes cannot be
instantiated)."""

from __future__ import annotations

from abc import ABC, abstractmethod
from collections.abc import Mapping, Sequence

import numpy as np
import torch as th


def to_numpy(x):
    """tensors (also inside sequences / mappings) to numpy arrays; everything else unchanged (utils.py:20-26)"""
    if isinstance(x, Sequence) and not isinstance(x, (str, bytes)):
        return x.__class__(to_numpy(v) for v in x)
    if isinstance(x, Mapping):
        return x.__class__((k, to_numpy(v)) for k, v in x.items())
    return x.numpy(force=True) if isinstance(x, th.Tensor) else x


def frechet_distance(x: np.ndarray, y: np.ndarray, isotropic=False, eps=1e-6):
    """Frechet distance between the Gaussians fitted to two sets of samples (rows).  ``isotropic``: per-dimension standard deviations
    instead of the covariances:  |mu_x - mu_y|^2 + |std_x - std_y|^2.  Else  |mu_x - mu_y|^2 + tr(S_x) + tr(S_y) - 2 tr((S_x S_y)^1/2);
    a matrix square root that comes out non-finite is retried with ``eps`` on both diagonals, a small imaginary part is dropped and a
    large one (diagonal beyond 1e-3) raises."""
    from scipy import linalg   # (here: only the full form needs scipy, the package imports without it)
    mu_x, mu_y = x.mean(0), y.mean(0)
    if isotropic:
        return np.sum((mu_x - mu_y) ** 2) + np.sum((x.std(0) - y.std(0)) ** 2)
    cov_x, cov_y = np.cov(x, rowvar=False), np.cov(y, rowvar=False)
    covmean, _ = linalg.sqrtm(cov_x @ cov_y, disp=False)
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(cov_x.shape[0]) * eps
        covmean = linalg.sqrtm((cov_x + offset) @ (cov_y + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return np.sum((mu_x - mu_y) ** 2) + np.trace(cov_x) + np.trace(cov_y) - 2 * np.trace(covmean)


def inception_score(prob: np.ndarray):
    """exp(mean_i KL(p(y | x_i) || p(y))) from the (N, K) class probabilities (metric.py:171-173)"""
    marginal = prob.mean(axis=0)
    kl = np.sum(prob * (np.log(prob) - np.log(marginal)), axis=-1)
    return np.exp(kl.mean())


class Metric(ABC):
    """A metric on one channel (``channel=None``: all of them) of predicted and target signals (N, C, T)."""

    def __init__(self, channel=0):
        self.channel = channel

    @property
    def name(self):
        return f"{self.__class__.__name__} - Channel {self.channel}"

    def __call__(self, pred, target):
        pred, target = to_numpy(pred), to_numpy(target)
        if self.channel is not None:
            pred, target = pred[:, self.channel], target[:, self.channel]
        return self.compute(pred, target)

    @abstractmethod
    def compute(self, pred, target):
        pass


class MeanSquaredError(Metric):
    def compute(self, pred, target):
        return ((pred - target) ** 2).mean()


class AmplitudeSpectralDensity(Metric):
    """Frechet distance between the log amplitude spectra of two sets of signals.  numpy arrays and CPU tensors: ``np.fft.rfft`` on the
    host, as in the reference.  Two tensors on a GPU: the log spectra are one launch on the channel view (``spectra``, tqe_rdft in LOG
    mode: no waveform and no spectrum leaves the device); ``isotropic=True`` then takes the float64 column moments and the two sums on
    the device too, ``isotropic=False`` moves the log spectra to the host for the matrix square root, as FID does."""

    def __init__(self, fs, channel=0, log_eps=1e-8, isotropic=True):
        super().__init__(channel)
        self.fs, self.log_eps, self.isotropic = fs, log_eps, isotropic

    def __call__(self, pred, target):
        if isinstance(pred, th.Tensor) and isinstance(target, th.Tensor) and pred.is_cuda and target.is_cuda:
            if self.channel is not None:
                pred, target = pred[:, self.channel], target[:, self.channel]
            return self.compute_device(pred, target)
        return super().__call__(pred, target)

    def spectral_density(self, signal):
        return np.log(np.clip(np.abs(np.fft.rfft(signal, axis=-1)), self.log_eps, None))

    def compute(self, pred, target):
        return frechet_distance(self.spectral_density(pred), self.spectral_density(target), isotropic=self.isotropic)

    def compute_device(self, pred, target):
        from . import spectra
        sp, st = (spectra.log_amplitude_spectrum(x.detach(), self.log_eps) for x in (pred, target))
        if not self.isotropic:
            return frechet_distance(sp.cpu().numpy().astype(np.float64), st.cpu().numpy().astype(np.float64), isotropic=False)
        (mu_p, sd_p), (mu_t, sd_t) = (spectra.column_moments(s.reshape(s.shape[0], -1)) for s in (sp, st))
        d = ((mu_p - mu_t) ** 2).sum() + ((sd_p - sd_t) ** 2).sum()
        # (the host path's result type for this input type, whatever numpy's promotion rules make it)
        host_type = self.spectral_density(np.zeros((1, 2), to_numpy(pred.new_zeros(()).cpu()).dtype)).dtype.type
        return host_type(d.item())


class NeuralMetric(Metric):
    """A metric on the outputs of a trained classifier.  ``representation``: the one the classifier was trained on (its
    ``get_representation`` is applied to the waveforms first).  ``batch_size``: samples per classifier call; None: all at once."""

    def __init__(self, classifier, representation, batch_size=None):
        self.classifier = classifier.eval()
        self.representation = representation
        self.batch_size = batch_size

    @property
    def name(self):
        return self.__class__.__name__

    def _prepare(self, waveform):
        r = self.representation.get_representation(waveform)
        r = th.as_tensor(np.asarray(r) if not isinstance(r, th.Tensor) else r, device=self.classifier.device)
        return r.to(self.classifier.dtype)   # (a float64 representation of numpy's: the classifier computes in its own precision)

    def __call__(self, pred, target=None):
        pred = self._prepare(pred)
        if target is not None:
            target = self._prepare(target)
        return self.compute(pred, target)

    def _batched(self, fn, x):
        """fn over ``x`` in batches of ``batch_size`` (the whole of it when None), results concatenated on the host"""
        n = len(x)
        step = n if self.batch_size is None else int(self.batch_size)
        with th.no_grad():
            return np.concatenate([fn(x[i:i + step]).numpy(force=True) for i in range(0, n, max(step, 1))])


class FrechetInceptionDistance(NeuralMetric):
    """Frechet distance between the classifier embeddings of predicted and target signals."""

    def compute(self, pred, target):
        return frechet_distance(self._batched(self.classifier.embed, pred), self._batched(self.classifier.embed, target))


class InceptionScore(NeuralMetric):
    """Inception score of the classifier's class probabilities on the predicted signals."""

    def compute(self, pred, target=None):
        return inception_score(self._batched(lambda x: th.softmax(self.classifier(x), dim=-1), pred))
