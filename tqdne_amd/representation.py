"""Signal representations either side of the diffusion path (mirror of tqdne/representation.py).

``MovingAverageEnvelope`` is the representation of the reference's 1-D experiments (experiments/config.py:62-67): it turns a
3-channel waveform into the 6-channel signal the EDM is trained on and back.  The reference computes it with
``np.apply_along_axis(np.convolve)`` on the host (a loader bottleneck and a post-sampling step); here both directions are one
HBM-bound HIP launch (tq_envelope_fwd / tq_envelope_inv) on tensors that already live on the GPU.

Interface: same class and method names and arguments.  Inputs may be torch tensors on a GPU (returned as GPU tensors) or numpy
arrays / CPU tensors (uploaded, computed on the GPU, returned as numpy like the reference's NumpyArgMixin does).  Results are
fp32 (computed in float64 inside the kernel, as numpy does; the reference returns float64 arrays that its Dataset casts to
fp32).  There is no host fallback: without a GPU and the HIP library the calls raise.

``LogSpectrogram`` is the representation of the reference's spectrogram family and of its 1-D evaluation (experiments/evaluate.py
pushes every sampled batch through it before the classifier).  The reference computes it with librosa on the host in a process
pool -- the STFT per waveform, the inversion by 128 Griffin-Lim iterations per waveform; here ``get_representation`` is one launch
(tq_stft_fwd, log-magnitude written directly) and ``invert_representation`` is one launch (tq_griffinlim: one workgroup per
waveform keeps the whole iteration on chip).  librosa's semantics are restated (csrc/spectrogram.hip), not run.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check


def _to_gpu(x):
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.contiguous().float(), "cuda"
    if not torch.cuda.is_available():
        raise RuntimeError("tqdne_amd.representation runs on the GPU (no CPU fallback): no GPU is visible")
    kind = "torch" if isinstance(x, torch.Tensor) else "numpy"
    t = torch.as_tensor(np.asarray(x) if kind == "numpy" else x, dtype=torch.float32)
    return t.contiguous().to("cuda"), kind


def _back(y, kind):
    if kind == "cuda":
        return y
    return y.cpu() if kind == "torch" else y.cpu().numpy()


class Representation:
    def get_representation(self, waveform):
        raise NotImplementedError

    def invert_representation(self, representation):
        raise NotImplementedError


class Identity(Representation):  # representation.py:21-26
    def get_representation(self, waveform):
        return waveform

    def invert_representation(self, representation):
        return representation


class Normalization(Representation):  # representation.py:29-38
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def get_representation(self, waveform):
        return (waveform - self.mean) / self.std

    def invert_representation(self, representation):
        return representation * self.std + self.mean


class MovingAverageEnvelope(Representation):  # representation.py:41-60
    def __init__(self, window_size=128, log_eps=1e-6, eps=1e-6):
        self.window_size, self.log_eps, self.eps = window_size, log_eps, eps

    def get_representation(self, waveform):
        x, kind = _to_gpu(waveform)
        if x.dim() < 2:
            raise ValueError("expected (..., channels, time)")
        C_, T = x.shape[-2], x.shape[-1]
        if T < self.window_size:
            raise ValueError(f"signal length {T} < window {self.window_size} (np.convolve(mode='same') would change the length)")
        N = x.numel() // (C_ * T)
        out = torch.empty(x.shape[:-2] + (2 * C_, T), device=x.device, dtype=torch.float32)
        lib = _lib.load()
        check(lib.tq_envelope_fwd(x.data_ptr(), out.data_ptr(), N, C_, T, self.window_size, float(self.log_eps), float(self.eps),
                                  torch.cuda.current_stream(x.device).cuda_stream), "envelope_fwd")
        return _back(out, kind)

    def invert_representation(self, representation):
        r, kind = _to_gpu(representation)
        C2, T = r.shape[-2], r.shape[-1]
        if C2 % 2:
            raise ValueError("representation must have an even number of channels (scaled waveform | log envelope)")
        C_ = C2 // 2
        N = r.numel() // (C2 * T)
        out = torch.empty(r.shape[:-2] + (C_, T), device=r.device, dtype=torch.float32)
        lib = _lib.load()
        check(lib.tq_envelope_inv(r.data_ptr(), out.data_ptr(), N, C_, T, float(self.log_eps), float(self.eps),
                                  torch.cuda.current_stream(r.device).cuda_stream), "envelope_inv")
        return _back(out, kind)


class LogSpectrogram(Representation):  # representation.py:63-175
    """Log-magnitude STFT and its Griffin-Lim inversion on the GPU: same constructor, methods and shapes as the reference's class with
    ``library="librosa"``.  (..., T) -> (..., stft_channels / 2, 1 + T // hop_size) and back to (..., hop_size * (frames - 1)).

    ``multiprocessing`` is accepted and ignored (there is no process pool).  ``library="tifresi"`` / ``"torchaudio"`` are refused
    (the reference's torchaudio branch cannot run either: it calls an undefined ``griffinlim``).  The inversion holds a waveform's
    state on one compute unit, which limits the frames per waveform to ``max_frames``.  The first call for a new frame count uploads
    the window / twiddle / window-sum-square table and the initial phases (numpy's RandomState(0), as librosa draws them); later
    calls on GPU tensors enqueue one launch on the current stream and do not synchronise."""

    n_iter, momentum = 128, 0.99   # LogSpectrogram's griffinlim(n_iter=128) and librosa's default momentum

    def __init__(self, stft_channels=256, hop_size=None, clip=1e-8, log_max=3, library="librosa", multiprocessing=True):
        if library != "librosa":
            raise NotImplementedError(f"LogSpectrogram(library={library!r}): only the librosa semantics are built on the HIP path")
        self.clip, self.log_clip, self.log_max, self.library = clip, np.log(clip), log_max, library
        self.stft_channels = int(stft_channels)
        self.hop_size = self.stft_channels // 4 if hop_size is None else int(hop_size)
        if not (clip > 0 and log_max > self.log_clip):
            raise ValueError(f"LogSpectrogram: clip = {clip} must be positive and log_max = {log_max} above log(clip)")
        rc = _lib.load().tq_griffinlim_max_frames(self.stft_channels, self.hop_size)
        if rc == -1:
            raise ValueError(f"LogSpectrogram: hop_size = {self.hop_size} must be positive and divide stft_channels = {self.stft_channels}")
        if rc < 0:
            raise NotImplementedError(f"LogSpectrogram(stft_channels={self.stft_channels}, hop_size={self.hop_size}): the HIP kernels "
                                      "are built for stft_channels = 256 with hop_size 32 or 64")
        self.max_frames = rc
        self._cache = {}   # (frames, device) -> (tables, phases) on that device

    def disable_multiprocessing(self):
        pass

    def _tables(self, F, device):
        key = (F, str(device))
        if key not in self._cache:
            lib = _lib.load()
            n_fft, hop = self.stft_channels, self.hop_size
            buf = np.empty(lib.tq_spectrogram_table_floats(n_fft, hop, F), np.float32)
            check(lib.tq_spectrogram_tables(n_fft, hop, F, buf.ctypes.data), "spectrogram_tables")
            ang = 2.0 * np.pi * np.random.RandomState(0).random((n_fft // 2 + 1, F))[:-1]   # drawn WITH the Nyquist row, as librosa does
            phase = np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)
            self._cache[key] = (torch.from_numpy(buf).to(device), torch.from_numpy(phase).to(device))
        return self._cache[key]

    def _forward(self, waveform, want_repr):
        x, kind = _to_gpu(waveform)
        n_fft, hop = self.stft_channels, self.hop_size
        T = x.shape[-1] if x.dim() else 0
        if T < n_fft:
            raise ValueError(f"LogSpectrogram: signal length {T} < stft_channels = {n_fft}")
        N, F = x.numel() // T, 1 + T // hop
        shape = tuple(x.shape[:-1]) + (n_fft // 2, F)
        out = torch.empty(shape if want_repr else shape + (2,), device=x.device, dtype=torch.float32)
        if N:
            tables, _ = self._tables(0, x.device)   # window and twiddles only: the forward needs no window sum-square
            check(_lib.load().tq_stft_fwd(x.data_ptr(), None if want_repr else out.data_ptr(), out.data_ptr() if want_repr else None,
                                          tables.data_ptr(), N, T, n_fft, hop, float(self.clip), float(self.log_max),
                                          torch.cuda.current_stream(x.device).cuda_stream), "stft_fwd")
        return _back(out if want_repr else torch.view_as_complex(out), kind)

    def _inverse(self, spec, log_input):
        if isinstance(spec, torch.Tensor) and spec.is_complex():
            spec = spec.abs()
        elif not isinstance(spec, torch.Tensor) and np.iscomplexobj(spec):
            spec = np.abs(spec)
        s, kind = _to_gpu(spec)
        n_fft, hop = self.stft_channels, self.hop_size
        if s.dim() < 2 or s.shape[-2] != n_fft // 2:
            raise ValueError(f"LogSpectrogram: expected (..., {n_fft // 2}, frames) -- stft_channels / 2 = {n_fft // 2} frequency rows "
                             f"(no Nyquist row) -- got {tuple(s.shape)}")
        F = s.shape[-1]
        if F > self.max_frames:
            raise NotImplementedError(f"LogSpectrogram: {F} frames per waveform; the one-launch Griffin-Lim keeps a waveform on one "
                                      f"compute unit and is built for at most {self.max_frames} frames at hop_size = {hop}")
        if hop * (F - 1) < n_fft:
            raise ValueError(f"LogSpectrogram: {F} frames give a signal of {hop * (F - 1)} < stft_channels = {n_fft} samples")
        N = s.numel() // (s.shape[-2] * F)
        out = torch.empty(tuple(s.shape[:-2]) + (hop * (F - 1),), device=s.device, dtype=torch.float32)
        if N:
            tables, phase = self._tables(F, s.device)
            check(_lib.load().tq_griffinlim(s.data_ptr(), out.data_ptr(), tables.data_ptr(), phase.data_ptr(), N, F, n_fft, hop,
                                            self.n_iter, self.momentum, int(log_input), float(self.clip), float(self.log_max),
                                            torch.cuda.current_stream(s.device).cuda_stream), "griffinlim")
        return _back(out, kind)

    def get_spectrogram(self, waveform):
        """(..., T) -> complex64 (..., stft_channels / 2, frames): librosa.stft without its Nyquist row."""
        return self._forward(waveform, want_repr=False)

    def invert_spectrogram(self, spec):
        """magnitudes (..., stft_channels / 2, frames) -> (..., hop_size * (frames - 1)) by 128 Griffin-Lim iterations (a complex
        input contributes its modulus, as librosa.griffinlim takes it)."""
        return self._inverse(spec, log_input=False)

    def get_representation(self, waveform):
        return self._forward(waveform, want_repr=True)

    def invert_representation(self, representation):
        return self._inverse(representation, log_input=True)
