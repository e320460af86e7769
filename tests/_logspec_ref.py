"""TEST INFRASTRUCTURE -- numpy-only restatement of the reference's ``LogSpectrogram`` (tqdne/representation.py:63-175), i.e. of
librosa 0.11.0 ``stft`` / ``istft`` / ``griffinlim`` at the defaults the reference uses (win_length = n_fft, periodic Hann,
center=True, pad_mode="constant", momentum=0.99, init="random", random_state=0) and of the two log-magnitude maps.

librosa itself is NOT run anywhere in this project: the algorithm below is restated from its source and pinned only against
scipy.signal (tests/test_logspec_host.py).  ``dtype=np.float64`` (default) is the reference the GPU is held to;
``dtype=np.float32`` is the complex64 variant: the same steps with every intermediate rounded to fp32 / complex64, which shows
what fp32 arithmetic alone costs.
"""

import numpy as np


def _c(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def hann(n_fft, dtype=np.float64):
    """scipy.signal.get_window("hann", n_fft, fftbins=True): the periodic Hann window (computed in float64, then cast)."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(dtype)


def n_frames(T, hop):
    return 1 + T // hop


def frames_of(y, n_fft, hop):
    """(..., T) -> (..., F, n_fft): the frames of the centred, zero-padded signal (no window)."""
    y = np.asarray(y)
    T = y.shape[-1]
    pad = np.zeros(y.shape[:-1] + (T + n_fft,), dtype=y.dtype)
    pad[..., n_fft // 2:n_fft // 2 + T] = y
    idx = np.arange(n_frames(T, hop))[:, None] * hop + np.arange(n_fft)[None, :]
    return pad[..., idx]


def stft(y, n_fft=256, hop=None, dtype=np.float64):
    """librosa.stft(y, n_fft, hop_length): (..., T) -> (..., n_fft / 2 + 1, 1 + T // hop) complex."""
    hop = n_fft // 4 if hop is None else hop
    y = np.asarray(y, dtype=dtype)
    fr = (frames_of(y, n_fft, hop) * hann(n_fft, dtype)).astype(dtype)
    return np.swapaxes(np.fft.rfft(fr, axis=-1), -1, -2).astype(_c(dtype))


def window_sumsquare(n_fft, hop, F, dtype=np.float64):
    w2 = hann(n_fft, np.float64) ** 2
    wss = np.zeros(n_fft + hop * (F - 1))
    for f in range(F):
        wss[f * hop:f * hop + n_fft] += w2
    return wss.astype(dtype)


def istft(S, n_fft=256, hop=None, dtype=np.float64):
    """librosa.istft(S, hop_length, n_fft): (..., n_fft / 2 + 1, F) -> (..., hop * (F - 1)).  irfft per frame (which ignores the
    imaginary parts of DC and Nyquist), times the window, overlap-added, divided by the window sum-square wherever that exceeds
    ``tiny``, n_fft / 2 trimmed from each end."""
    hop = n_fft // 4 if hop is None else hop
    S = np.asarray(S).astype(_c(dtype))
    F = S.shape[-1]
    fr = (np.fft.irfft(np.swapaxes(S, -1, -2), n=n_fft, axis=-1).astype(dtype) * hann(n_fft, dtype)).astype(dtype)
    y = np.zeros(S.shape[:-2] + (n_fft + hop * (F - 1),), dtype=dtype)
    for f in range(F):
        y[..., f * hop:f * hop + n_fft] += fr[..., f, :]
    wss = window_sumsquare(n_fft, hop, F, dtype)
    nz = wss > np.finfo(dtype).tiny
    y[..., nz] /= wss[nz]
    return y[..., n_fft // 2:y.shape[-1] - n_fft // 2]


def phase_field(n_fft, F):
    """exp(2 pi i U), U = RandomState(0).random((n_fft / 2 + 1, F)): the reference seeds every waveform with 0, so this one field
    starts them all (complex128)."""
    u = np.random.RandomState(0).random((n_fft // 2 + 1, F))
    return np.cos(2.0 * np.pi * u) + 1j * np.sin(2.0 * np.pi * u)


def griffinlim(S, n_iter=128, hop=None, n_fft=256, momentum=0.99, dtype=np.float64):
    """librosa.griffinlim(S, n_iter, hop_length, n_fft=n_fft, momentum=0.99, init="random", random_state=0) for magnitudes
    S (..., n_fft / 2 + 1, F)."""
    hop = n_fft // 4 if hop is None else hop
    S = np.asarray(S, dtype=dtype)
    cd = _c(dtype)
    tiny = np.finfo(dtype).tiny
    A = (phase_field(n_fft, S.shape[-1]).astype(cd) * S).astype(cd)
    alpha = momentum / (1 + momentum)
    prev = None
    for _ in range(n_iter):
        y = istft(A, n_fft, hop, dtype)
        R = stft(y, n_fft, hop, dtype)
        C = R if prev is None else (R - alpha * prev).astype(cd)
        A = ((C / (np.abs(C) + tiny).astype(dtype)).astype(cd) * S).astype(cd)
        prev = R
    return istft(A, n_fft, hop, dtype)


def with_nyquist(S):
    """(..., n_fft / 2, F) -> (..., n_fft / 2 + 1, F) with a zero Nyquist row (LogSpectrogram.invert_spectrogram)."""
    return np.concatenate([S, np.zeros_like(S[..., :1, :])], axis=-2)


def get_spectrogram(x, n_fft=256, hop=None, dtype=np.float64):
    """LogSpectrogram.get_spectrogram: the STFT without its Nyquist row."""
    return stft(x, n_fft, hop, dtype)[..., :-1, :]


def to_representation(S, clip=1e-8, log_max=3.0):
    """LogSpectrogram.get_representation after the STFT: complex or magnitude -> normalised log-magnitude (float64)."""
    lc = np.log(clip)
    return 2.0 * (np.log(np.clip(np.abs(S), clip, None)) - lc) / (log_max - lc) - 1.0


def from_representation(r, clip=1e-8, log_max=3.0):
    """LogSpectrogram.invert_representation before Griffin-Lim: normalised log-magnitude -> magnitude (float64)."""
    lc = np.log(clip)
    return np.exp((np.asarray(r, dtype=np.float64) + 1.0) / 2.0 * (log_max - lc) + lc)


def make_signal(T, n_waves=1):
    """The suite's test signal: a burst on a noise floor (which keeps the spectrum free of deep nulls), one waveform per power of ten
    from 1e-3 to 1e2 (cycled)."""
    rng = np.random.default_rng(1)
    n = np.arange(T)
    out = np.empty((n_waves, T))
    for i in range(n_waves):
        x = rng.standard_normal(T) * np.exp(-((n - 0.3 * T) / (0.15 * T)) ** 2) * np.sin(0.002 * n) ** 2 + 1e-3 * rng.standard_normal(T)
        out[i] = x * 10.0 ** (-3 + i % 6)
    return out
