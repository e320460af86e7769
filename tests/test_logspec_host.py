"""LogSpectrogram without a GPU: the float64 restatement of librosa's stft / istft (tests/_logspec_ref.py) against scipy.signal, the
C-ABI argument checks and limit query of csrc/spectrogram.hip, the class surface, and that the entry points are declared, bound and exported.
librosa itself is not installed anywhere this suite runs: its semantics are restated, and scipy is the independent witness."""

import os
import re

import numpy as np
import pytest

import _logspec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tq_stft_fwd", "tq_griffinlim", "tq_griffinlim_max_frames", "tq_spectrogram_tables", "tq_spectrogram_table_floats"]


def _nrm(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_restatement_matches_scipy_stft_and_round_trips():
    ss = pytest.importorskip("scipy.signal")
    x = R.make_signal(4064, 3)
    win = ss.get_window("hann", 256)
    assert np.abs(win - R.hann(256)).max() < 1e-15   # the same window up to the rounding of two formulas
    kw = dict(window="hann", nperseg=256, noverlap=224, padded=False, scaling="spectrum")
    _, _, Z = ss.stft(x, boundary="zeros", **kw)
    S = R.stft(x, 256, 32)
    assert S.shape == Z.shape == (3, 129, 128)
    e_fwd = _nrm(S, Z * win.sum())
    y = R.istft(S, 256, 32)
    e_rt = _nrm(y, x)
    _, xs = ss.istft(Z, boundary=True, **{k: v for k, v in kw.items() if k != "padded"})
    e_inv = _nrm(y, xs[..., :4064])
    print(f"stft vs scipy {e_fwd:.1e}, istft(stft(x)) vs x {e_rt:.1e}, istft vs scipy {e_inv:.1e}")
    assert e_fwd < 1e-12 and e_rt < 1e-12 and e_inv < 1e-12
    # hop 64 and a ragged length (the tail past the last full hop only reaches the padding)
    _, _, Z = ss.stft(x[:, :1000], window="hann", nperseg=256, noverlap=192, boundary="zeros", padded=False, scaling="spectrum")
    assert _nrm(R.stft(x[:, :1000], 256, 64)[..., :Z.shape[-1]], Z * win.sum()) < 1e-12
    S = R.stft(x[:, :1000], 256, 32)
    assert S.shape[-1] == 32 and _nrm(R.istft(S, 256, 32), x[:, :992]) < 1e-12


def test_restatement_griffinlim_is_a_fixed_point_iteration_that_converges():
    """the figures the GPU test's 1 % bar stands on: spectral convergence falls monotonically over the first iterations, and the
    complex64 variant follows the float64 one"""
    x = R.make_signal(4064, 1)
    M = np.abs(R.stft(x, 256, 32))
    M[:, -1] = 0.0
    sc = []
    for it in (0, 1, 4):
        y = R.griffinlim(M, it, 32, 256)
        assert y.shape == (1, 4064)
        sc.append(float(np.linalg.norm(np.abs(R.stft(y, 256, 32)) - M) / np.linalg.norm(M)))
    assert sc[0] > sc[1] > sc[2] and 0.6 < sc[0] < 0.85
    y32 = R.griffinlim(M, 4, 32, 256, dtype=np.float32)
    assert y32.dtype == np.float32 and _nrm(y32, y) < 1e-5
    r = R.to_representation(M[:, :-1])
    assert r.min() >= -1.0 and _nrm(R.from_representation(r), np.clip(M[:, :-1], 1e-8, None)) < 1e-12


def test_c_abi_argument_checks_return_error_codes_without_a_gpu():
    from tqdne_amd import _lib
    lib = _lib.load()
    fake = 0x1000   # never dereferenced: every call below is rejected during validation
    stft = lambda x=fake, spec=fake, rep=fake, tab=fake, N=2, T=4064, n_fft=256, hop=32, clip=1e-8, log_max=3.0: \
        lib.tq_stft_fwd(x, spec, rep, tab, N, T, n_fft, hop, clip, log_max, None)
    assert stft(x=None) == -1 and stft(tab=None) == -1
    assert stft(spec=None, rep=None) == -1            # at least one output
    assert stft(T=255) == -2                          # T < n_fft
    assert stft(hop=48) == -1                         # hop does not divide n_fft
    assert stft(hop=0) == -1 and stft(n_fft=0) == -1
    assert stft(n_fft=512, hop=128) == -2 and stft(n_fft=128, hop=32) == -2 and stft(hop=16) == -2   # no kernel
    assert stft(N=0) == -2
    assert stft(clip=0.0) == -1 and stft(log_max=-20.0) == -1
    gl = lambda i=fake, o=fake, tab=fake, ph=fake, N=2, F=128, n_fft=256, hop=32, n_iter=128, mom=0.99, flag=0, clip=1e-8, log_max=3.0: \
        lib.tq_griffinlim(i, o, tab, ph, N, F, n_fft, hop, n_iter, mom, flag, clip, log_max, None)
    assert gl(i=None) == -1 and gl(o=None) == -1 and gl(tab=None) == -1 and gl(ph=None) == -1
    assert gl(n_iter=-1) == -1
    assert gl(hop=48) == -1
    assert gl(F=8) == -2                              # hop (F - 1) < n_fft
    assert gl(F=lib.tq_griffinlim_max_frames(256, 32) + 1) == -2
    assert gl(n_fft=512, hop=128) == -2 and gl(N=0) == -2
    assert gl(flag=1, clip=-1.0) == -1
    assert lib.tq_spectrogram_tables(256, 32, 128, None) == -1
    assert lib.tq_spectrogram_table_floats(256, 48, 128) == 0 and lib.tq_spectrogram_table_floats(512, 128, 16) == 0


def test_frame_limit_query():
    from tqdne_amd import _lib
    lib = _lib.load()
    assert lib.tq_griffinlim_max_frames(256, 32) >= 128
    assert lib.tq_griffinlim_max_frames(256, 64) >= 64
    assert lib.tq_griffinlim_max_frames(256, 48) == -1 and lib.tq_griffinlim_max_frames(0, 32) == -1
    assert lib.tq_griffinlim_max_frames(256, 0) == -1 and lib.tq_griffinlim_max_frames(256, -32) == -1
    assert lib.tq_griffinlim_max_frames(512, 128) == -2 and lib.tq_griffinlim_max_frames(256, 8) == -2


def test_host_tables_are_the_float64_values():
    from tqdne_amd import _lib
    lib = _lib.load()
    for hop, F in ((32, 9), (32, 128), (64, 64)):
        n = lib.tq_spectrogram_table_floats(256, hop, F)
        assert n == 3 * 256 + hop * (F - 1) + 256
        buf = np.full(n + 8, np.nan, np.float32)
        assert lib.tq_spectrogram_tables(256, hop, F, buf.ctypes.data) == 0
        assert np.isnan(buf[n:]).all()
        m = np.arange(256)
        assert np.array_equal(buf[:256], R.hann(256, np.float32))
        assert np.abs(buf[256:512] - np.cos(2 * np.pi * m / 256)).max() <= 2.0 ** -24
        assert np.abs(buf[512:768] - np.sin(2 * np.pi * m / 256)).max() <= 2.0 ** -24
        wss = R.window_sumsquare(256, hop, F)
        assert np.abs(buf[768:n] - wss).max() <= 2.0 ** -23 * wss.max()
    assert lib.tq_spectrogram_table_floats(256, 32, 0) == 768


def test_class_surface():
    import inspect
    import torch
    from tqdne_amd.representation import LogSpectrogram, Representation
    sig = inspect.signature(LogSpectrogram.__init__)
    assert [(k, p.default) for k, p in sig.parameters.items() if k != "self"] == [
        ("stft_channels", 256), ("hop_size", None), ("clip", 1e-8), ("log_max", 3), ("library", "librosa"), ("multiprocessing", True)]
    rep = LogSpectrogram()
    assert isinstance(rep, Representation)
    assert (rep.stft_channels, rep.hop_size, rep.clip, rep.log_max, rep.library) == (256, 64, 1e-8, 3, "librosa")
    assert rep.log_clip == np.log(1e-8) and rep.max_frames >= 64
    assert LogSpectrogram(256, 32, multiprocessing=False).hop_size == 32
    assert rep.disable_multiprocessing() is None
    for name in ("get_spectrogram", "invert_spectrogram", "get_representation", "invert_representation"):
        assert callable(getattr(rep, name))
    for lib in ("tifresi", "torchaudio"):
        with pytest.raises(NotImplementedError):
            LogSpectrogram(library=lib)
    with pytest.raises(NotImplementedError, match="256"):
        LogSpectrogram(stft_channels=512)
    with pytest.raises(ValueError):
        LogSpectrogram(256, 48)
    if not torch.cuda.is_available():   # there is no host fallback
        with pytest.raises(RuntimeError, match="GPU"):
            rep.get_representation(np.zeros((3, 4064), np.float32))
        with pytest.raises(RuntimeError, match="GPU"):
            rep.invert_representation(torch.zeros(3, 128, 64))


def test_entry_points_are_declared_exported_and_bound():
    from tqdne_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tqdne_hip.h")).read()
    assert lib.tq_abi_version() == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        decl = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, header, re.S | re.M)
        assert decl, f"{name} is not declared in include/tqdne_hip.h"
        assert name in _lib._PROTOS and hasattr(lib, name)
    from tqdne_amd import _build
    assert "spectrogram.hip" in _build.SOURCES
