"""LogSpectrogram on the GPU (csrc/spectrogram.hip) against the float64 restatement of librosa's stft / griffinlim
(tests/_logspec_ref.py; librosa itself is not run).  The kernels are called through the C ABI with every output inside NaN-filled
guard bands; the class is exercised by the chain and refusal tests.

Bars.  Forward, complex output: |S_gpu - S_ref| <= delta element-wise, delta = 2 n_fft 2^-24 max_f sum_n |w_n x_(f,n)| per waveform,
the worst case of ANY fp32 evaluation order (about 1.3e-4 of max|S| on the test signal; the complex64 restatement sits at 6.5e-8).
Forward, representation: mapped back to magnitudes in float64, | |S|_gpu - max(|S_ref|, clip) | <= delta + 1e-5 |S_ref| (fp32 log at
|log| <= 18.5: at most 4.4e-6; rounding of the normalised value: 10.7 * 2^-24).  Inverse at 0 / 1 / 2 / 4 iterations: the suite's
standing bar (conftest.rel_err: 1e-3 norm-wise and element-wise) per waveform.  Inverse at 128 iterations: the spectral convergence
of the GPU result may exceed the float64 restatement's by at most 1 %.

Log-input flag: the kernel applies exp((r + 1) / 2 (log_max - log clip) + log clip) with the device's expf and a fused multiply-add;
numpy's float32 exp on the host is another implementation (both within an ulp or two of the true value, not of each other), so the
comparison with host-computed magnitudes is held to the same 1e-3 bar, not to equal bits; the measured difference is printed."""

import functools

import numpy as np
import pytest
import torch

import _logspec_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
G = 4096          # floats of NaN either side of every output
N_FFT, NB = 256, 128
CLIP, LOG_MAX = 1e-8, 3.0


def _dev():
    return torch.device("cuda:0")


def _guarded(n):
    buf = torch.full((n + 2 * G,), float("nan"), device=_dev(), dtype=torch.float32)
    return buf, buf[G:G + n]


def _intact(buf, n):
    return bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all()) and not bool(torch.isnan(buf[G:G + n]).any())


@functools.lru_cache(maxsize=None)
def _rep(hop):
    from tqdne_amd.representation import LogSpectrogram
    return LogSpectrogram(N_FFT, hop)


def gpu_stft(x, hop, spec=True, rep=True):
    """x (N, T) float32 numpy -> (complex64 (N, 128, F) or None, float32 (N, 128, F) or None) through tq_stft_fwd"""
    from tqdne_amd import _lib
    lib = _lib.load()
    N, T = x.shape
    F = 1 + T // hop
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(_dev())
    tables, _ = _rep(hop)._tables(0, _dev())
    sb, s = _guarded(N * NB * F * 2) if spec else (None, None)
    rb, r = _guarded(N * NB * F) if rep else (None, None)
    _lib.check(lib.tq_stft_fwd(xd.data_ptr(), _lib._p(s), _lib._p(r), tables.data_ptr(), N, T, N_FFT, hop, CLIP, LOG_MAX,
                               torch.cuda.current_stream().cuda_stream), "stft_fwd")
    torch.cuda.synchronize()
    out_s = out_r = None
    if spec:
        assert _intact(sb, N * NB * F * 2), "complex output: guard band touched or an element left unwritten"
        out_s = s.cpu().numpy().reshape(N, NB, F, 2).view(np.complex64)[..., 0]
    if rep:
        assert _intact(rb, N * NB * F), "representation: guard band touched or an element left unwritten"
        out_r = r.cpu().numpy().reshape(N, NB, F)
    return out_s, out_r


def gpu_griffinlim(S, hop, n_iter, log_input=False):
    """S (N, 128, F) float32 numpy -> (N, hop (F - 1)) float32 through tq_griffinlim"""
    from tqdne_amd import _lib
    lib = _lib.load()
    N, nb, F = S.shape
    assert nb == NB
    sd = torch.from_numpy(np.ascontiguousarray(S, dtype=np.float32)).to(_dev())
    tables, phase = _rep(hop)._tables(F, _dev())
    n = N * hop * (F - 1)
    ob, o = _guarded(n)
    _lib.check(lib.tq_griffinlim(sd.data_ptr(), o.data_ptr(), tables.data_ptr(), phase.data_ptr(), N, F, N_FFT, hop, n_iter, 0.99,
                                 int(log_input), CLIP, LOG_MAX, torch.cuda.current_stream().cuda_stream), "griffinlim")
    torch.cuda.synchronize()
    assert _intact(ob, n), "waveform output: guard band touched or an element left unwritten"
    return o.cpu().numpy().reshape(N, hop * (F - 1))


@functools.lru_cache(maxsize=None)
def _signal(T, N):
    return R.make_signal(T, N).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _forward_ref(T, N, hop):
    """(S_ref float64-complex (N, 128, F), delta (N, 1, 1)) of the fp32 test signal"""
    x = _signal(T, N).astype(np.float64)
    S = R.get_spectrogram(x, N_FFT, hop)
    l1 = np.abs(R.frames_of(x, N_FFT, hop) * R.hann(N_FFT)).sum(-1).max(-1)
    return S, (2.0 * N_FFT * 2.0 ** -24 * l1)[:, None, None]


FORWARD = [(32, 256, 1), (32, 256, 300), (32, 1000, 6), (32, 4064, 1), (32, 4064, 6), (64, 4032, 6)]


@pytest.mark.parametrize("hop,T,N", FORWARD)
def test_forward_complex_and_representation(hop, T, N):
    x = _signal(T, N)
    S_ref, delta = _forward_ref(T, N, hop)
    S, r = gpu_stft(x, hop)
    assert S.shape == S_ref.shape == (N, NB, 1 + T // hop)
    d = np.abs(S.astype(np.complex128) - S_ref)
    smax = np.abs(S_ref).max(axis=(1, 2), keepdims=True)
    print(f"forward hop {hop} T {T} N {N}: max |S_gpu - S_ref| / max|S| = {(d / smax).max():.2e}, max / delta = {(d / delta).max():.2e}, "
          f"delta / max|S| = {(delta / smax).max():.2e}")
    assert (d <= delta).all()
    lc = np.log(CLIP)
    mag = np.exp((r.astype(np.float64) + 1.0) / 2.0 * (LOG_MAX - lc) + lc)
    dm = np.abs(mag - np.maximum(np.abs(S_ref), CLIP))
    bar = delta + 1e-5 * np.abs(S_ref)
    print(f"  representation: max excess over |S_ref| in units of the bar = {(dm / bar).max():.2e}")
    assert (dm <= bar).all()
    # either output alone: the same bits
    S1, _ = gpu_stft(x, hop, rep=False)
    _, r1 = gpu_stft(x, hop, spec=False)
    assert np.array_equal(S1.view(np.float32), S.view(np.float32)) and np.array_equal(r1, r)


def test_forward_leading_dimensions_and_kinds():
    rep = _rep(32)
    x = _signal(1000, 6)
    S, r = gpu_stft(x, 32)
    xd = torch.from_numpy(x).to(_dev()).reshape(2, 3, 1000)
    Sd, rd = rep.get_spectrogram(xd), rep.get_representation(xd)
    assert Sd.is_cuda and Sd.dtype == torch.complex64 and Sd.shape == (2, 3, NB, 32) and rd.is_cuda and rd.shape == (2, 3, NB, 32)
    assert np.array_equal(Sd.cpu().numpy().reshape(6, NB, 32), S) and np.array_equal(rd.cpu().numpy().reshape(6, NB, 32), r)
    Sn = rep.get_spectrogram(x.reshape(2, 3, 1000))
    assert isinstance(Sn, np.ndarray) and Sn.dtype == np.complex64 and np.array_equal(Sn.reshape(6, NB, 32), S)
    rt = rep.get_representation(torch.from_numpy(x))
    assert isinstance(rt, torch.Tensor) and not rt.is_cuda and np.array_equal(rt.numpy(), r)


INVERSE = [(32, 9), (32, 32), (32, 128), (64, 64)]


@functools.lru_cache(maxsize=None)
def _magnitudes(hop, F, N=3):
    """fp32 magnitudes (N, 128, F) of the test signal of length hop (F - 1)"""
    x = _signal(hop * (F - 1), N).astype(np.float64)
    return np.abs(R.get_spectrogram(x, N_FFT, hop)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inverse_ref(hop, F, n_iter, log_input=False):
    M = _magnitudes(hop, F)
    if log_input:
        M = R.from_representation(R.to_representation(M.astype(np.float64), CLIP, LOG_MAX).astype(np.float32), CLIP, LOG_MAX)
    return R.griffinlim(R.with_nyquist(M.astype(np.float64)), n_iter, hop, N_FFT)


@pytest.mark.parametrize("n_iter", [0, 1, 2, 4])
@pytest.mark.parametrize("hop,F", INVERSE)
def test_inverse_few_iterations(hop, F, n_iter):
    M = _magnitudes(hop, F)
    y = gpu_griffinlim(M, hop, n_iter)
    ref = _inverse_ref(hop, F, n_iter)
    assert y.shape == ref.shape == (3, hop * (F - 1))
    errs = [rel_err(y[i], ref[i]) for i in range(3)]
    print(f"inverse hop {hop} F {F} n_iter {n_iter}: norm-wise errors per waveform {['%.1e' % e for e in errs]}")
    assert max(errs) < 1e-3


@pytest.mark.parametrize("hop,F", INVERSE)
def test_inverse_of_the_log_representation(hop, F):
    M = _magnitudes(hop, F)
    lc = np.log(CLIP)
    r32 = R.to_representation(M.astype(np.float64), CLIP, LOG_MAX).astype(np.float32)
    y = gpu_griffinlim(r32, hop, 4, log_input=True)
    ref = _inverse_ref(hop, F, 4, log_input=True)
    errs = [rel_err(y[i], ref[i]) for i in range(3)]
    # the same fp32 formula on the host (numpy's expf, no fused multiply-add), fed as magnitudes
    m32 = np.exp((r32 + np.float32(1.0)) * np.float32(0.5) * np.float32(LOG_MAX - lc) + np.float32(lc)).astype(np.float32)
    y2 = gpu_griffinlim(m32, hop, 4)
    errs2 = [rel_err(y[i], y2[i]) for i in range(3)]
    print(f"log input hop {hop} F {F}: vs float64 {max(errs):.1e}; vs host-exp magnitudes {max(errs2):.1e}, equal bits: {np.array_equal(y, y2)}")
    assert max(errs) < 1e-3 and max(errs2) < 1e-3


def _convergence(y, M, hop):
    S = np.abs(R.get_spectrogram(np.asarray(y, dtype=np.float64), N_FFT, hop))
    M = M.astype(np.float64)
    return np.linalg.norm((S - M).reshape(len(M), -1), axis=1) / np.linalg.norm(M.reshape(len(M), -1), axis=1)


def test_inverse_128_iterations_converges_like_float64():
    """Measured on an MI355X: see the figures printed here and quoted in DESIGN.md section 'LogSpectrogram'."""
    hop, F = 32, 128
    M = _magnitudes(hop, F)
    y = gpu_griffinlim(M, hop, 128)
    ref = _inverse_ref(hop, F, 128)
    c_gpu, c_ref, c_0 = _convergence(y, M, hop), _convergence(ref, M, hop), _convergence(_inverse_ref(hop, F, 0), M, hop)
    dist = [float(np.abs(y[i] - ref[i]).max() / np.abs(ref[i]).max()) for i in range(3)]
    print(f"128 iterations: spectral convergence GPU {c_gpu}, float64 {c_ref} (0 iterations: {c_0}); distance to float64 {dist}")
    assert (c_ref < 0.2 * c_0).all()                 # the reference itself converged
    assert (c_gpu <= 1.01 * c_ref).all()


def test_waveforms_are_independent_and_runs_repeat():
    hop, F = 32, 9
    x = _signal(256, 300).astype(np.float64)
    M = np.abs(R.get_spectrogram(x, N_FFT, hop)).astype(np.float32)
    y = gpu_griffinlim(M, hop, 4)
    alone = gpu_griffinlim(M[:1], hop, 4)
    assert np.array_equal(y[:1], alone)
    assert np.array_equal(gpu_griffinlim(M, hop, 4), y)
    ref = R.griffinlim(R.with_nyquist(M[[0, 299]].astype(np.float64)), 4, hop, N_FFT)
    assert max(rel_err(y[0], ref[0]), rel_err(y[299], ref[1])) < 1e-3
    S, _ = gpu_stft(x[:1].astype(np.float32), hop, rep=False)
    S_all, _ = gpu_stft(x.astype(np.float32), hop, rep=False)
    assert np.array_equal(S.view(np.float32), S_all[:1].view(np.float32))


def test_chain_from_the_envelope_representation():
    from oracle import representation as O
    from tqdne_amd.representation import LogSpectrogram, MovingAverageEnvelope
    g = torch.Generator().manual_seed(5)
    z = torch.cat([torch.randn(4, 3, 4064, generator=g), 0.5 * torch.randn(4, 3, 4064, generator=g) + 2.0], dim=1)
    zd = z.to(_dev())
    rep = LogSpectrogram(256, 32)
    wave = MovingAverageEnvelope().invert_representation(zd)
    out = rep.get_representation(wave)
    assert out.is_cuda and out.shape == (4, 3, 128, 128) and out.dtype == torch.float32
    wref = O.invert_representation(z.numpy().astype(np.float64)).reshape(12, 4064)
    S_ref = R.get_spectrogram(wref, N_FFT, 32)
    delta = (2.0 * N_FFT * 2.0 ** -24 * np.abs(R.frames_of(wref, N_FFT, 32) * R.hann(N_FFT)).sum(-1).max(-1))[:, None, None]
    lc = np.log(CLIP)
    mag = np.exp((out.cpu().numpy().reshape(12, 128, 128).astype(np.float64) + 1.0) / 2.0 * (LOG_MAX - lc) + lc)
    dm = np.abs(mag - np.maximum(np.abs(S_ref), CLIP))
    bar = delta + 1e-5 * np.abs(S_ref)
    print(f"chain: max error in units of the forward bar {(dm / bar).max():.2e}")
    assert (dm <= bar).all()
    back = rep.invert_representation(out)
    assert back.is_cuda and back.shape == (4, 3, 4064) and bool(torch.isfinite(back).all())


def test_refusals_name_the_limit():
    rep = _rep(32)
    with pytest.raises((ValueError, NotImplementedError), match=str(rep.max_frames)):
        rep.invert_spectrogram(torch.zeros(1, NB, rep.max_frames + 1, device=_dev()))
    with pytest.raises((ValueError, NotImplementedError), match="128"):
        rep.invert_representation(torch.zeros(1, NB + 1, 64, device=_dev()))
    with pytest.raises((ValueError, NotImplementedError), match="256"):
        rep.get_representation(torch.zeros(2, 255, device=_dev()))
    with pytest.raises((ValueError, NotImplementedError), match="256"):
        rep.invert_spectrogram(torch.zeros(1, NB, 8, device=_dev()))
