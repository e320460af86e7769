"""The evaluation library's kernels on the GPU (csrc_eval/spectra.hip through the C ABI and through tqdne_amd/spectra.py, metric.py,
ground_motion.py) against numpy float64 and the restatement tests/_spectra_ref.py.

Inputs are channel views of a tensor that is NaN elsewhere (row stride 3 N); outputs of the C-ABI calls sit between NaN guard bands
that must stay NaN.  Rows: decaying noise over four decades of scale, one row with an offset, one all-zero row (R.make_rows).

Bars.  None comes from the kernel: each is 8 x the same figure of a float32 evaluation on the host (scipy.fft keeps single precision),
floored at 2^-24, computed here and printed next to the kernel's figure.  The factor 8 is the margin test_intensity_gpu.py gives
over its fp32 emulation.
  forward    e = max_k |X - X64| / ||x||_2 against numpy.fft.rfft in float64, worst row of the case
  LOG / ABS  |exp(out) - max(|X64|, eps)| <= bar ||x||_2 + 1e-5 max(|X64|, eps)   (|out| <= 24: three ulps of 2^-19 are 5.7e-6)
  filter     max_t |y - y64| / max_t |y64| against the restatement, worst row; yardstick: the same pipeline on scipy.fft in complex64
  moments    1e-12 (|mean| + std) against numpy float64 (R <= 1000 terms of 2^-53 each, with room to spare)
  metric     8 x the deviation of the same formula fed with scipy.fft float32 spectra, floored at 1e-6 of the value
  ratios     2 x the filter bar (two components under a hypot)"""

import functools

import numpy as np
import pytest
import scipy.fft
import torch

import _spectra_ref as R

pytestmark = pytest.mark.gpu
G = 1024          # elements of NaN either side of every output
FACTOR = 8.0
FLOOR = 2.0 ** -24
DT = 0.01
LOG_EPS = 1e-8
LENGTHS = [2, 3, 5, 127, 255, 256, 257, 1000, 4064, 4095, 4096]
FILTER_LENGTHS = [3, 127, 257, 1000, 4064, 4095, 4096]
COMPLEX, ABS, LOG = 0, 1, 2


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def channel_view(rows):
    """float32 numpy (R, N) -> GPU view (R, N) with row stride 3 N into a tensor that is NaN elsewhere"""
    big = torch.full((rows.shape[0], 3, rows.shape[1]), float("nan"), device=_dev())
    big[:, 1] = torch.from_numpy(np.array(rows)).to(_dev())
    v = big[:, 1]
    assert v.stride(0) == 3 * rows.shape[1] and v.stride(1) == 1
    return v


def guarded(n, dtype=torch.float32):
    return torch.full((G + n + G,), float("nan"), device=_dev(), dtype=dtype)


def unguard(buf, n):
    assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all(), "a guard band was written"
    return buf[G:G + n].cpu().numpy()


def gpu_rdft(rows, mode, log_eps=LOG_EPS):
    """rows (R, N) float32 numpy -> numpy (R, K, 2) or (R, K) through tqe_rdft"""
    from tqdne_amd import _lib_eval, spectra
    Rn, N = rows.shape
    K = N // 2 + 1
    n = Rn * K * (2 if mode == COMPLEX else 1)
    v, out = channel_view(rows), guarded(n)
    tab = spectra._tables(N, _dev())
    _lib_eval.check(_lib_eval.load().tqe_rdft(v.data_ptr(), out[G:].data_ptr(), tab.data_ptr(), Rn, N, v.stride(0), mode, log_eps,
                                              _stream()), "rdft")
    return unguard(out, n).reshape((Rn, K, 2) if mode == COMPLEX else (Rn, K))


def gpu_filter(rows, h):
    """rows (R, N) float32, h complex (K,) -> (R, N) through tqe_spectral_filter"""
    from tqdne_amd import _lib_eval, spectra
    Rn, N = rows.shape
    hg = torch.from_numpy(np.stack([h.real, h.imag], -1).astype(np.float32)).to(_dev())
    v, out = channel_view(rows), guarded(Rn * N)
    _lib_eval.check(_lib_eval.load().tqe_spectral_filter(v.data_ptr(), hg.data_ptr(), out[G:].data_ptr(),
                                                         spectra._tables(N, _dev()).data_ptr(), Rn, N, v.stride(0), _stream()), "filter")
    return unguard(out, Rn * N).reshape(Rn, N)


def gpu_moments(a):
    from tqdne_amd import _lib_eval
    Rn, F = a.shape
    ag = torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    mean, std = guarded(F, torch.float64), guarded(F, torch.float64)
    _lib_eval.check(_lib_eval.load().tqe_column_moments(ag.data_ptr(), mean[G:].data_ptr(), std[G:].data_ptr(), Rn, F, _stream()), "moments")
    return unguard(mean, F), unguard(std, F)


@functools.lru_cache(None)
def forward_case(N):
    """(rows, X64, ||x||_2 per row, the case's bar, scipy's figure) -- computed once, shared by the three modes, never modified"""
    x = R.make_rows(5, N)
    X64 = np.fft.rfft(x.astype(np.float64), axis=-1)
    norm = np.linalg.norm(x.astype(np.float64), axis=-1)
    live = norm > 0
    e32 = float((np.abs(scipy.fft.rfft(x, axis=-1) - X64).max(-1)[live] / norm[live]).max())
    for a in (x, X64, norm):
        a.setflags(write=False)
    return x, X64, norm, FACTOR * max(e32, FLOOR), e32


@pytest.mark.parametrize("N", LENGTHS)
def test_forward_complex_against_float64(N):
    x, X64, norm, bar, e32 = forward_case(N)
    got = gpu_rdft(x, COMPLEX)
    X = got[..., 0].astype(np.float64) + 1j * got[..., 1]
    live = norm > 0
    assert live.sum() == 4 and (got[~live] == 0).all()   # the zero row: exact zeros
    e = float((np.abs(X - X64).max(-1)[live] / norm[live]).max())
    print(f"rdft N={N}: e = {e:.3e}, scipy float32 {e32:.3e}, ratio {e / max(e32, FLOOR):.2f}, bar {bar:.3e}")
    assert e <= bar
    # the Python surface: the same launch on the same view, complex64 on the device
    from tqdne_amd import spectra
    y = spectra.rdft(channel_view(x))
    assert y.is_cuda and y.dtype == torch.complex64 and y.shape == (5, N // 2 + 1)
    assert np.array_equal(torch.view_as_real(y).cpu().numpy(), got)


@pytest.mark.parametrize("N", LENGTHS)
def test_abs_and_log_modes(N):
    x, X64, norm, bar, _ = forward_case(N)
    eps32 = np.float64(np.float32(LOG_EPS))
    amp = gpu_rdft(x, ABS).astype(np.float64)
    log = gpu_rdft(x, LOG).astype(np.float64)
    want_abs, want_log = np.abs(X64), np.maximum(np.abs(X64), eps32)
    assert (np.abs(amp - want_abs) <= bar * norm[:, None] + 1e-5 * want_abs).all()
    assert (np.abs(log) <= 24).all()
    assert (np.abs(np.exp(log) - want_log) <= bar * norm[:, None] + 1e-5 * want_log).all()
    zero = np.float32(np.log(eps32))
    assert (np.abs(log[-1] - np.float64(zero)) <= np.spacing(np.abs(zero))).all() and (amp[-1] == 0).all()
    from tqdne_amd import spectra
    v = channel_view(x)
    assert np.array_equal(spectra.amplitude_spectrum(v).cpu().numpy().astype(np.float64), amp)
    assert np.array_equal(spectra.log_amplitude_spectrum(v, LOG_EPS).cpu().numpy().astype(np.float64), log)


@functools.lru_cache(None)
def filter_case(kind, N, Rn=5, seed=0):
    """(rows, y64, the case's bar, the complex64 pipeline's figure)"""
    x = R.make_rows(Rn, N, seed)
    y64 = R.apply_multiplier(kind, x.astype(np.float64), DT)
    y32 = R.apply_multiplier(kind, x, DT, scipy.fft)
    assert y32.dtype == np.float32
    e32 = _filter_error(y32, y64)
    x.setflags(write=False)
    y64.setflags(write=False)
    return x, y64, FACTOR * max(e32, FLOOR), e32


def _filter_error(y, y64):
    top = np.abs(y64).max(-1)
    live = top > 0
    return float((np.abs(y - y64).max(-1)[live] / top[live]).max())


@pytest.mark.parametrize("N", FILTER_LENGTHS)
@pytest.mark.parametrize("kind", ["integrate", "filter"])
def test_filter_against_the_restatement(kind, N):
    from tqdne_amd import spectra
    x, y64, bar, e32 = filter_case(kind, N)
    y = gpu_filter(x, spectra.multiplier(kind, N, DT))
    assert (y[-1] == 0).all()   # the zero row
    e = _filter_error(y, y64)
    print(f"{kind} N={N}: e = {e:.3e}, complex64 pipeline {e32:.3e}, ratio {e / max(e32, FLOOR):.2f}, bar {bar:.3e}")
    assert e <= bar
    fn = spectra.integrate_frequency_domain if kind == "integrate" else spectra.filter_frequency_domain
    out = fn(channel_view(x), DT)
    assert out.is_cuda and out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), y)
    assert np.array_equal(spectra.spectral_filter(channel_view(x), spectra.multiplier(kind, N, DT)).cpu().numpy(), y)


def test_filter_edge_lengths():
    from tqdne_amd import spectra
    # N = 2: DC is removed and the Nyquist multiplier is imaginary on a real bin -- identically zero in the reference
    x = R.make_rows(5, 2)
    h = spectra.multiplier("integrate", 2, DT)
    y = gpu_filter(x, h)
    assert (np.abs(y) <= 2.0 ** -24 * np.abs(h).max() * np.abs(x).max()).all()
    # N = 8 at dt = 10: every bin lies below 0.1 Hz
    x = R.make_rows(5, 8)
    for kind in ("integrate", "filter"):
        h = spectra.multiplier(kind, 8, 10.0)
        assert (h == 0).all()
        assert (gpu_filter(x, h) == 0).all()
        fn = spectra.integrate_frequency_domain if kind == "integrate" else spectra.filter_frequency_domain
        assert (fn(x, 10.0) == 0).all()


def test_fft_and_host_inputs_follow_the_reference():
    from tqdne_amd import spectra
    x, X64, norm, bar, _ = forward_case(1000)
    x = x.copy()   # (torch.from_numpy wants a writable array)
    fr, amp = spectra.fft(x[0], DT)
    wf, wa = R.fft(x[0], DT)
    assert isinstance(fr, np.ndarray) and isinstance(amp, np.ndarray) and amp.dtype == np.float32 and amp.shape == (500,)
    assert np.array_equal(fr, wf) and (np.abs(amp - wa) <= bar * norm[0] + 1e-5 * wa).all()
    fr, amp = spectra.fft(torch.from_numpy(x).to(_dev()), DT)
    assert fr.is_cuda and amp.is_cuda and amp.shape == (5, 500)
    y = spectra.rdft(torch.from_numpy(x))   # CPU tensor in, CPU tensor out
    assert isinstance(y, torch.Tensor) and not y.is_cuda and y.dtype == torch.complex64
    y3 = spectra.rdft(x.reshape(5, 1, 1000))   # leading axes are kept
    assert isinstance(y3, np.ndarray) and y3.dtype == np.complex64 and np.array_equal(y3[:, 0], y.numpy())
    t = torch.from_numpy(x).to(_dev()).t().contiguous().t()   # strided samples: copied, same values
    assert np.array_equal(spectra.rdft(t).cpu().numpy(), y.numpy())


@pytest.mark.parametrize("F", [1, 3, 2033, 2049])
@pytest.mark.parametrize("Rn", [1, 2, 70, 1000])
def test_column_moments_against_float64(Rn, F):
    from tqdne_amd import spectra
    rng = np.random.default_rng(Rn * 10007 + F)
    a = (rng.standard_normal((Rn, F)) * 10.0 ** rng.uniform(-2, 2, F) + rng.uniform(-20, 5, F)).astype(np.float32)
    mean, std = gpu_moments(a)
    a64 = a.astype(np.float64)
    wm, ws = a64.mean(0), a64.std(0)
    tol = 1e-12 * (np.abs(wm) + ws)
    assert (np.abs(mean - wm) <= tol).all() and (np.abs(std - ws) <= tol).all()
    if Rn == 1:
        assert (std == 0).all() and np.array_equal(mean, a64[0])
    m2, s2 = spectra.column_moments(torch.from_numpy(a).to(_dev()))
    assert m2.is_cuda and m2.dtype == torch.float64 and np.array_equal(m2.cpu().numpy(), mean) and np.array_equal(s2.cpu().numpy(), std)


# ---- bitwise properties -------------------------------------------------------------------------------------------

def _all_kernels(x, N):
    from tqdne_amd import spectra
    return [gpu_rdft(x, COMPLEX), gpu_rdft(x, ABS), gpu_rdft(x, LOG), gpu_filter(x, spectra.multiplier("integrate", N, DT))]


@pytest.mark.parametrize("N", [256, 1000, 4064])
def test_rows_are_independent_of_the_batch_and_repeatable_bit_for_bit(N):
    base = R.make_rows(70, N, seed=3)
    row = base[7:8].copy()
    alone = _all_kernels(row, N)
    again = _all_kernels(row, N)
    in5 = _all_kernels(np.concatenate([base[:2], row, base[3:5]]), N)        # position 2 of 5
    in70 = _all_kernels(np.concatenate([base[:41], row, base[42:]]), N)      # position 41 of 70
    for a, b, c, d in zip(alone, again, in5, in70):
        assert np.array_equal(a, b) and np.array_equal(a[0], c[2]) and np.array_equal(a[0], d[41])


def test_column_moments_are_repeatable_and_independent_of_the_other_columns():
    rng = np.random.default_rng(11)
    a = rng.standard_normal((70, 2033)).astype(np.float32)
    m, s = gpu_moments(a)
    m2, s2 = gpu_moments(a)
    assert np.array_equal(m, m2) and np.array_equal(s, s2)
    for col in (0, 31, 32, 2032):
        m1, s1 = gpu_moments(a[:, col:col + 1])
        assert m1[0] == m[col] and s1[0] == s[col]
        m3, s3 = gpu_moments(np.concatenate([a[:, 100:105], a[:, col:col + 1]], axis=1))
        assert m3[5] == m[col] and s3[5] == s[col]


@pytest.mark.parametrize("N", [256, 1000])
def test_a_non_finite_row_is_all_nan_and_its_neighbours_are_untouched(N):
    clean = R.make_rows(5, N, seed=5)[:4]   # four non-zero rows
    dirty = clean.copy()
    dirty[1, N // 3] = np.nan
    dirty[2, N - 1] = np.inf
    for a, b in zip(_all_kernels(clean, N), _all_kernels(dirty, N)):
        assert np.isnan(b[1]).all() and np.isnan(b[2]).all()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and np.isfinite(b[[0, 3]]).all()


# ---- the metric, end to end -----------------------------------------------------------------------------------------

def _metric_data(n, T, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    pred = (rng.standard_normal((n, 3, T)) * np.exp(-t / (T / 3.0))).astype(np.float32)
    target = (1.3 * rng.standard_normal((n, 3, T)) * np.exp(-t / (T / 2.0))).astype(np.float32)
    return pred, target


@pytest.mark.parametrize("T", [4064, 257])
def test_metric_on_the_device_against_its_host_path(T):
    from tqdne_amd import metric
    pred, target = _metric_data(70, T, 17)
    pg, tg = torch.from_numpy(pred).to(_dev()), torch.from_numpy(target).to(_dev())
    for ch in (1, None):
        m = metric.AmplitudeSpectralDensity(fs=100, channel=ch)
        host = m(pred.astype(np.float64), target.astype(np.float64))   # the same values: the host path then computes in float64
        dev = m(pg, tg)
        assert isinstance(host, np.float64) and type(dev) is type(m(pg[:2].cpu(), tg[:2].cpu()))   # the type the host path gives
        p, t = (pred, target) if ch is None else (pred[:, ch], target[:, ch])
        sp, st = (R.log_spectra(a, m.log_eps, scipy.fft) for a in (p, t))
        assert sp.dtype == np.float32
        yard = abs(R.asd_isotropic(sp.reshape(70, -1), st.reshape(70, -1)) - host)
        bar = max(FACTOR * yard, 1e-6 * abs(host))
        print(f"ASD T={T} channel={ch}: host {host:.9g}, device {dev:.9g}, |diff| {abs(dev - host):.3e}, float32 spectra {yard:.3e}, bar {bar:.3e}")
        assert abs(dev - host) <= bar


def test_metric_with_full_covariance_forms_the_spectra_on_the_device():
    from tqdne_amd import metric
    pred, target = _metric_data(70, 64, 23)
    m = metric.AmplitudeSpectralDensity(fs=100, channel=2, isotropic=False)
    host = m(pred.astype(np.float64), target.astype(np.float64))
    dev = m(torch.from_numpy(pred).to(_dev()), torch.from_numpy(target).to(_dev()))
    sp, st = (R.log_spectra(a[:, 2], m.log_eps, scipy.fft).astype(np.float64) for a in (pred, target))
    yard = abs(metric.frechet_distance(sp, st) - host)
    bar = max(FACTOR * yard, 1e-6 * abs(host))
    print(f"ASD full covariance: host {host:.9g}, device {dev:.9g}, |diff| {abs(dev - host):.3e}, float32 spectra {yard:.3e}, bar {bar:.3e}")
    assert abs(dev - host) <= bar


# ---- evaluate_ratio ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("PGV", [True, False])
@pytest.mark.parametrize("kanno", [False, True])
@pytest.mark.parametrize("evaluate_obs", [True, False])
def test_evaluate_ratio_against_the_restatement(PGV, kanno, evaluate_obs):
    from tqdne_amd import ground_motion as GM
    T = 1000
    target = R.make_rows(14, T, seed=31).reshape(7, 2, T)   # (the all-zero row is one component of the last pair)
    predicted = R.make_rows(14, T, seed=37).reshape(7, 2, T)
    kind = "integrate" if PGV else "filter"
    e32 = max(_filter_error(R.apply_multiplier(kind, w, DT, scipy.fft), R.apply_multiplier(kind, w.astype(np.float64), DT))
              for w in (target.reshape(14, T), predicted.reshape(14, T)))
    bar = 2 * FACTOR * max(e32, FLOOR)
    want = R.evaluate_ratio(target.astype(np.float64), predicted.astype(np.float64), DT, evaluate_obs, PGV, kanno)
    got = GM.evaluate_ratio(target, predicted, dt=DT, n_worker=3, evaluate_obs=evaluate_obs, PGV=PGV, kanno=kanno)
    on_gpu = GM.evaluate_ratio(torch.from_numpy(target).to(_dev()), torch.from_numpy(predicted).to(_dev()), DT, 4, evaluate_obs, PGV, kanno)
    if not evaluate_obs:
        want, got, on_gpu = {"only": want}, {"only": got}, {"only": on_gpu}
    assert sorted(got) == sorted(want) == sorted(on_gpu)
    for k in want:
        assert isinstance(got[k], np.ndarray) and got[k].shape == want[k].shape == (7,) and on_gpu[k].is_cuda
        assert np.array_equal(on_gpu[k].cpu().numpy(), got[k])
        err = float((np.abs(got[k] - want[k]) / want[k]).max())
        print(f"evaluate_ratio PGV={PGV} kanno={kanno} {k}: {err:.3e}, bar {bar:.3e}")
        assert err <= bar


def test_lengths_above_the_limit_are_refused_by_name():
    from tqdne_amd import ground_motion as GM, metric, spectra
    x = torch.zeros(2, 3, 4097, device=_dev())
    for call in (lambda: spectra.rdft(x), lambda: spectra.log_amplitude_spectrum(x), lambda: spectra.integrate_frequency_domain(x, DT),
                 lambda: metric.AmplitudeSpectralDensity(fs=100)(x, x), lambda: GM.evaluate_ratio(x, x)):
        with pytest.raises(ValueError, match="limit of 4096 samples"):
            call()
