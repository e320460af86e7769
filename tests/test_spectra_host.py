"""Host-side checks of the evaluation library libtqdne_eval.so (include/tqdne_eval.h, tqdne_amd/_lib_eval.py, csrc_eval/) and of
tqdne_amd/spectra.py: the C surface stated once and held against its three hand-written statements (the shape of test_abi_host.py),
the tables against a float64 recomputation, every argument check without a device, the float64 restatement of the reference
(tests/_spectra_ref.py) against an explicit DFT matrix and the analytic integral of on-bin sinusoids, and the Python surface."""

import ctypes
import functools
import glob
import os
import re

import numpy as np
import pytest
import torch

import _spectra_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ABI = 1
SURFACE = """
    tqe_abi_version tqe_column_moments tqe_rdft tqe_rdft_max_length tqe_rdft_table_floats tqe_rdft_tables tqe_spectral_filter
""".split()
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "int64_t": ctypes.c_int64}


@functools.lru_cache(None)
def _built():
    """(binding module, loaded library, header text without comments)"""
    from tqdne_amd import _build, _lib_eval
    _build.build(verbose=False)
    header = open(os.path.join(ROOT, "include", "tqdne_eval.h")).read()
    return _lib_eval, _lib_eval.load(), re.sub(r"/\*.*?\*/", "", header, flags=re.S)


@functools.lru_cache(None)
def _header_prototypes():
    protos = {}
    for res, name, params in re.findall(r"^(\w+)\s+(tqe_\w+)\s*\((.*?)\)\s*;", _built()[2], re.S | re.M):
        assert name not in protos, name
        params = " ".join(params.split())
        protos[name] = (res, [] if params == "void" else [p.strip() for p in params.split(",")])
    return protos


def test_the_surface_is_the_list_in_the_header_the_binding_the_library_and_the_sources():
    from tqdne_amd import _build, _lib
    L, lib, header = _built()
    assert SURFACE == sorted(set(SURFACE)) and len(SURFACE) == 7
    assert re.search(r"^#define TQE_ABI_VERSION %d$" % ABI, header, re.M) and L.ABI_VERSION == ABI and lib.tqe_abi_version() == ABI
    assert set(_header_prototypes()) == set(SURFACE)
    assert set(L._PROTOS) == set(SURFACE) == set(L.exported_symbols())
    assert [n for n in SURFACE if not hasattr(lib, n)] == []
    defined = []
    paths = sorted(glob.glob(os.path.join(ROOT, "tqdne_amd", "csrc_eval", "*")))
    assert [os.path.basename(p) for p in paths] == sorted(_build.EVAL_SOURCES)
    for path in paths:
        text = open(path).read()
        found = re.findall(r'extern "C"\s+(?:int|size_t)\s+(\w+)\s*\(', text)
        assert len(found) == text.count('extern "C"'), f"{path}: an extern \"C\" this scan does not read"
        defined += found
    assert sorted(set(defined)) == SURFACE
    # two libraries, two name spaces: nothing of this one is in the model library's binding or sources list
    assert not set(L._PROTOS) & set(_lib._PROTOS) and not set(_build.EVAL_SOURCES) & set(_build.SOURCES)
    assert os.path.basename(_build.EVAL_LIBPATH) == "libtqdne_eval.so" and os.path.exists(_build.EVAL_LIBPATH)
    assert _build.build(verbose=False) == _build.LIBPATH and not _build.eval_needs_build()


@pytest.mark.parametrize("name", SURFACE)
def test_binding_prototype_matches_the_header(name):
    L = _built()[0]
    h_res, h_params = _header_prototypes()[name]
    res, args = L._PROTOS[name]
    assert res is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[h_res]
    assert len(args) == len(h_params), (len(args), h_params)
    for i, (p, a) in enumerate(zip(h_params, args)):
        if "*" in p or p.startswith("hipStream_t"):
            assert a is ctypes.c_void_p, (i, p, a)
        else:
            assert a is _SCALARS[p.split()[0]], (i, p, a)


def test_binding_constants_match_the_header():
    L, lib, header = _built()
    consts = {}
    for name, expr in re.findall(r"^#define\s+(TQE?_\w+)[ \t]+(\S.*)$", header, re.M):
        consts[name] = eval(expr, {"__builtins__": {}}, dict(consts))
    assert consts["TQ_ERR_ARG"] == -1 and consts["TQ_ERR_SHAPE"] == -2 and consts["TQE_RDFT_MAX_LENGTH"] == 4096
    bound = {n: v for n, v in vars(L).items() if n.startswith(("TQ_", "TQE_"))}
    assert {"TQ_ERR_ARG", "TQ_ERR_SHAPE", "TQE_RDFT_COMPLEX", "TQE_RDFT_ABS", "TQE_RDFT_LOG", "TQE_RDFT_MAX_LENGTH"} == set(bound)
    assert {n: v for n, v in bound.items() if consts[n] != v} == {}
    assert lib.tqe_rdft_max_length() == consts["TQE_RDFT_MAX_LENGTH"]


def _plan(N):
    pow2 = N & (N - 1) == 0
    M = 1
    while M < (N if pow2 else 2 * N - 1):
        M *= 2
    return M, pow2


def _bitrev(M):
    bits = M.bit_length() - 1
    j = np.arange(M)
    k = np.zeros(M, np.int64)
    for b in range(bits):
        k |= ((j >> b) & 1) << (bits - 1 - b)
    return k


@pytest.mark.parametrize("N", [2, 3, 5, 8, 127, 256, 257, 1000, 4064, 4095, 4096])
def test_tables_are_the_float64_values_rounded_once(N):
    from tqdne_amd import spectra
    lib = _built()[1]
    M, pow2 = _plan(N)
    n_floats = M if pow2 else 3 * M + 2 * N
    assert lib.tqe_rdft_table_floats(N) == n_floats
    tab = spectra.rdft_tables(N)
    assert tab.dtype == np.float32 and tab.shape == (n_floats,)

    def one_rounding(got, want, slack):
        got = got.astype(np.float64).view(np.complex128) if got.dtype != np.complex128 else got
        for g, w in ((got.real, want.real), (got.imag, want.imag)):
            assert (np.abs(g - w) <= 2.0 ** -24 * np.abs(w) + slack).all(), float(np.abs(g - w).max())

    j = np.arange(M // 2)
    tw = np.exp(-2j * np.pi * j / M)
    one_rounding(tab[:M].astype(np.float64).view(np.complex128), tw, 1e-15)
    assert tab[0] == 1.0 and tab[1] == 0.0
    if pow2:
        return
    n = np.arange(N, dtype=np.int64)
    c = np.exp(-1j * np.pi * ((n * n) % (2 * N)) / N)
    one_rounding(tab[M:M + 2 * N].astype(np.float64).view(np.complex128), c, 1e-15)
    b = np.zeros(M, np.complex128)
    b[:N] = np.conj(c)
    b[M - N + 1:] = np.conj(c[1:][::-1])
    want = (np.fft.fft(b) / M)[_bitrev(M)]
    # (two float64 FFTs of M points differ by a few 1e-16 of the largest entry, sqrt(N) / M at most 0.05)
    one_rounding(tab[M + 2 * N:].astype(np.float64).view(np.complex128), want, 1e-15)


def test_table_floats_is_zero_where_there_is_no_kernel():
    lib = _built()[1]
    for N in (-1, 0, 1, 4097, 8192, 1 << 30):
        assert lib.tqe_rdft_table_floats(N) == 0
    assert lib.tqe_rdft_table_floats(2) == 2 and lib.tqe_rdft_table_floats(4096) == 4096
    assert lib.tqe_rdft_table_floats(4095) == 3 * 8192 + 2 * 4095


def test_c_abi_argument_checks_return_error_codes_without_a_gpu():
    lib = _built()[1]
    fake = 0x1000   # never dereferenced: every call below is rejected during validation
    buf = np.zeros(64, np.float32)
    assert lib.tqe_rdft_tables(8, None) == -1
    assert lib.tqe_rdft_tables(1, buf.ctypes.data) == -2 and lib.tqe_rdft_tables(4097, buf.ctypes.data) == -2
    assert lib.tqe_rdft_tables(8, buf.ctypes.data) == 0 and lib.tqe_rdft_tables(5, buf.ctypes.data) == 0
    rd = lambda x=fake, o=fake, t=fake, R=3, N=100, ld=100, mode=0, eps=1e-8: lib.tqe_rdft(x, o, t, R, N, ld, mode, eps, None)
    assert rd(x=None) == -1 and rd(o=None) == -1 and rd(t=None) == -1
    assert rd(mode=3) == -1 and rd(mode=-1) == -1
    assert rd(mode=2, eps=0.0) == -1 and rd(mode=2, eps=-1.0) == -1 and rd(mode=2, eps=float("nan")) == -1
    assert rd(R=0) == -2 and rd(R=-1) == -2
    assert rd(N=1, ld=1) == -2 and rd(N=0) == -2 and rd(N=4097, ld=4097) == -2
    assert rd(ld=99) == -2 and rd(ld=0) == -2 and rd(ld=-100) == -2
    fl = lambda x=fake, h=fake, y=fake, t=fake, R=3, N=100, ld=100: lib.tqe_spectral_filter(x, h, y, t, R, N, ld, None)
    assert fl(x=None) == -1 and fl(h=None) == -1 and fl(y=None) == -1 and fl(t=None) == -1
    assert fl(R=0) == -2 and fl(N=1, ld=1) == -2 and fl(N=4097, ld=4097) == -2 and fl(ld=99) == -2
    cm = lambda a=fake, m=fake, s=fake, R=3, F=5: lib.tqe_column_moments(a, m, s, R, F, None)
    assert cm(a=None) == -1 and cm(m=None) == -1 and cm(s=None) == -1
    assert cm(R=0) == -2 and cm(F=0) == -2 and cm(R=-1) == -2 and cm(F=-1) == -2


# ---- the restatement ----------------------------------------------------------------------------------------------

def _dft_matrix(N, sign):
    n = np.arange(N)
    return np.exp(sign * 2j * np.pi * ((n[:, None] * n[None, :]) % N) / N)


@pytest.mark.parametrize("N", [2, 3, 8, 127, 256, 257])
@pytest.mark.parametrize("kind", ["integrate", "filter"])
def test_restatement_is_the_explicit_dft_matrix_evaluation(N, kind):
    """the reference's lines, one signal at a time, with the transforms written as matrix products"""
    dt = 0.01 if N > 8 else 1.0
    x = R.make_rows(3, N).astype(np.float64)
    f = np.array([k if k < (N + 1) // 2 else k - N for k in range(N)], np.float64) * (1.0 / (N * dt))   # numpy.fft.fftfreq
    assert np.array_equal(f, np.fft.fftfreq(N, dt))
    for row in x:
        X = _dft_matrix(N, -1) @ row
        X = X * (np.abs(f) >= 0.1)
        if kind == "integrate":
            X[1:] = X[1:] / (1j * 2 * np.pi * f[1:])
            X[0] = 0
        want = ((_dft_matrix(N, +1) @ X) / N).real
        got = R.apply_multiplier(kind, row, dt)
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), np.abs(row).max())
    # batched == row by row, and the half-spectrum multiplier of the package is the restatement's on the non-negative bins
    from tqdne_amd import spectra
    assert np.array_equal(R.apply_multiplier(kind, x, dt)[1], R.apply_multiplier(kind, x[1], dt))
    h, full = spectra.multiplier(kind, N, dt), R.full_multiplier(kind, N, dt)
    K = N // 2 + 1
    assert np.array_equal(h[:(N + 1) // 2], full[:(N + 1) // 2])
    if N % 2 == 0:   # the Nyquist bin: fftfreq calls it negative; only its real part matters (it multiplies a real bin)
        assert h[K - 1].real == full[K - 1].real and abs(h[K - 1].imag) == abs(full[K - 1].imag)
    assert np.array_equal(np.conj(h[1:(N + 1) // 2]), full[:N // 2:-1][:(N - 1) // 2])


def test_restatement_integrates_and_passes_on_bin_sinusoids():
    N, dt = 1000, 0.01
    n = np.arange(N)
    for k in (1, 2, 7, 100, 499):   # f = k / (N dt) = 0.1 k Hz: at or above the corner
        f = k / (N * dt)
        phase = 2 * np.pi * ((k * n) % N) / N + 0.3   # (2 pi f t with the whole turns taken out in integers)
        a = np.cos(phase)
        want = np.sin(phase) / (2 * np.pi * f)
        assert np.abs(R.integrate_frequency_domain(a, dt) - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(R.filter_frequency_domain(a, dt) - a).max() <= 1e-12
    # below the corner (N dt = 20 s: bin 1 is 0.05 Hz) and DC are removed
    N = 2000
    t = np.arange(N) * dt
    low = 2.0 + np.cos(2 * np.pi * 0.05 * t)
    assert np.abs(R.filter_frequency_domain(low, dt)).max() <= 1e-12
    assert np.abs(R.integrate_frequency_domain(low, dt)).max() <= 1e-12
    # N = 2: only DC (removed) and the Nyquist bin, whose multiplier is imaginary on a real bin
    assert np.array_equal(R.integrate_frequency_domain(np.array([1.0, -2.0]), dt), np.zeros(2))
    # every bin masked
    assert np.array_equal(R.filter_frequency_domain(R.make_rows(2, 8), 10.0), np.zeros((2, 8)))


def test_restatement_fft_and_reductions():
    x = R.make_rows(4, 50).astype(np.float64)
    fr, amp = R.fft(x[0], 0.02)
    assert fr.shape == amp.shape == (25,) and np.allclose(fr, np.arange(25) / (50 * 0.02))
    assert np.abs(amp - np.abs(_dft_matrix(50, -1) @ x[0])[:25]).max() <= 1e-12 * np.abs(amp).max()
    # the median over the rotation angles does not depend on the angle
    for i in range(3):
        assert abs(R.gmrotd50_by_rotation(x[i], x[i + 1]) - R.gmrotd50(x[i], x[i + 1])) <= 1e-12 * R.gmrotd50(x[i], x[i + 1])
    assert np.allclose(R.kanno(x[:2], x[2:]), [np.hypot(np.abs(x[0]).max(), np.abs(x[2]).max()), np.hypot(np.abs(x[1]).max(), np.abs(x[3]).max())])
    w = np.stack([x[:2], x[2:]], axis=1)   # (2, 2, 50)
    out = R.evaluate_ratio(w, 2 * w, dt=0.02)
    assert sorted(out) == ["PGV_geom_mean_gwm", "PGV_geom_mean_obs"] and out["PGV_geom_mean_obs"].shape == (2,)
    assert np.allclose(out["PGV_geom_mean_gwm"], 2 * out["PGV_geom_mean_obs"])
    v = R.integrate_frequency_domain(w, 0.02)
    assert np.allclose(out["PGV_geom_mean_obs"], [R.gmrotd50_by_rotation(v[i, 1], v[i, 0]) for i in range(2)])
    assert sorted(R.evaluate_ratio(w, w, PGV=False)) == ["PGA_geom_mean_gwm", "PGA_geom_mean_obs"]
    assert R.evaluate_ratio(w, w, evaluate_obs=False, kanno_=True).shape == (2,)


# ---- the Python surface -------------------------------------------------------------------------------------------

def test_class_and_function_surface():
    import inspect
    import tqdne_amd
    from tqdne_amd import ground_motion as G, metric, spectra
    for name in ("rdft", "amplitude_spectrum", "log_amplitude_spectrum", "spectral_filter", "column_moments",
                 "integrate_frequency_domain", "filter_frequency_domain"):
        assert getattr(tqdne_amd, name) is getattr(spectra, name) and name in tqdne_amd.__all__ and name in spectra.__all__
    assert tqdne_amd.spectra is spectra and callable(spectra.fft) and "fft" in spectra.__all__
    assert tqdne_amd.evaluate_ratio is G.evaluate_ratio and "evaluate_ratio" in tqdne_amd.__all__
    assert str(inspect.signature(G.evaluate_ratio)) == "(target, predicted, dt=0.01, n_worker=4, evaluate_obs=True, PGV=True, kanno=False)"
    assert str(inspect.signature(spectra.log_amplitude_spectrum)) == "(x, log_eps=1e-08)"
    assert str(inspect.signature(spectra.fft)) == "(signal, dt=0.01)"
    assert "does not depend on the angle" in G.calculate_gmrotd50.__doc__
    assert spectra.max_length() == 4096
    m = metric.AmplitudeSpectralDensity(fs=100, channel=1, log_eps=1e-6, isotropic=False)
    assert (m.fs, m.channel, m.log_eps, m.isotropic) == (100, 1, 1e-6, False) and m.name == "AmplitudeSpectralDensity - Channel 1"
    assert callable(m.compute_device)


def test_numpy_input_to_the_metric_is_the_formula_on_the_host():
    from tqdne_amd import metric
    rng = np.random.default_rng(5)
    pred, target = rng.standard_normal((9, 3, 257)), 1.5 * rng.standard_normal((11, 3, 257))
    for ch in (0, 2):
        m = metric.AmplitudeSpectralDensity(fs=100, channel=ch)
        want = R.asd_isotropic(R.log_spectra(pred[:, ch]), R.log_spectra(target[:, ch]))
        for a, b in ((pred, target), (torch.from_numpy(pred), torch.from_numpy(target)), (pred, torch.from_numpy(target))):
            got = m(a, b)
            assert isinstance(got, np.float64) and abs(got - want) <= 1e-12 * want
    full = metric.AmplitudeSpectralDensity(fs=100, channel=0, isotropic=False)(pred[:, :, :16], target[:, :, :16])
    sp, st = R.log_spectra(pred[:, 0, :16]), R.log_spectra(target[:, 0, :16])
    assert abs(full - metric.frechet_distance(sp, st)) <= 1e-9 * abs(full)


def test_python_argument_checks():
    from tqdne_amd import ground_motion as G, spectra
    long = np.zeros((2, 4097), np.float32)
    for call in (lambda: spectra.rdft(long), lambda: spectra.amplitude_spectrum(long), lambda: spectra.log_amplitude_spectrum(long),
                 lambda: spectra.spectral_filter(long, np.zeros(2049, np.complex64)), lambda: spectra.integrate_frequency_domain(long, 0.01),
                 lambda: spectra.filter_frequency_domain(long, 0.01), lambda: spectra.fft(long[0]),
                 lambda: G.evaluate_ratio(np.zeros((1, 2, 4097)), np.zeros((1, 2, 4097)))):
        with pytest.raises(ValueError, match="limit of 4096 samples"):
            call()
    x = np.zeros((2, 16), np.float32)
    with pytest.raises(ValueError, match="N >= 2"):
        spectra.rdft(x[:, :1])
    with pytest.raises(ValueError, match="scalar"):
        spectra.rdft(np.float32(1.0))
    for eps in (0.0, -1.0, 1e-60, float("nan")):
        with pytest.raises(ValueError, match="log_eps"):
            spectra.log_amplitude_spectrum(x, eps)
    for h in (np.zeros(8, np.complex64), np.zeros((9, 3), np.float32), np.zeros((2, 9), np.complex64)):
        with pytest.raises(ValueError, match="9 non-negative bins"):
            spectra.spectral_filter(x, h)
    for dt in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dt"):
            spectra.integrate_frequency_domain(x, dt)
        with pytest.raises(ValueError, match="dt"):
            spectra.fft(x[0], dt)
    for a in (np.zeros(4), np.zeros((0, 4)), np.zeros((4, 0)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match=r"\(R, F\)"):
            spectra.column_moments(a)
    for w in (np.zeros((3, 16)), np.zeros((3, 1, 16))):
        with pytest.raises(ValueError, match=r"\(n, 2, T\)"):
            G.evaluate_ratio(w, w)


def test_no_gpu_is_refused_by_name():
    """there is no host fallback behind the device functions: host inputs are either computed on a GPU or refused"""
    from tqdne_amd import ground_motion as G, spectra
    x = np.ones((2, 16), np.float32)
    w = np.ones((2, 2, 16), np.float32)
    for call in (lambda: spectra.rdft(x), lambda: spectra.amplitude_spectrum(torch.ones(2, 16)), lambda: spectra.log_amplitude_spectrum(x),
                 lambda: spectra.spectral_filter(x, np.ones(9, np.complex64)), lambda: spectra.integrate_frequency_domain(x, 0.01),
                 lambda: spectra.filter_frequency_domain(x, 0.01), lambda: spectra.fft(x[0]), lambda: spectra.column_moments(x),
                 lambda: G.evaluate_ratio(w, w)):
        if torch.cuda.is_available():
            assert call() is not None
        else:
            with pytest.raises(RuntimeError, match="GPU"):
                call()


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from tqdne_amd import _build, _lib_eval
    monkeypatch.setattr(_lib_eval, "_LIB", None)
    monkeypatch.setattr(_build, "EVAL_LIBPATH", str(tmp_path / "libtqdne_eval.so"))
    with pytest.raises(RuntimeError, match="libtqdne_eval.so is missing"):
        _lib_eval.load()
