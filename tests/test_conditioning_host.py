"""Host-side checks of the conditioning library libtqdne_series.so (include/tqdne_series.h, tqdne_amd/_lib_series.py, csrc_series/)
and of tqdne_amd/conditioning.py: the C surface held against its three hand-written statements (the shape of test_spectra_host.py),
every argument check without a device, the filter designs against scipy and obspy's construction, the host paths against the
reference's arithmetic bit for bit, and the float64 restatement (tests/_conditioning_ref.py) against scipy and a literal loop."""

import ctypes
import functools
import glob
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import scipy.signal
import torch

import _conditioning_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ABI = 1
SURFACE = "tqs_abi_version tqs_hold_envelope tqs_sosfilt tqs_sosfilt_max_sections".split()
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "int64_t": ctypes.c_int64}


@functools.lru_cache(None)
def _built():
    """(binding module, loaded library, header text without comments)"""
    from tqdne_amd import _build, _lib_series
    _build.build(verbose=False)
    header = open(os.path.join(ROOT, "include", "tqdne_series.h")).read()
    return _lib_series, _lib_series.load(), re.sub(r"/\*.*?\*/", "", header, flags=re.S)


@functools.lru_cache(None)
def _header_prototypes():
    protos = {}
    for res, name, params in re.findall(r"^(\w+)\s+(tqs_\w+)\s*\((.*?)\)\s*;", _built()[2], re.S | re.M):
        assert name not in protos, name
        params = " ".join(params.split())
        protos[name] = (res, [] if params == "void" else [p.strip() for p in params.split(",")])
    return protos


# ---- the C surface ------------------------------------------------------------------------------------------------

def test_the_surface_is_the_list_in_the_header_the_binding_the_library_and_the_sources():
    from tqdne_amd import _build, _lib, _lib_eval
    L, lib, header = _built()
    assert SURFACE == sorted(set(SURFACE)) and len(SURFACE) == 4
    assert re.search(r"^#define TQS_ABI_VERSION %d$" % ABI, header, re.M) and L.ABI_VERSION == ABI and lib.tqs_abi_version() == ABI
    assert set(_header_prototypes()) == set(SURFACE)
    assert set(L._PROTOS) == set(SURFACE) == set(L.exported_symbols())
    assert [n for n in SURFACE if not hasattr(lib, n)] == []
    defined = []
    paths = sorted(glob.glob(os.path.join(ROOT, "tqdne_amd", "csrc_series", "*")))
    assert [os.path.basename(p) for p in paths] == sorted(_build.SERIES_SOURCES) == ["series.hip"]
    for path in paths:
        text = open(path).read()
        found = re.findall(r'extern "C"\s+int\s+(\w+)\s*\(', text)
        assert len(found) == text.count('extern "C"'), f"{path}: an extern \"C\" this scan does not read"
        defined += found
    assert sorted(set(defined)) == SURFACE
    # three libraries, three disjoint name spaces and source lists
    names = [set(L._PROTOS), set(_lib_eval._PROTOS), set(_lib._PROTOS)]
    assert len(set.union(*names)) == sum(len(n) for n in names)
    assert all(n.startswith("tqs_") for n in names[0]) and not any(n.startswith("tqs_") for n in names[1] | names[2])
    sources = [_build.SERIES_SOURCES, _build.EVAL_SOURCES, _build.SOURCES]
    assert len(set(sum(sources, []))) == sum(len(s) for s in sources)
    assert len({_build.SERIES_LIBPATH, _build.EVAL_LIBPATH, _build.LIBPATH}) == 3
    assert os.path.basename(_build.SERIES_LIBPATH) == "libtqdne_series.so" and L.lib_path() == _build.SERIES_LIBPATH


def test_build_leaves_all_three_libraries_fresh():
    from tqdne_amd import _build
    _built()
    assert _build.build(verbose=False) == _build.LIBPATH
    assert not _build.needs_build() and not _build.eval_needs_build() and not _build.series_needs_build()
    for path in (_build.LIBPATH, _build.EVAL_LIBPATH, _build.SERIES_LIBPATH):
        assert os.path.exists(path)
    assert os.path.basename(_build.CSRC_SERIES) == "csrc_series"


@pytest.mark.parametrize("name", SURFACE)
def test_binding_prototype_matches_the_header(name):
    L = _built()[0]
    h_res, h_params = _header_prototypes()[name]
    res, args = L._PROTOS[name]
    assert h_res == "int" and res is ctypes.c_int
    assert len(args) == len(h_params), (len(args), h_params)
    for i, (p, a) in enumerate(zip(h_params, args)):
        if "*" in p or p.startswith("hipStream_t"):
            assert a is ctypes.c_void_p, (i, p, a)
        else:
            assert a is _SCALARS[p.split()[0]], (i, p, a)


def test_binding_constants_match_the_header():
    L, lib, header = _built()
    consts = {}
    for name, expr in re.findall(r"^#define\s+(TQS?_\w+)[ \t]+(\S.*)$", header, re.M):
        consts[name] = eval(expr, {"__builtins__": {}}, dict(consts))
    assert consts["TQ_ERR_ARG"] == -1 and consts["TQ_ERR_SHAPE"] == -2 and consts["TQS_SOSFILT_MAX_SECTIONS"] == 8
    assert (consts["TQS_DETREND_NONE"], consts["TQS_DETREND_DEMEAN"], consts["TQS_DETREND_LINEAR"]) == (0, 1, 2)
    bound = {n: v for n, v in vars(L).items() if n.startswith(("TQ_", "TQS_"))}
    assert {"TQ_ERR_ARG", "TQ_ERR_SHAPE", "TQS_DETREND_NONE", "TQS_DETREND_DEMEAN", "TQS_DETREND_LINEAR",
            "TQS_SOSFILT_MAX_SECTIONS"} == set(bound)
    assert {n: v for n, v in bound.items() if consts[n] != v} == {}
    assert lib.tqs_sosfilt_max_sections() == consts["TQS_SOSFILT_MAX_SECTIONS"]
    from tqdne_amd import conditioning
    assert conditioning.max_sections() == 8


def test_c_abi_argument_checks_return_error_codes_without_a_gpu():
    lib = _built()[1]
    fake, other = 0x1000, 0x100000   # never dereferenced: every call below is rejected during validation
    sf = lambda x=fake, y=other, sos=fake, R=3, T=100, ldx=100, ldy=100, n=4, detrend=0: lib.tqs_sosfilt(x, y, sos, R, T, ldx, ldy, n,
                                                                                                           detrend, None)
    assert sf(x=None) == -1 and sf(y=None) == -1 and sf(sos=None) == -1
    assert sf(detrend=3) == -1 and sf(detrend=-1) == -1
    assert sf(R=0) == -2 and sf(R=-1) == -2
    assert sf(T=0) == -2 and sf(T=-5) == -2 and sf(T=2 ** 30 + 1, ldx=2 ** 31, ldy=2 ** 31) == -2
    assert sf(ldx=99) == -2 and sf(ldy=99) == -2 and sf(ldx=0) == -2 and sf(ldy=-100) == -2
    assert sf(n=0) == -2 and sf(n=-1) == -2 and sf(n=9) == -2
    he = lambda x=fake, env=other, R=3, T=100, ldx=100, ldy=100, window=128, jump=5.0, eps=1e-6: lib.tqs_hold_envelope(
        x, env, R, T, ldx, ldy, window, jump, eps, None)
    assert he(x=None) == -1 and he(env=None) == -1 and he(env=fake) == -1
    assert he(jump=float("nan")) == -1 and he(jump=float("inf")) == -1 and he(eps=float("nan")) == -1
    assert he(R=0) == -2 and he(R=-1) == -2 and he(T=0) == -2 and he(T=2 ** 30 + 1, ldx=2 ** 31, ldy=2 ** 31) == -2
    assert he(ldx=99) == -2 and he(ldy=99) == -2
    assert he(window=0) == -2 and he(window=-1) == -2


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from tqdne_amd import _build, _lib_series
    monkeypatch.setattr(_lib_series, "_LIB", None)
    monkeypatch.setattr(_build, "SERIES_LIBPATH", str(tmp_path / "libtqdne_series.so"))
    with pytest.raises(RuntimeError, match="libtqdne_series.so is missing"):
        _lib_series.load()


# ---- designs ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order,Wn,btype", [(4, 0.002, "high"), (4, (0.002, 0.6), "band"), (8, (0.002, 0.6), "band"), (2, 0.3, "low"),
                                            (1, 0.5, "highpass")])
def test_butter_sos_is_scipys_table(order, Wn, btype):
    from tqdne_amd import conditioning as C
    want = scipy.signal.butter(order, Wn, btype=btype, output="sos")
    got = C.butter_sos(order, Wn, btype)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    got[0, 0] = 123.0   # a copy: the cache is not the caller's to change
    assert np.array_equal(C.butter_sos(order, Wn, btype), want)


def test_bandpass_is_obspys_construction():
    from tqdne_amd import conditioning as C
    for corners, n_sections in ((4, 4), (2, 2), (8, 8)):
        design = C._bandpass_design(0.1, 30, 100, corners, False)
        z, p, k = scipy.signal.iirfilter(corners, [0.1 / 50.0, 30 / 50.0], btype="band", ftype="butter", output="zpk")
        want = scipy.signal.zpk2sos(z, p, k)
        assert np.array_equal(C.butter_sos(*design), want) and want.shape == (n_sections, 6)
        assert np.array_equal(R.bandpass_sos(0.1, 30, 100, corners), want)
    # at or above Nyquist: obspy's fall-back to the high-pass, with a warning
    for freqmax in (50.0, 60.0, 50.0 - 1e-5):
        with pytest.warns(UserWarning, match="Nyquist"):
            design = C._bandpass_design(0.1, freqmax, 100, 4, False)
        z, p, k = scipy.signal.iirfilter(4, 0.1 / 50.0, btype="highpass", ftype="butter", output="zpk")
        assert np.array_equal(C.butter_sos(*design), scipy.signal.zpk2sos(z, p, k))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        C._bandpass_design(0.1, 49.0, 100, 4, False)
    with pytest.raises(ValueError, match="Nyquist"):
        C._bandpass_design(51.0, 60.0, 100, 4, False)


# ---- host paths: the reference's arithmetic, bit for bit -------------------------------------------------------------

def test_host_highpass_is_lfilter_of_the_transfer_function_row_by_row():
    from tqdne_amd import conditioning as C
    b, a = scipy.signal.butter(4, 0.1 / (0.5 * 100), btype="high")
    for dtype in (np.float32, np.float64):
        x = R.make_series(6, 500, seed=3).reshape(2, 3, 500).astype(dtype)
        want = np.zeros_like(x)
        for i in range(2):
            for j in range(3):
                want[i, j] = scipy.signal.lfilter(b, a, x[i, j])
        got = C.highpass_filter(x)
        assert got.dtype == dtype and np.array_equal(got, want)
        t = C.highpass_filter(torch.from_numpy(x))
        assert isinstance(t, torch.Tensor) and not t.is_cuda and np.array_equal(t.numpy(), want)
    b, a = scipy.signal.butter(4, 0.5 / 25.0, btype="high")
    assert np.array_equal(C.highpass_filter(x, cutoff_freq=0.5, sampling_rate=50), scipy.signal.lfilter(b, a, x, axis=-1))
    assert np.array_equal(R.highpass_ba64(x), scipy.signal.lfilter(*scipy.signal.butter(4, 0.002, btype="high"), x, axis=-1))


def test_host_bandpass_detrend_and_chain_are_scipys():
    from tqdne_amd import conditioning as C
    x = R.make_series(6, 700, seed=5).reshape(2, 3, 700)
    sos = R.bandpass_sos(0.1, 30, 100)
    assert np.array_equal(C.bandpass(x, 0.1, 30, 100), scipy.signal.sosfilt(sos, x, axis=-1))
    assert np.array_equal(C.bandpass(x[0, 0], 0.1, 30, 100), scipy.signal.sosfilt(sos, x[0, 0]))
    assert np.array_equal(C.sosfilt(sos, x), scipy.signal.sosfilt(sos, x, axis=-1))
    x64 = x.astype(np.float64)
    dm = scipy.signal.detrend(x64, axis=-1, type="constant")
    dl = scipy.signal.detrend(dm, axis=-1, type="linear")
    assert np.array_equal(C.detrend(x, "demean"), dm) and np.array_equal(C.detrend(x, "constant"), dm)
    assert np.array_equal(C.detrend(x), dl) and np.array_equal(C.detrend(x, type="linear"), dl)
    assert np.array_equal(C.condition_stream(x), scipy.signal.sosfilt(sos, dl, axis=-1))
    assert np.array_equal(C.sosfilt(sos, x, detrend="linear"), C.condition_stream(x, df=100, freqmin=0.1, freqmax=30))
    assert np.array_equal(C.sosfilt(sos, x, detrend="demean"), R.sosfilt64(sos, x, "demean"))
    assert np.array_equal(R.sosfilt64(sos, x, "linear"), C.condition_stream(x)) and np.array_equal(R.detrend64(x, None), x64)
    t = C.condition_stream(torch.from_numpy(x))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and np.array_equal(t.numpy(), C.condition_stream(x))
    # a table whose a0 is not 1 is normalised
    assert np.array_equal(C.sosfilt(2.0 * sos[:1], x), scipy.signal.sosfilt(sos[:1], x, axis=-1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("window", [1, 16, 128, 5000])
def test_host_envelope_and_the_restatement_equal_the_literal_recurrence(dtype, window):
    from tqdne_amd import conditioning as C
    x = R.make_series(4, 300, seed=7, offset=False).astype(dtype)
    x[1, ::7] *= 30.0   # more jumps
    x[2] = 1.0 + 0.1 * np.sin(np.arange(300))   # none
    want = R.envelope_literal(x, window, 1e-6)
    got = C.moving_average_envelope_adaptive(x, window_size=window)
    assert got.dtype == want.dtype == dtype and np.array_equal(got, want)
    assert np.array_equal(C.moving_average_envelope_adaptive(x.reshape(2, 2, 300), window, 1e-3), R.envelope_literal(x, window, 1e-3).reshape(2, 2, 300))
    t = C.moving_average_envelope_adaptive(torch.from_numpy(x), window)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), want)
    # the restatement: float32 decisions, float64 values
    env64, jumps = R.hold_envelope(x, window, 1e-6)
    lit64 = R.envelope_literal(x.astype(np.float32).astype(np.float64), window, 1e-6)
    assert jumps[1].sum() > 10 and not jumps[2].any() and not jumps[:, 0].any()
    if dtype == np.float32:
        assert np.array_equal(jumps[:, 1:], x[:, 1:].__abs__() > 5 * np.abs(x[:, :-1]))
        assert R.jump_margin_ulps(x) > 4   # else the float64 literal loop below could decide differently
    assert np.array_equal(env64, lit64)
    assert np.array_equal(np.diff(env64, axis=-1) != 0, jumps[:, 1:] & (np.diff(env64, axis=-1) != 0))   # a change only at a jump


def test_envelope_first_sample_and_single_sample():
    from tqdne_amd import conditioning as C
    x = np.array([[-3.0], [0.5]], np.float32)
    assert np.array_equal(C.moving_average_envelope_adaptive(x), np.abs(x) + 1e-6)
    assert np.array_equal(R.hold_envelope(x, 128, 1e-6)[0], np.abs(x).astype(np.float64) + 1e-6)
    y = np.array([1.0, 6.0, 6.0, 31.0], np.float64)   # jumps at 1 and 3
    assert np.array_equal(C.moving_average_envelope_adaptive(y, 2, 0.0), [1.0, 3.5, 3.5, 18.5])
    assert np.array_equal(C.moving_average_envelope_adaptive(y, 128, 0.0), [1.0, 3.5, 3.5, 11.0])


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sos_name", ["highpass", "bandpass", "one", "eight"])
def test_the_cascade_loop_in_float64_is_scipys_sosfilt(sos_name):
    sos = {"highpass": R.butter_sos(4, R.HIGHPASS_WN, "high"), "bandpass": R.bandpass_sos(0.1, 30, 100),
           "one": R.butter_sos(2, 0.1, "low"), "eight": R.butter_sos(8, (0.002, 0.6), "band")}[sos_name]
    x = R.make_series(3, 600, seed=11).astype(np.float64)
    assert np.array_equal(R.cascade(sos, x, np.float64), scipy.signal.sosfilt(sos, x, axis=-1))
    assert R.cascade(sos, x[0], np.float64).shape == (1, 600)


def test_long_double_is_wider_and_float64_is_close_to_it():
    """the figures the GPU tests' slack rests on: float64 sosfilt within 1e-12 of the peak of the long-double cascade, the
    transfer-function form orders of magnitude further"""
    assert np.finfo(np.longdouble).eps < 1e-18
    x = R.make_series(6, 4064, seed=13, offset=False)
    for sos in (R.butter_sos(4, R.HIGHPASS_WN, "high"), R.bandpass_sos(0.1, 30, 100)):
        ld = R.cascade(sos, x)
        d = float((np.abs(R.sosfilt64(sos, x) - ld).max(-1) / np.abs(ld).max(-1)).max())
        print(f"float64 sosfilt to long double, of the peak: {d:.2e}")
        assert d <= 1e-12
    ld = R.cascade(R.butter_sos(4, R.HIGHPASS_WN, "high"), x)
    d_ba = float((np.abs(R.highpass_ba64(x) - ld).max(-1) / np.abs(ld).max(-1)).max())
    print(f"float64 lfilter(b, a) to long double, of the peak: {d_ba:.2e}")
    assert 1e-12 < d_ba < 1e-5


# ---- the Python surface -----------------------------------------------------------------------------------------------

def test_function_surface():
    import tqdne_amd
    from tqdne_amd import conditioning as C
    for name in ("sosfilt", "butter_sos", "highpass_filter", "bandpass", "detrend", "condition_stream", "moving_average_envelope_adaptive"):
        assert getattr(tqdne_amd, name) is getattr(C, name) and name in tqdne_amd.__all__ and name in C.__all__
    assert tqdne_amd.conditioning is C and "conditioning" in tqdne_amd.__all__
    assert str(inspect.signature(C.highpass_filter)) == "(data, cutoff_freq=0.1, sampling_rate=100)"
    assert str(inspect.signature(C.moving_average_envelope_adaptive)) == "(waveform, window_size: 'int' = 128, log_eps: 'float' = 1e-06)"
    assert str(inspect.signature(C.bandpass)) == "(data, freqmin, freqmax, df, corners=4, zerophase=False)"
    assert str(inspect.signature(C.condition_stream)) == "(data, df=100, freqmin=0.1, freqmax=30)"
    assert str(inspect.signature(C.sosfilt)) == "(sos, x, detrend=None)"
    assert str(inspect.signature(C.detrend)) == "(data, type='linear')"
    assert str(inspect.signature(C.butter_sos)) == "(order, Wn, btype)"


def test_refusals():
    from tqdne_amd import conditioning as C
    x = np.zeros((2, 3, 64), np.float32)
    with pytest.raises(NotImplementedError, match="zerophase"):
        C.bandpass(x, 0.1, 30, 100, zerophase=True)
    nine = np.tile(R.butter_sos(2, 0.1, "low"), (9, 1))
    with pytest.raises(ValueError, match="at most 8 sections"):
        C.sosfilt(nine, x)
    with pytest.raises(ValueError, match="at most 8 sections"):
        C.bandpass(x, 0.1, 30, 100, corners=9)
    assert C.sosfilt(nine[:8], x).shape == x.shape
    for name in ("quadratic", "", "Linear", 1, 2.0):
        with pytest.raises(ValueError, match="detrend"):
            C.sosfilt(nine[:1], x, detrend=name)
        with pytest.raises(ValueError, match="detrend"):
            C.detrend(x, name)
    with pytest.raises(ValueError, match="type = None"):
        C.detrend(x, None)
    for sos in (np.zeros(6), np.zeros((2, 5)), np.zeros((0, 6)), np.full((1, 6), np.nan), [[1, 0, 0, 0, 0, 0]]):
        with pytest.raises(ValueError, match="sos"):
            C.sosfilt(sos, x)
    for bad in (np.float32(1.0), np.zeros((3, 0), np.float32)):
        for call in (lambda: C.sosfilt(nine[:1], bad), lambda: C.highpass_filter(bad), lambda: C.bandpass(bad, 0.1, 30, 100),
                     lambda: C.detrend(bad), lambda: C.condition_stream(bad), lambda: C.moving_average_envelope_adaptive(bad)):
            with pytest.raises(ValueError, match=r"T >= 1"):
                call()
    with pytest.raises(ValueError, match=r"\(n, C, T\)"):
        C.highpass_filter(np.zeros((3, 64), np.float32))
    for w in (0, -1, 1.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="window_size"):
            C.moving_average_envelope_adaptive(x, w)
    with pytest.raises(ValueError, match="log_eps"):
        C.moving_average_envelope_adaptive(x, 128, float("nan"))
