"""Host-side checks of the duration library libtqdne_duration.so (include/tqdne_duration.h, tqdne_amd/_lib_duration.py,
csrc_duration/) and of tqdne_amd/duration.py: the C surface held against its three hand-written statements (the shape of
test_conditioning_host.py), every argument check without a device, the float64 restatement (tests/_duration_ref.py) against scipy and
numpy, the host path of every public function against the reference's own results (tests/golden/duration.npz, written by
tools/make_duration_goldens.py), the time-axis rules and the argument checks of the Python surface."""

import ctypes
import functools
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch
from scipy.integrate import cumulative_trapezoid

import _duration_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ABI = 1
SURFACE = "tqd_abi_version tqd_arias tqd_gradient tqd_max_fractions".split()
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "int64_t": ctypes.c_int64}
SIZES = (257, 1000, 4064)


@functools.lru_cache(None)
def _built():
    """(binding module, loaded library, header text without comments)"""
    from tqdne_amd import _build, _lib_duration
    _build.build(verbose=False)
    header = open(os.path.join(ROOT, "include", "tqdne_duration.h")).read()
    return _lib_duration, _lib_duration.load(), re.sub(r"/\*.*?\*/", "", header, flags=re.S)


@functools.lru_cache(None)
def _header_prototypes():
    protos = {}
    for res, name, params in re.findall(r"^(\w+)\s+(tqd_\w+)\s*\((.*?)\)\s*;", _built()[2], re.S | re.M):
        assert name not in protos, name
        params = " ".join(params.split())
        protos[name] = (res, [] if params == "void" else [p.strip() for p in params.split(",")])
    return protos


@functools.lru_cache(None)
def _fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "duration.npz"), allow_pickle=False)
    fx = {k: z[k] for k in z.files}
    for v in fx.values():
        v.setflags(write=False)
    return fx


# ---- the C surface ------------------------------------------------------------------------------------------------

def test_the_surface_is_the_list_in_the_header_the_binding_the_library_and_the_sources():
    from tqdne_amd import _build, _lib, _lib_eval, _lib_series
    L, lib, header = _built()
    assert SURFACE == sorted(set(SURFACE)) and len(SURFACE) == 4
    assert re.search(r"^#define TQD_ABI_VERSION %d$" % ABI, header, re.M) and L.ABI_VERSION == ABI and lib.tqd_abi_version() == ABI
    assert set(_header_prototypes()) == set(SURFACE)
    assert set(L._PROTOS) == set(SURFACE) == set(L.exported_symbols())
    assert [n for n in SURFACE if not hasattr(lib, n)] == []
    defined = []
    paths = sorted(glob.glob(os.path.join(ROOT, "tqdne_amd", "csrc_duration", "*")))
    assert [os.path.basename(p) for p in paths] == sorted(_build.DURATION_SOURCES) == ["duration.hip"]
    for path in paths:
        text = open(path).read()
        found = re.findall(r'extern "C"\s+int\s+(\w+)\s*\(', text)
        assert len(found) == text.count('extern "C"'), f"{path}: an extern \"C\" this scan does not read"
        defined += found
    assert sorted(set(defined)) == SURFACE
    # four libraries: pairwise disjoint name sets, source lists and paths; the other three keep their name counts
    names = [set(L._PROTOS), set(_lib_series._PROTOS), set(_lib_eval._PROTOS), set(_lib._PROTOS)]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not a & b
    assert all(n.startswith("tqd_") for n in names[0]) and not any(n.startswith("tqd_") for n in names[1] | names[2] | names[3])
    sources = [_build.DURATION_SOURCES, _build.SERIES_SOURCES, _build.EVAL_SOURCES, _build.SOURCES]
    assert len(set(sum(sources, []))) == sum(len(s) for s in sources)
    assert (len(_build.SERIES_SOURCES), len(_build.EVAL_SOURCES), len(_build.SOURCES)) == (1, 1, 18)
    assert len({_build.DURATION_LIBPATH, _build.SERIES_LIBPATH, _build.EVAL_LIBPATH, _build.LIBPATH}) == 4
    assert os.path.basename(_build.DURATION_LIBPATH) == "libtqdne_duration.so" and L.lib_path() == _build.DURATION_LIBPATH


def test_the_other_three_libraries_keep_their_name_counts():
    """96, 7 and 4 names, the counts their own pins state (test_abi_host.py, test_spectra_host.py, test_conditioning_host.py); none of
    them exports a name of the fourth"""
    from tqdne_amd import _lib, _lib_eval, _lib_series
    _built()
    for mod, count in ((_lib, 96), (_lib_eval, 7), (_lib_series, 4)):
        loaded = mod.load()
        assert len(mod._PROTOS) == count == len(mod.exported_symbols())
        assert [n for n in mod._PROTOS if not hasattr(loaded, n)] == []
        assert not any(hasattr(loaded, n) for n in SURFACE)


def test_build_returns_the_model_library_and_leaves_all_four_fresh():
    from tqdne_amd import _build
    _built()
    assert _build.build(verbose=False) == _build.LIBPATH
    assert not _build.needs_build() and not _build.eval_needs_build() and not _build.series_needs_build()
    assert not _build.duration_needs_build()
    for path in (_build.LIBPATH, _build.EVAL_LIBPATH, _build.SERIES_LIBPATH, _build.DURATION_LIBPATH):
        assert os.path.exists(path)
    assert os.path.basename(_build.CSRC_DURATION) == "csrc_duration"


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
    for name, expr in re.findall(r"^#define\s+(TQD?_\w+)[ \t]+(\S.*)$", header, re.M):
        consts[name] = eval(expr, {"__builtins__": {}}, dict(consts))
    assert consts["TQ_ERR_ARG"] == -1 and consts["TQ_ERR_SHAPE"] == -2 and consts["TQD_MAX_FRACTIONS"] == 8
    bound = {n: v for n, v in vars(L).items() if n.startswith(("TQ_", "TQD_"))}
    assert {"TQ_ERR_ARG", "TQ_ERR_SHAPE", "TQD_MAX_FRACTIONS"} == set(bound)
    assert {n: v for n, v in bound.items() if consts[n] != v} == {}
    assert lib.tqd_max_fractions() == 8
    from tqdne_amd import duration
    assert duration.max_fractions() == 8


def test_c_abi_argument_checks_return_error_codes_without_a_gpu():
    lib = _built()[1]
    fake, other, third, out = 0x1000, 0x100000, 0x200000, 0x400000   # never dereferenced: every call is rejected in validation
    fr = (ctypes.c_double * 8)(0.05, 0.95, 0.5, 0.0, 1.0, 0.25, 0.75, 0.1)

    def ar(x=fake, y=other, energy=out, peak2=out + 0x1000, index=out + 0x2000, husid=third, R=3, T=100, ldx=100, ldy=100, step=0.01,
           fractions=fr, F=2):
        return lib.tqd_arias(x, y, energy, peak2, index, husid, R, T, ldx, ldy, step, fractions, F, None)

    assert ar(x=None) == -1 and ar(energy=None) == -1 and ar(peak2=None) == -1 and ar(index=None) == -1 and ar(fractions=None) == -1
    assert ar(R=0) == -2 and ar(R=-1) == -2
    assert ar(T=1) == -2 and ar(T=0) == -2 and ar(T=-5) == -2 and ar(T=2 ** 30 + 1, ldx=2 ** 31, ldy=2 ** 31) == -2
    assert ar(ldx=99) == -2 and ar(ldy=99) == -2 and ar(ldx=0) == -2 and ar(ldy=-100) == -2
    assert ar(F=0) == -2 and ar(F=-1) == -2 and ar(F=9) == -2
    for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf"), -float("inf")):
        for F, at in ((1, 0), (8, 7), (3, 1)):
            fb = (ctypes.c_double * 8)(*fr)
            fb[at] = bad
            assert ar(fractions=fb, F=F) == -1, (bad, F, at)
    for step in (0.0, -0.01, float("nan"), float("inf")):
        assert ar(step=step) == -1
    # the Husid rows (R, T) dense must not overlap the spans of x or y
    assert ar(husid=fake) == -1 and ar(husid=other) == -1
    assert ar(husid=fake + 4 * 299) == -1 and ar(husid=fake - 4 * 299) == -1 and ar(husid=other + 4 * 150, y=other) == -1
    assert ar(husid=fake + 4 * 299, ldx=300, y=None) == -1   # inside the strided span of x
    g = lambda x=fake, out=other, R=3, T=100, ldx=100, ldg=100, dt=0.01: lib.tqd_gradient(x, out, R, T, ldx, ldg, dt, None)
    assert g(x=None) == -1 and g(out=None) == -1
    assert g(out=fake) == -1 and g(out=fake + 4 * 299) == -1 and g(out=fake - 4 * 299) == -1
    for dt in (0.0, -0.01, float("nan"), float("inf")):
        assert g(dt=dt) == -1
    assert g(R=0) == -2 and g(R=-1) == -2 and g(T=1) == -2 and g(T=0) == -2 and g(T=2 ** 30 + 1, ldx=2 ** 31, ldg=2 ** 31) == -2
    assert g(ldx=99) == -2 and g(ldg=99) == -2


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from tqdne_amd import _build, _lib_duration
    monkeypatch.setattr(_lib_duration, "_LIB", None)
    monkeypatch.setattr(_build, "DURATION_LIBPATH", str(tmp_path / "libtqdne_duration.so"))
    with pytest.raises(RuntimeError, match="libtqdne_duration.so is missing"):
        _lib_duration.load()


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [2, 3, 65, 1000])
def test_the_recurrence_in_float64_is_scipys_cumulative_trapezoid_and_numpys_gradient(T):
    x, y = R.make_pairs(5, T, seed=3)
    step = 0.01 * T / (T - 1)
    for yy in (None, y):
        s = R.squares(x, yy)
        want = cumulative_trapezoid(s, dx=step, initial=0)
        cum = R.cumulative(x, yy, step)
        assert cum.dtype == np.float64 and cum.shape == (5, T) and np.array_equal(cum, want)
        assert (np.diff(cum, axis=-1) >= 0).all() and (cum[:, 0] == 0).all()
        # the exactly rounded total: the recurrence is within (T - 2) half-ulps-of-the-result steps of it
        exact = R.exact_total(x, yy, step)
        assert (np.abs(cum[:, -1] - exact) <= (T + 8) * 2.0 ** -53 * exact).all()
        assert np.array_equal(R.husid(cum)[:, -1], np.ones(5))
    g = R.gradient(x, 0.01)
    assert np.array_equal(g, np.gradient(x.astype(np.float64), float(np.float32(0.01)), axis=-1))
    # numpy's own float32 result: three roundings away at most
    g32 = np.gradient(x, 0.01, axis=-1)
    assert g32.dtype == np.float32 and (np.abs(g32 - g) <= 4 * 2.0 ** -24 * np.abs(g) + 1e-37).all()


def test_first_crossing_rule_and_margin():
    cum = np.array([[0.0, 1.0, 1.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 1.0, np.nan, np.nan, np.nan]])
    got = R.crossings(cum, [0.0, 0.25, 0.26, 0.75, 1.0, 0.5])
    assert np.array_equal(got, [[0, 1, 3, 3, 4, 3], [-1] * 6, [-1] * 6])
    assert R.crossing_margin(cum[:1], [0.5]) == pytest.approx(0.25)   # cum[3] = 3 and cum[2] = 1 around the threshold 2
    assert R.crossing_margin(cum[:1], [0.0, 1.0]) == np.inf


# ---- host paths against the reference's own results --------------------------------------------------------------------

def _close(got, want, rtol=1e-6):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool((np.abs(got - want) <= rtol * np.abs(want)).all())


@pytest.mark.parametrize("T", SIZES)
def test_host_path_of_every_function_is_the_references(T):
    from tqdne_amd import duration as D
    fx = _fx()
    w, time = fx[f"w{T}"], fx[f"time{T}"]
    assert np.array_equal(time, np.linspace(0, 0.01 * T, T)) and w.dtype == np.float32
    acc = D.calculate_resultant_horizontal(w[:, 1], w[:, 0])
    assert acc.dtype == np.float32
    if T == 257:
        assert np.array_equal(acc, fx["resultant257"])
    norm = acc / np.abs(acc).max(-1, keepdims=True)
    percents = [tuple(p) for p in fx["percents"]]
    for tag, rows in (("raw", acc), ("norm", norm)):
        Ia, cum = D.calculate_arias_intensity(time, rows)            # batched
        assert _close(Ia, fx[f"{tag}_Ia{T}"]) and cum.shape == rows.shape
        if f"{tag}_cum{T}" in fx:
            assert _close(cum, fx[f"{tag}_cum{T}"])
        for k, (lo, hi) in enumerate(percents):
            want = fx[f"{tag}_dur{T}"][:, k]
            got = D.calculate_signal_duration(time, cum, Ia, lower_percent=lo, upper_percent=hi)
            assert np.array_equal(np.stack(got, -1)[:, :2], time[fx[f"{tag}_idx{T}"][:, k]])   # the indices, exactly
            assert _close(np.stack(got, -1), want)
            fused = D.significant_duration(w[:, 1], w[:, 0], time=time, lower_percent=lo, upper_percent=hi, normalize=tag == "norm")
            assert _close(fused[0], fx[f"{tag}_Ia{T}"]) and np.array_equal(np.stack(fused[1:], -1), np.stack(got, -1))
        # one row at a time, as the notebook calls them: scalars out
        ia0, cum0 = D.calculate_arias_intensity(time, rows[0])
        assert np.ndim(ia0) == 0 and ia0 == Ia[0] and np.array_equal(cum0, cum[0])
        one = D.calculate_signal_duration(time, cum0, ia0)
        assert all(np.ndim(v) == 0 for v in one) and _close(one, fx[f"{tag}_dur{T}"][0, 0])
    # one component
    single = D.significant_duration(w[0, 0], time=time)
    assert _close(single[0], fx[f"single_Ia{T}"]) and _close(single[1:], fx[f"single_dur{T}"])
    # the notebook's loop for two sets
    a, b = D.shaking_duration(w, w[::-1])
    assert isinstance(a, np.ndarray) and _close(a, fx[f"norm_dur{T}"][:, 0, 2]) and np.array_equal(b, a[::-1])
    c, _ = D.shaking_duration(w, w, lower_percent=20, upper_percent=75)
    assert _close(c, fx[f"norm_dur{T}"][:, 1, 2])
    # the Husid curve: the cumulative curve over its last value
    if f"raw_cum{T}" in fx:
        h = D.husid(w[:, 1], w[:, 0], time=time)
        assert _close(h, fx[f"raw_cum{T}"] / fx[f"raw_cum{T}"][:, -1:]) and (h[:, -1] == 1).all() and (h[:, 0] == 0).all()
    # CPU tensors: the same values in tensors
    t = D.significant_duration(torch.from_numpy(np.array(w[:, 1])), torch.from_numpy(np.array(w[:, 0])), time=time)
    want = D.significant_duration(w[:, 1], w[:, 0], time=time)
    assert all(isinstance(v, torch.Tensor) and not v.is_cuda for v in t)
    assert all(np.array_equal(v.numpy(), u) for v, u in zip(t, want))


def test_host_gradient_is_numpys():
    from tqdne_amd import duration as D
    fx = _fx()
    w = fx["w257"]
    g = D.compute_time_derivative(w)
    assert g.dtype == np.float32 and np.array_equal(g, fx["gradient257"]) and np.array_equal(g, np.gradient(w, 0.01, axis=-1))
    assert np.array_equal(D.compute_time_derivative(w, sampling_rate=50), fx["gradient50_257"])
    t = D.compute_time_derivative(torch.from_numpy(np.array(w)))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and np.array_equal(t.numpy(), g)
    assert np.array_equal(D.compute_time_derivative(w[0, 0]), g[0, 0])
    assert (np.abs(g - R.gradient(w, 0.01)) <= 4 * 2.0 ** -24 * np.abs(R.gradient(w, 0.01)) + 1e-37).all()


def test_the_restatement_agrees_with_the_reference_on_the_fixture():
    """the float64 evaluation against the reference's float32 intermediates: totals to 1e-6, every crossing identical, each crossing
    at least 1e-6 of the total away from its threshold on both sides"""
    fx = _fx()
    fracs = [p / 100 for p in fx["percents"].ravel()]
    for T in SIZES:
        w, time = fx[f"w{T}"], fx[f"time{T}"]
        step = (time[-1] - time[0]) / (T - 1)
        cum = R.cumulative(w[:, 1], w[:, 0], step)
        assert R.crossing_margin(cum, fracs) >= 1e-6
        assert _close(np.pi / (2 * 9.81) * cum[:, -1], fx[f"raw_Ia{T}"])
        assert np.array_equal(R.crossings(cum, fracs).reshape(-1, 2, 2), fx[f"raw_idx{T}"])
        assert np.array_equal(fx[f"norm_idx{T}"], fx[f"raw_idx{T}"])
        peak2 = R.squares(w[:, 1], w[:, 0]).max(-1)
        assert _close(np.pi / (2 * 9.81) * cum[:, -1] / peak2, fx[f"norm_Ia{T}"])


# ---- the time axis ----------------------------------------------------------------------------------------------------

def test_time_axis_rules():
    from tqdne_amd import duration as D
    T = 257
    x, y = R.make_pairs(3, T, seed=5)
    lin = np.linspace(0, 0.01 * T, T)
    t, t0, step = D._axis(lin, None, T, True)
    assert t0 == 0.0 and step == pytest.approx(0.01 * T / (T - 1), rel=1e-15) and step != 0.01 and t is not None
    assert D._axis(None, 0.01, T, True) == (None, 0.0, 0.01)
    assert D._axis(lin + 3.5, None, T, True)[1:] == (3.5, pytest.approx(step, rel=1e-12))
    assert D._axis(torch.from_numpy(lin), None, T, True)[1:] == (0.0, step)
    # dt: t0 = 0 and step = dt; a uniform time array gives the same result as its step, shifted by its start
    a = D.significant_duration(x, y, dt=0.02)
    b = D.significant_duration(x, y, time=7.0 + 0.02 * np.arange(T))
    assert _close(a[0], b[0], 1e-12) and _close(np.asarray(b[1]) - 7.0, a[1], 1e-9) and _close(a[3], b[3], 1e-9)
    # the GPU route's uniformity rule; the host path keeps scipy's general rule
    bent = lin.copy()
    bent[100] += 1e-8 * step * 2
    for bad in (bent, lin[::-1].copy(), np.zeros(T), np.where(np.arange(T) == 5, np.nan, lin)):
        with pytest.raises(ValueError, match="uniform"):
            D._axis(bad, None, T, True)
    assert D._axis(bent, None, T, False)[0] is not None
    warped = np.cumsum(np.linspace(0.005, 0.02, T))
    Ia, cum = D.calculate_arias_intensity(warped, x)
    assert np.array_equal(cum, np.pi / (2 * 9.81) * cumulative_trapezoid(x ** 2, warped, initial=0))
    got = D.significant_duration(x, time=warped)
    assert np.array_equal(got[0], Ia) and np.isin(got[1], warped).all()
    almost = lin.copy()
    almost[100] += 1e-10 * step
    assert D._axis(almost, None, T, True)[2] == step
    # exactly one of time and dt, and a time array of the series' length
    for kw in ({}, {"time": lin, "dt": 0.01}):
        with pytest.raises(ValueError, match="exactly one"):
            D.significant_duration(x, y, **kw)
        with pytest.raises(ValueError, match="exactly one"):
            D.husid(x, **kw)
    for bad in (lin[:-1], lin.reshape(1, T), 0.01):
        with pytest.raises(ValueError, match="time"):
            D.significant_duration(x, time=bad)
        with pytest.raises(ValueError, match="time"):
            D.calculate_arias_intensity(bad, x)
        with pytest.raises(ValueError, match="time"):
            D.calculate_signal_duration(bad, np.zeros((3, T)), np.ones(3))


# ---- the Python surface -----------------------------------------------------------------------------------------------

def test_function_surface():
    import tqdne_amd
    from tqdne_amd import duration as D
    for name in ("compute_time_derivative", "calculate_resultant_horizontal", "calculate_arias_intensity", "calculate_signal_duration",
                 "significant_duration", "husid", "shaking_duration"):
        assert getattr(tqdne_amd, name) is getattr(D, name) and name in tqdne_amd.__all__ and name in D.__all__
    assert tqdne_amd.duration is D and "duration" in tqdne_amd.__all__ and "max_fractions" in D.__all__
    assert str(inspect.signature(D.compute_time_derivative)) == "(waveform, sampling_rate=100)"
    assert str(inspect.signature(D.calculate_resultant_horizontal)) == "(acc_x, acc_y)"
    assert str(inspect.signature(D.calculate_arias_intensity)) == "(time, acceleration, gravity=9.81)"
    assert str(inspect.signature(D.calculate_signal_duration)) == "(time, cumulative_arias, arias_intensity, lower_percent=5, upper_percent=95)"
    assert str(inspect.signature(D.significant_duration)) == ("(x, y=None, *, time=None, dt=None, lower_percent=5, upper_percent=95, "
                                                              "normalize=False, gravity=9.81)")
    assert str(inspect.signature(D.husid)) == "(x, y=None, *, time=None, dt=None)"
    assert str(inspect.signature(D.shaking_duration)) == "(target, predicted, dt=0.01, lower_percent=5, upper_percent=95)"


def test_edge_rows_on_the_host_path():
    from tqdne_amd import duration as D
    x = np.array(R.make_pairs(4, 65, seed=9)[0])
    x[1] = 0.0
    x[2, 30] = np.nan
    Ia, t0, t1, d = D.significant_duration(x, dt=0.01)
    assert Ia[1] == 0 and np.isnan(Ia[2]) and np.isfinite(Ia[[0, 3]]).all()
    assert np.isnan(t0[2]) and np.isnan(t1[2]) and np.isnan(d[2]) and np.isfinite(d[[0, 3]]).all()
    assert t0[1] == 0 and t1[1] == 0      # the reference's own answer for a silent row: 0 >= 0 at the first sample
    h = D.husid(x, dt=0.01)
    assert np.isnan(h[1]).all() and np.isnan(h[2, 30:]).all() and (h[[0, 3], -1] == 1).all()


def test_refusals():
    from tqdne_amd import duration as D
    x = np.ones((2, 3, 64), np.float32)
    for bad in (np.float32(1.0), np.zeros((3, 1), np.float32), np.zeros((3, 0), np.float32)):
        for call in (lambda: D.significant_duration(bad, dt=0.01), lambda: D.husid(bad, dt=0.01), lambda: D.compute_time_derivative(bad),
                     lambda: D.calculate_arias_intensity(np.arange(1.0), bad),
                     lambda: D.calculate_signal_duration(np.arange(1.0), bad, 1.0)):
            with pytest.raises(ValueError, match=r"T >= 2"):
                call()
    with pytest.raises(ValueError, match="shapes"):
        D.significant_duration(x[:, 0], x[:1, 1], dt=0.01)
    with pytest.raises(ValueError, match="shapes"):
        D.husid(x[:, 0], x[:, 1, :63], dt=0.01)
    for dt in (0.0, -0.01, float("nan"), float("inf"), True, "0.01"):
        with pytest.raises(ValueError, match="dt"):
            D.significant_duration(x, dt=dt)
        with pytest.raises(ValueError, match="dt"):
            D.shaking_duration(x, x, dt=dt)
    for rate in (0, -100, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="sampling_rate"):
            D.compute_time_derivative(x, rate)
    for g in (0.0, -9.81, float("nan")):
        with pytest.raises(ValueError, match="gravity"):
            D.significant_duration(x, dt=0.01, gravity=g)
        with pytest.raises(ValueError, match="gravity"):
            D.calculate_arias_intensity(np.arange(64.0), x, gravity=g)
    for p in (-1, 100.5, float("nan"), True, None, "5"):
        with pytest.raises(ValueError, match="lower_percent"):
            D.significant_duration(x, dt=0.01, lower_percent=p)
        with pytest.raises(ValueError, match="upper_percent"):
            D.calculate_signal_duration(np.arange(64.0), x, np.ones((2, 3)), upper_percent=p)
        with pytest.raises(ValueError, match="lower_percent"):
            D.shaking_duration(x, x, lower_percent=p)
    for bad in (x[:, 0], x[:, :1], x[0, 0]):
        with pytest.raises(ValueError, match=r"\(n, C, T\)"):
            D.shaking_duration(x, bad)
    assert D.significant_duration(x, dt=0.01, lower_percent=0, upper_percent=100)[3].shape == (2, 3)
