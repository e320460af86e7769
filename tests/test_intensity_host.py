"""Ground-motion intensity measures without a GPU: the float64 restatement (tests/_intensity_ref.py) against scipy.signal.lsim, the
rotation identity behind the GMRotD form, the device-side percentile against numpy's, the host tables of csrc/intensity.hip, every
argument check, and that the entry points are declared, bound and exported.  smtk is not installed anywhere this suite runs: its semantics are
restated, and scipy is the independent witness."""

import os
import re

import numpy as np
import pytest
import torch

import _intensity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tq_oscillator_table_floats", "tq_oscillator_tables", "tq_rotd_peaks"]
DT, T_REAL = 0.01, 4064


def test_restatement_matches_lsim():
    """lsim(interp=True) is exact for piecewise-linear input; measured 3e-13 of the peak at 5 and 10 s, 1e-14 and below elsewhere"""
    ss = pytest.importorskip("scipy.signal")
    x, _ = R.make_waveforms(3, T_REAL)
    a = x[0].astype(np.float64)
    resp = R.nigam_jennings(a, DT, R.PERIODS7)
    assert resp.shape == (7, T_REAL - 1)
    t = np.arange(T_REAL) * DT
    for i, Tp in enumerate(R.PERIODS7):
        w, xi = 2.0 * np.pi / Tp, 0.05
        sys_ = ss.StateSpace([[0.0, 1.0], [-w * w, -2.0 * xi * w]], [[0.0], [-1.0]], [[-w * w, -2.0 * xi * w]], [[0.0]])
        _, yo, _ = ss.lsim(sys_, a, t, interp=True)
        e = float(np.abs(yo[1:] - resp[i]).max() / np.abs(yo).max())
        print(f"period {Tp}: restatement vs lsim {e:.1e} of the peak")
        assert e <= 1e-11
    assert np.array_equal(R.response_spectrum(a, DT, R.PERIODS7), np.abs(resp).max(-1))


def test_ground_series_are_scipys_cumulative_trapezoids():
    si = pytest.importorskip("scipy.integrate")
    x, _ = R.make_waveforms(2, 257)
    a = x.astype(np.float64)
    g = R.ground_series(a, DT)
    v = DT * si.cumulative_trapezoid(a[:, :-1], initial=0.0)
    d = DT * si.cumulative_trapezoid(v, initial=0.0)
    assert g.shape == (2, 3, 256) and np.array_equal(g[:, 0], a[:, :-1])
    assert np.abs(g[:, 1] - v).max() <= 1e-14 * np.abs(v).max() and np.abs(g[:, 2] - d).max() <= 1e-14 * np.abs(d).max()


def test_rotation_identity_behind_the_gmrotd_form():
    """smtk's second rotated component at theta is the first at theta + 90: max|rot_y|(theta) = m[theta + 90], and so
    sqrt(max|rot_x| max|rot_y|) = sqrt(m[theta] m[theta + 90])"""
    x, y = R.make_waveforms(3, 257)
    sx, sy = R.series(x, DT, R.PERIODS7), R.series(y, DT, R.PERIODS7)
    m = R.directional_peaks(sx, sy)
    assert m.shape == (3, 10, 180)
    assert np.array_equal(m[..., 0], np.abs(sx).max(-1)) and np.array_equal(m[..., 90], np.abs(sy).max(-1))   # unrotated, exactly
    top = m.max(-1)
    for theta in (0, 1, 17, 45, 89):
        rx, ry = R.rotate_literal(sx, sy, float(theta))
        assert (np.abs(np.abs(rx).max(-1) - m[..., theta]) <= 1e-14 * top).all()
        assert (np.abs(np.abs(ry).max(-1) - m[..., theta + 90]) <= 1e-14 * top).all()
    g = R.combine(m, 50, "gmrotd")
    lit = np.stack([np.sqrt(np.abs(rx).max(-1) * np.abs(ry).max(-1)) for rx, ry in (R.rotate_literal(sx, sy, float(t)) for t in range(90))], -1)
    assert np.abs(g - np.percentile(lit, 50, axis=-1)).max() <= 1e-13 * top.max()
    assert (m[2, :, 135] <= 1e-14 * top[2]).all()   # x = y: nothing left at 135 degrees


def test_device_percentile_is_numpys():
    from tqdne_amd.ground_motion import _percentile
    v = np.random.default_rng(0).random((4, 7, 90))
    for n in (90, 180, 1, 2):
        w = np.concatenate([v, v[::-1]], -1)[..., :n]
        for q in (0, 16, 50, 84, 100, 33.3, 99.9):
            got = _percentile(torch.from_numpy(w), q).numpy()
            assert np.abs(got - np.percentile(w, q, axis=-1)).max() <= 1e-15, (n, q)
    nan = torch.full((2, 90), float("nan"), dtype=torch.float64)
    assert bool(torch.isnan(_percentile(nan, 50)).all())


def test_host_tables_are_the_float64_values():
    from tqdne_amd import _lib
    from tqdne_amd.ground_motion import oscillator_tables
    lib = _lib.load()
    for per, dt, xi in ((R.PERIODS7, 0.01, 0.05), (R.periods_log(70), 0.005, 0.2), ((0.5,), 0.02, 0.0), ((), 0.01, 0.05)):
        P = len(per)
        n = lib.tq_oscillator_table_floats(P)
        assert n == 360 + 12 * P
        buf = np.full(n + 8, np.nan, np.float32)
        p64 = np.array(per, np.float64)
        assert lib.tq_oscillator_tables(p64.ctypes.data if P else None, P, dt, xi, buf.ctypes.data) == 0
        assert np.isnan(buf[n:]).all() and not np.isnan(buf[:n]).any()
        c, s = R.angle_table(np.float32)
        assert np.array_equal(buf[:180], c) and np.array_equal(buf[180:360], s)
        assert buf[0] == 1.0 and buf[180] == 0.0 and buf[90] == 0.0 and buf[270] == 1.0
        if not P:
            continue
        A, B0, B1 = R.step_matrices(per, dt, xi)
        t = buf[360:n].reshape(P, 12)
        want = np.concatenate([A.reshape(P, 4), B0, B1, np.full((P, 1), 2.0 * xi), np.zeros((P, 3))], -1)
        # fp32 rounding of an O(1) value, plus the cancellation left in either double evaluation (1e-11 of w dt / 2)
        assert (np.abs(t - want) <= 2.0 ** -24 * np.abs(want) + 1e-11).all()
        assert np.array_equal(oscillator_tables(per, dt, xi), buf[:n])
    assert lib.tq_oscillator_table_floats(-1) == 0


def test_c_abi_argument_checks_return_error_codes_without_a_gpu():
    from tqdne_amd import _lib
    lib = _lib.load()
    fake = 0x1000   # never dereferenced: every call below is rejected during validation
    per = np.array([0.1, 1.0], np.float64)
    out = np.zeros(360 + 24, np.float32)
    tab = lambda p=per, P=2, dt=0.01, xi=0.05, o=out: lib.tq_oscillator_tables(None if p is None else p.ctypes.data, P, dt, xi,
                                                                                None if o is None else o.ctypes.data)
    assert tab() == 0
    assert tab(o=None) == -1 and tab(p=None) == -1 and tab(P=-1) == -1
    assert tab(dt=0.0) == -1 and tab(dt=-0.01) == -1 and tab(dt=float("nan")) == -1 and tab(dt=float("inf")) == -1
    assert tab(xi=-0.1) == -1 and tab(xi=1.0) == -1 and tab(xi=float("nan")) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert tab(p=np.array([0.1, bad])) == -1
    pk = lambda x=fake, y=fake, t=fake, o=fake, N=2, T=4064, P=4, dt=0.01: lib.tq_rotd_peaks(x, y, t, o, N, T, P, dt, None)
    assert pk(x=None) == -1 and pk(y=None) == -1 and pk(t=None) == -1 and pk(o=None) == -1
    assert pk(P=-1) == -1 and pk(dt=0.0) == -1 and pk(dt=float("nan")) == -1
    assert pk(T=1) == -2 and pk(T=0) == -2 and pk(N=0) == -2


def test_python_argument_checks_name_the_argument():
    import tqdne_amd
    from tqdne_amd import ground_motion as G
    x = np.zeros((2, 16), np.float32)
    ok = dict(x=x, y=x, dt=0.01, periods=[0.1, 1.0])
    bad = [("y", dict(y=np.zeros((2, 15), np.float32))), ("y", dict(y=np.zeros((3, 16), np.float32))),
           ("T", dict(x=x[:, :1], y=x[:, :1])), ("dt", dict(dt=0.0)), ("dt", dict(dt=-1.0)), ("dt", dict(dt=float("nan"))),
           ("periods", dict(periods=[0.1, 0.0])), ("periods", dict(periods=[-1.0])), ("periods", dict(periods=[float("inf")])),
           ("periods", dict(periods=[float("nan"), 1.0])), ("periods", dict(periods=[[0.1, 1.0]])),
           ("damping", dict(damping=-0.01)), ("damping", dict(damping=1.0)), ("damping", dict(damping=float("nan")))]
    for name, kw in bad:
        with pytest.raises(ValueError, match=name):
            G.rotd_peaks(**{**ok, **kw})
        with pytest.raises(ValueError, match=name):
            G.gmrotdpp_with_pg(**{**ok, **kw})
    for q in (-1.0, 100.5, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            G.gmrotdpp_with_pg(**ok, percentile=q)
        with pytest.raises(ValueError, match="percentile"):
            G.parallel_processing_sa(x, x, 0.01, [1.0], q)
    with pytest.raises(ValueError, match="kind"):
        G.gmrotdpp_with_pg(**ok, kind="geomean")
    with pytest.raises(ValueError, match="T"):
        G.response_spectrum(x[:, :1], 0.01, [1.0])
    with pytest.raises(ValueError, match="periods"):
        G.response_spectrum(x, 0.01, [0.0])
    with pytest.raises(ValueError, match="damping"):
        G.response_spectrum(x, 0.01, [1.0], damping=1.5)
    for name in ("rotd_peaks", "gmrotdpp_with_pg", "response_spectrum", "parallel_processing_sa"):
        assert getattr(tqdne_amd, name) is getattr(G, name) and name in tqdne_amd.__all__


def test_no_gpu_is_refused_by_name():
    """there is no host fallback: host inputs are either computed on a GPU or refused"""
    from tqdne_amd import ground_motion as G
    x = np.zeros((2, 16), np.float32)
    for call in (lambda: G.rotd_peaks(x, x, 0.01, [1.0]), lambda: G.gmrotdpp_with_pg(torch.zeros(2, 16), torch.zeros(2, 16), 0.01, [1.0]),
                 lambda: G.response_spectrum(x, 0.01, [1.0]), lambda: G.parallel_processing_sa(x, x, 0.01, [1.0], 50)):
        if torch.cuda.is_available():
            assert call() is not None
        else:
            with pytest.raises(RuntimeError, match="GPU"):
                call()


def test_entry_points_are_declared_exported_and_bound():
    from tqdne_amd import _build, _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tqdne_hip.h")).read()
    assert lib.tq_abi_version() == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        decl = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, header, re.S | re.M)
        assert decl, f"{name} is not declared in include/tqdne_hip.h"
        assert name in _lib._PROTOS and hasattr(lib, name)
    assert "intensity.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "intensity.hip"))
    assert not hasattr(lib, "tq_rotd_max_samples")   # the kernel walks the time axis: it has no limit on T to ask for
