"""The conditioning kernels (csrc_series/series.hip, tqdne_amd/conditioning.py) against the float64 restatement of
tests/_conditioning_ref.py.  tqs_sosfilt and tqs_hold_envelope are called through the C ABI: the input rows are a channel view of a
(R, 3, T + pad) tensor that is NaN elsewhere (row stride 3 (T + pad)), the output rows sit T + 3 apart inside a NaN-filled buffer, and
every NaN outside the rows is checked untouched.  The kernels give one lane to a row and 16 rows to a workgroup (series.hip THREADS),
so R = 3 is a partial workgroup, R = 65 is four workgroups and one row and R = 130 is eight and two: more than a wave's 64 lanes too.

Bar of the filter, element-wise per row:  |y - y64| <= 2^-24 |y64| + 1e-11 max|y64|,  y64 = float64 scipy sosfilt after float64 scipy
detrend.  The first term is the one rounding of the output to fp32.  The second is 100 x the distance between float64 and the exact
cascade (1e-13 of the peak); every sweep case measures that distance on its own inputs with the long-double loop and asserts it is at
most 1e-12, so the slack rests on a number checked in the same run.  Where the exact result is identically zero (T = 1 after any
detrend, T = 2 after the linear one, a pure line) y64 is scipy's own rounding residue, of the order 1e-16 of the INPUT, and says nothing
about the size of the result; there the kernel's output is held to 1e-11 of the input's peak instead.  The envelope is held to the
same form of bar against the float64 recurrence, its decisions to equality with float32's."""

import functools

import numpy as np
import pytest
import torch

import _conditioning_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
G = 1024           # floats of NaN either side of every output
THREADS = 16       # rows per workgroup (series.hip)
PAD, GAP = 5, 3    # input rows: (R, 3, T + PAD) channel 1; output rows T + GAP apart
ROWS = [1, 3, 65, 130]
LENGTHS = [1, 2, 3, 127, 128, 129, 4064]
NONE, DEMEAN, LINEAR = 0, 1, 2
MODES = [(None, NONE), ("demean", DEMEAN), ("linear", LINEAR)]
RND, SLACK = 2.0 ** -24, 1e-11


def _dev():
    return torch.device("cuda:0")


def _lib():
    from tqdne_amd import _lib_series
    return _lib_series.load()


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _sos(name):
    sos = {"highpass": R.butter_sos(4, R.HIGHPASS_WN, "high"), "bandpass": R.bandpass_sos(0.1, 30, 100),
           "one": R.butter_sos(2, 0.05, "high"), "eight": R.butter_sos(8, (0.002, 0.6), "band"),
           "identity": np.array([[1.0, 0, 0, 1, 0, 0]])}[name]
    assert sos.shape == ({"highpass": 2, "bandpass": 4, "one": 1, "eight": 8, "identity": 1}[name], 6)
    return sos


@functools.lru_cache(None)
def _sos_dev(name):
    return torch.from_numpy(np.array(_sos(name))).to(_dev())


def _channel_view(rows):
    """rows (R, T) float32 -> (the (R, 3, T + PAD) tensor, NaN but for channel 1's first T samples; pointer to row 0; row stride)"""
    Rn, T = rows.shape
    big = torch.full((Rn, 3, T + PAD), float("nan"), device=_dev())
    big[:, 1, :T] = torch.from_numpy(np.array(rows)).to(_dev())   # (a copy: the cached series are read-only)
    return big, big.data_ptr() + 4 * (T + PAD), 3 * (T + PAD)


def _check_input_untouched(big, rows):
    Rn, T = rows.shape
    got = big.cpu().numpy()
    assert np.array_equal(got[:, 1, :T], rows, equal_nan=True), "the input was written"
    assert np.isnan(got[:, 0]).all() and np.isnan(got[:, 2]).all() and np.isnan(got[:, 1, T:]).all(), "around the input was written"


def _unguard(buf, Rn, T):
    """the (R, T) rows out of a guarded buffer with rows T + GAP apart; every other float must still be NaN"""
    body = buf[G:G + Rn * (T + GAP)].reshape(Rn, T + GAP)
    assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + Rn * (T + GAP):]).all(), "a guard band was written"
    assert torch.isnan(body[:, T:]).all(), "between the output rows was written"
    return body[:, :T].cpu().numpy()


def _guarded(Rn, T):
    return torch.full((G + Rn * (T + GAP) + G,), float("nan"), device=_dev())


def c_sosfilt(rows, sos_name, mode):
    Rn, T = rows.shape
    big, ptr, ld = _channel_view(rows)
    out = _guarded(Rn, T)
    rc = _lib().tqs_sosfilt(ptr, out.data_ptr() + 4 * G, _sos_dev(sos_name).data_ptr(), Rn, T, ld, T + GAP, len(_sos(sos_name)), mode,
                            _stream())
    assert rc == 0, rc
    y = _unguard(out, Rn, T)
    _check_input_untouched(big, rows)
    return y


def c_envelope(rows, window, jump=5.0, eps=1e-6):
    Rn, T = rows.shape
    big, ptr, ld = _channel_view(rows)
    out = _guarded(Rn, T)
    rc = _lib().tqs_hold_envelope(ptr, out.data_ptr() + 4 * G, Rn, T, ld, T + GAP, window, jump, eps, _stream())
    assert rc == 0, rc
    env = _unguard(out, Rn, T)
    _check_input_untouched(big, rows)
    return env


def _bound(y64):
    return RND * np.abs(y64) + SLACK * np.abs(y64).max(axis=-1, keepdims=True)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(None)
def _series(T):
    x = R.make_series(max(ROWS), T, seed=1)
    x.setflags(write=False)
    return x


def _identically_zero(T, mode):
    return (T == 1 and mode is not None) or (T == 2 and mode == "linear")


# ---- filter sweep -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sos_name", ["highpass", "bandpass", "one", "eight"])
@pytest.mark.parametrize("T", LENGTHS)
def test_filter_sweep_against_float64_sosfilt(T, sos_name):
    x = _series(T)
    sos = _sos(sos_name)
    assert min(ROWS) < THREADS < 64 < max(ROWS) and all(r % THREADS for r in ROWS)
    # float64 against the exact cascade, on this case's own inputs (six rows of every detrend mode)
    det = np.concatenate([R.detrend64(x[:6], name) for name, _ in MODES])
    ld = R.cascade(sos, det)
    peak = np.abs(ld).max(-1)
    dist = float((np.abs(R.sosfilt64(sos, det) - ld).max(-1)[peak > 0] / peak[peak > 0]).max())
    print(f"T={T} {sos_name}: float64 to long double {dist:.2e} of the peak")
    assert np.finfo(np.longdouble).eps < 1e-18 and dist <= 1e-12
    worst = 0.0
    for name, mode in MODES:
        y64 = R.sosfilt64(sos, x, name)
        for Rn in ROWS:
            y = c_sosfilt(x[:Rn], sos_name, mode)
            assert np.isfinite(y).all()
            if _identically_zero(T, name):
                assert (np.abs(y) <= SLACK * np.abs(x[:Rn]).max(-1, keepdims=True)).all()
                continue
            err, bound = np.abs(y - y64[:Rn]), _bound(y64[:Rn])
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (name, Rn, float((err / bound).max()))
    print(f"T={T} {sos_name}: worst error / bound {worst:.3f}")


def test_highpass_against_the_references_transfer_function_form():
    """|y - y_ba| <= |y_ba - y_ld| + bar, per row on the rows' maxima: the triangle inequality through the exact filter y_ld.  The
    reference's float64 lfilter(b, a) is itself about 1e-8 of the peak away from the filter it designs."""
    from tqdne_amd import conditioning as C
    T = 4064
    x = R.make_series(12, T, seed=2, offset=False).reshape(4, 3, T)
    y = C.highpass_filter(torch.from_numpy(x).to(_dev()))
    assert y.is_cuda and y.dtype == torch.float32 and y.shape == (4, 3, T)
    y = y.cpu().numpy().reshape(12, T).astype(np.float64)
    sos = _sos("highpass")
    y_ba, y_ld, y64 = R.highpass_ba64(x.reshape(12, T)), R.cascade(sos, x.reshape(12, T)).astype(np.float64), R.sosfilt64(sos, x.reshape(12, T))
    peak = np.abs(y64).max(-1)
    d_gpu, d_ref, bar = np.abs(y - y_ba).max(-1), np.abs(y_ba - y_ld).max(-1), _bound(y64).max(-1)
    print(f"of the peak: kernel to lfilter(b, a) {float((d_gpu / peak).max()):.2e}, lfilter(b, a) to long double "
          f"{float((d_ref / peak).max()):.2e}, kernel to long double {float((np.abs(y - y_ld).max(-1) / peak).max()):.2e}")
    assert (d_gpu <= d_ref + bar).all()
    assert (np.abs(y - y64) <= _bound(y64)).all()


# ---- detrend ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 2, 129, 4064])
def test_detrend_modes(T):
    from tqdne_amd import conditioning as C
    x = np.array(_series(T)[:5])
    t = np.arange(T, dtype=np.float32)
    x[3] = 10.0 + 0.375 * t        # a line whose samples, sums and slope are exact in float32 / float64
    x[4] = -1534.0                 # a constant
    xg = torch.from_numpy(x).to(_dev())
    for name, mode in MODES:
        y = c_sosfilt(x, "identity", mode)
        if name is None:
            assert np.array_equal(_bits(y), _bits(x))   # one section b0 = 1: the samples themselves
            continue
        assert np.array_equal(_bits(C.detrend(xg, name).cpu().numpy()), _bits(y))
        y64 = R.detrend64(x, name)
        scale = np.abs(x).max(-1, keepdims=True)
        zero = np.array([_identically_zero(T, name), _identically_zero(T, name), _identically_zero(T, name), name == "linear" or T == 1,
                         True])
        assert (np.abs(y[zero]) <= SLACK * scale[zero]).all(), float(np.abs(y[zero]).max())
        assert (np.abs(y - y64)[~zero] <= _bound(y64)[~zero]).all()
    assert np.array_equal(_bits(C.detrend(xg, "constant").cpu().numpy()), _bits(C.detrend(xg, "demean").cpu().numpy()))
    assert np.array_equal(_bits(C.detrend(xg).cpu().numpy()), _bits(C.sosfilt(_sos("identity"), xg, detrend="linear").cpu().numpy()))


# ---- in place, batch independence, non-finite rows ----------------------------------------------------------------------

@pytest.mark.parametrize("T", [3, 129, 4064])
def test_in_place_gives_the_same_bits(T):
    x = _series(T)[:67]
    for sos_name, mode in (("bandpass", LINEAR), ("highpass", NONE)):
        want = c_sosfilt(x, sos_name, mode)
        buf = torch.full((G + 67 * (T + GAP) + G,), float("nan"), device=_dev())
        buf[G:G + 67 * (T + GAP)].reshape(67, T + GAP)[:, :T] = torch.from_numpy(np.array(x)).to(_dev())
        p = buf.data_ptr() + 4 * G
        rc = _lib().tqs_sosfilt(p, p, _sos_dev(sos_name).data_ptr(), 67, T, T + GAP, T + GAP, len(_sos(sos_name)), mode, _stream())
        assert rc == 0
        assert np.array_equal(_bits(_unguard(buf, 67, T)), _bits(want))


def test_a_row_does_not_depend_on_its_batch_and_launches_repeat():
    T = 4064
    x = _series(T)
    for sos_name, mode in (("bandpass", LINEAR), ("eight", DEMEAN)):
        full = c_sosfilt(x, sos_name, mode)
        assert np.array_equal(_bits(c_sosfilt(x, sos_name, mode)), _bits(full))
        for r in (0, 15, 16, 64, 129):
            assert np.array_equal(_bits(c_sosfilt(x[r:r + 1], sos_name, mode)[0]), _bits(full[r]))
    env = c_envelope(x, 128)
    assert np.array_equal(_bits(c_envelope(x, 128)), _bits(env))
    for r in (0, 64, 129):
        assert np.array_equal(_bits(c_envelope(x[r:r + 1], 128)[0]), _bits(env[r]))


@pytest.mark.parametrize("T", [1, 129, 4064])
def test_a_non_finite_row_is_all_nan_and_its_neighbours_are_untouched(T):
    clean = np.array(_series(T)[:9])
    dirty = clean.copy()
    dirty[1, 0], dirty[3, T // 2], dirty[5, T - 1], dirty[7, T // 3] = np.nan, np.nan, np.nan, np.inf
    bad = np.array([False, True, False, True, False, True, False, True, False])
    runs = [lambda a: c_sosfilt(a, "highpass", NONE), lambda a: c_sosfilt(a, "bandpass", LINEAR), lambda a: c_sosfilt(a, "identity", DEMEAN),
            lambda a: c_envelope(a, 128), lambda a: c_envelope(a, 1)]
    for run in runs:
        a, b = run(clean), run(dirty)
        assert np.isfinite(a).all()
        assert np.isnan(b[bad]).all() and np.array_equal(_bits(b[~bad]), _bits(a[~bad]))


# ---- envelope -----------------------------------------------------------------------------------------------------

def _envelope_rows(T, n_noise=4):
    i = np.arange(T)
    steady = 1.0 + 0.1 * np.sin(i)                                 # never above 5 x its predecessor
    dense = 7.0 ** (i % 40) * np.where(i % 2 == 0, 1.0, -1.0)      # 39 jumps in every 40 samples: as dense as float32's range allows
    noise = R.make_series(n_noise, T, seed=3, offset=False)
    return np.concatenate([np.stack([steady, dense]).astype(np.float32), noise])


@pytest.mark.parametrize("window", [1, 128, 5000])
@pytest.mark.parametrize("T", [1, 2, 129, 4064])
def test_envelope_decisions_and_values(T, window):
    x = _envelope_rows(T, 128 if T == 129 else 4)   # (at T = 129: 130 rows)
    assert R.jump_margin_ulps(x) > 4, R.jump_margin_ulps(x)   # no decision within 4 ulp of its threshold
    env64, jumps = R.hold_envelope(x, window, 1e-6)
    if T > 40:
        assert not jumps[0].any() and jumps[1].sum() == (T - 1) - (T - 1) // 40 and jumps[2:].any(-1).all()
    env = c_envelope(x, window)
    assert np.isfinite(env).all()
    changes = lambda e: [np.flatnonzero(np.diff(row) != 0) + 1 for row in e]
    for got, want in zip(changes(env), changes(env64.astype(np.float32))):
        assert np.array_equal(got, want)
    err, bound = np.abs(env - env64), _bound(env64)
    print(f"T={T} window={window}: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


def test_envelope_python_surface_is_the_c_call():
    from tqdne_amd import conditioning as C
    x = _envelope_rows(129).reshape(2, 3, 129)
    xg = torch.from_numpy(x).to(_dev())
    for window, eps in ((128, 1e-6), (7, 1e-3)):
        got = C.moving_average_envelope_adaptive(xg, window, eps)
        assert got.is_cuda and got.shape == xg.shape and got.dtype == torch.float32
        assert np.array_equal(_bits(got.cpu().numpy().reshape(6, 129)), _bits(c_envelope(x.reshape(6, 129), window, 5.0, eps)))


# ---- chain and dispatch -------------------------------------------------------------------------------------------

def test_highpass_feeds_the_intensity_measures():
    from tqdne_amd import conditioning as C, ground_motion as GM
    T, dt, periods = 1000, 0.01, (0.1, 0.3, 1.0, 3.0)
    w = R.make_series(18, T, seed=5).reshape(6, 3, T)
    w2 = 1.5 * R.make_series(18, T, seed=6).reshape(6, 3, T)
    on_gpu = [C.highpass_filter(torch.from_numpy(a).to(_dev())) for a in (w, w2)]
    on_host = [C.highpass_filter(a) for a in (w, w2)]
    assert all(a.is_cuda for a in on_gpu) and all(isinstance(a, np.ndarray) and a.dtype == np.float32 for a in on_host)
    got = GM.gmrotdpp_with_pg(on_gpu[0][:, 0], on_gpu[0][:, 1], dt, periods)
    want = GM.gmrotdpp_with_pg(on_host[0][:, 0], on_host[0][:, 1], dt, periods)
    for k in ("PGA", "PGV", "PGD", "Acceleration"):
        assert got[k].is_cuda and isinstance(want[k], np.ndarray)
        assert rel_err(got[k].cpu().numpy(), want[k]) < 1e-3
    for PGV in (True, False):
        got = GM.evaluate_ratio(on_gpu[0][:, :2], on_gpu[1][:, :2], dt, PGV=PGV)
        want = GM.evaluate_ratio(on_host[0][:, :2], on_host[1][:, :2], dt, PGV=PGV)
        assert sorted(got) == sorted(want)
        for k in want:
            assert rel_err(got[k].cpu().numpy(), want[k]) < 1e-3


def test_dispatch_and_views():
    from tqdne_amd import conditioning as C
    T = 257
    x = R.make_series(12, T, seed=7).reshape(4, 3, T)
    big = torch.full((4, 3, T + PAD), float("nan"), device=_dev())
    big[:, :, :T] = torch.from_numpy(x).to(_dev())
    dense = torch.from_numpy(x).to(_dev())
    sos = np.array(_sos("bandpass"))
    calls = {"highpass_filter": lambda a: C.highpass_filter(a), "bandpass": lambda a: C.bandpass(a, 0.1, 30, 100),
             "detrend": lambda a: C.detrend(a, "linear"), "condition_stream": lambda a: C.condition_stream(a),
             "sosfilt": lambda a: C.sosfilt(sos, a, detrend="demean"), "envelope": lambda a: C.moving_average_envelope_adaptive(a)}
    for name, call in calls.items():
        host = call(x)
        assert isinstance(host, np.ndarray) and host.shape == x.shape, name
        cpu = call(torch.from_numpy(x))
        assert isinstance(cpu, torch.Tensor) and not cpu.is_cuda and np.array_equal(cpu.numpy(), host), name
        gpu = call(dense)
        assert gpu.is_cuda and gpu.dtype == torch.float32 and gpu.shape == x.shape and gpu.is_contiguous(), name
        assert rel_err(gpu.cpu().numpy(), host) < 1e-3, name
        # views: all channels of the padded tensor, one channel of it, one waveform's channel
        for view, same, want_ld in ((big[:, :, :T], gpu, T + PAD), (big[:, 1, :T], gpu[:, 1], 3 * (T + PAD)), (big[2, 0, :T], gpu[2, 0], T),
                                    (dense[:, 2], gpu[:, 2], 3 * T)):
            rows, Rn, Tn, ld = C._rows(view)
            assert rows.data_ptr() == view.data_ptr() and (Rn, Tn, ld) == (view.numel() // T, T, want_ld), name   # no copy
            assert torch.equal(call(view).view(torch.int32), same.contiguous().view(torch.int32)), name
    assert torch.isnan(big[:, :, T:]).all()
    # a view that does not collapse to one row stride is copied, not misread; float64 input is narrowed once
    odd = dense[::2, ::2]
    assert C._rows(odd)[0].data_ptr() != odd.data_ptr()
    assert torch.equal(C.highpass_filter(odd), C.highpass_filter(dense)[::2, ::2])
    assert torch.equal(C.highpass_filter(dense.double()), C.highpass_filter(dense))
    assert torch.equal(C.bandpass(dense, 0.1, 30, 100), C.sosfilt(sos, dense))
    with pytest.warns(UserWarning, match="Nyquist"):
        assert torch.equal(C.bandpass(dense, 0.1, 50, 100), C.highpass_filter(dense))
