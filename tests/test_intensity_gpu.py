"""Ground-motion intensity measures on the GPU (csrc/intensity.hip, tqdne_amd/ground_motion.py) against the float64 restatement of
tests/_intensity_ref.py (smtk itself is not run).  tq_rotd_peaks is called through the C ABI with its output inside NaN-filled
guard bands; the Python surface is exercised by the combination, kind and refusal tests.

Bar.  Per series (waveform, k) the error max_phi |m_gpu - m_ref| is divided by that series' largest peak max_phi m_ref.  The worst of
these over a case must be at most 8 x the worst of the SAME figure for the float32 emulation of the sequential scaled-state
recurrence (R.emulate_peaks_f32: fp32 coefficients, every product and sum rounded to fp32, no fused multiply-add) over the same
inputs and periods: the kernel may contract a product and a sum into one rounding and the emulation does not, which reorders
nothing but moves single roundings, hence a factor and not equality.  The bar is computed here from the emulation, never from the
kernel; both figures are printed.  Every series is also held to the suite's standing bar (conftest.rel_err: 1e-3 norm-wise and
element-wise).  The combined measures (percentiles over the angles, the spectral acceleration of one component) are 1-Lipschitz
in the peaks apart from GMRotD's square root, and are held to the same 8 x emulation figure of their case, per series and relative
to that series' largest peak."""

import functools

import numpy as np
import pytest
import torch

import _intensity_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
G = 4096          # floats of NaN either side of every output
DT = 0.01
FACTOR = 8.0


def _dev():
    return torch.device("cuda:0")


def _periods(P):
    return tuple(R.PERIODS7) if P == 7 else tuple(float(p) for p in R.periods_log(P))


def gpu_peaks(x, y, periods, dt=DT, damping=0.05):
    """x, y (N, T) float32 numpy -> (N, 3 + P, 180) float32 through tq_rotd_peaks, the output between guard bands"""
    from tqdne_amd import _lib
    from tqdne_amd.ground_motion import oscillator_tables
    lib = _lib.load()
    N, T = x.shape
    P = len(periods)
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(_dev())   # a copy: the cached inputs are read-only
    yd = torch.from_numpy(np.array(y, dtype=np.float32)).to(_dev())
    tab = torch.from_numpy(oscillator_tables(periods, dt, damping)).to(_dev())
    n = N * (3 + P) * 180
    buf = torch.full((n + 2 * G,), float("nan"), device=_dev(), dtype=torch.float32)
    _lib.check(lib.tq_rotd_peaks(xd.data_ptr(), yd.data_ptr(), tab.data_ptr(), buf[G:].data_ptr(), N, T, P, dt,
                                 torch.cuda.current_stream().cuda_stream), "rotd_peaks")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all()), "guard band touched"
    return buf[G:G + n].cpu().numpy().reshape(N, 3 + P, 180)


@functools.lru_cache(maxsize=None)
def _case(T, P, N=3):
    """inputs, the float64 peaks, and the emulation's worst per-series error (the bar is FACTOR times it); computed once, read only"""
    x, y = R.make_waveforms(N, T, seed=T + P)
    per = _periods(P)
    ref = R.rotd_peaks(x, y, DT, per)
    emu = float(R.series_error(R.emulate_peaks_f32(x, y, DT, per), ref).max())
    for a in (x, y, ref):
        a.setflags(write=False)
    return x, y, per, ref, emu


@pytest.mark.parametrize("T", [2, 3, 65, 257, 4064])
@pytest.mark.parametrize("P", [7, 1, 70])
def test_rotd_peaks_against_float64(T, P):
    """Measured on an MI355X: the figures printed here, quoted in DESIGN.md section 8e."""
    x, y, per, ref, emu = _case(T, P)
    m = gpu_peaks(x, y, per)
    assert m.shape == ref.shape == (3, 3 + P, 180) and not np.isnan(m).any(), "an element left unwritten"
    err = R.series_error(m, ref)
    print(f"rotd_peaks T {T} P {P}: worst series error GPU {err.max():.2e}, fp32 emulation {emu:.2e} (bar {FACTOR * emu:.2e}); "
          f"ground series {err[:, :3].max():.2e}")
    assert emu > 0.0
    assert err.max() <= FACTOR * emu
    nonzero = [(n, k) for n in range(3) for k in range(3 + P) if ref[n, k].max() > 0.0]
    assert max(rel_err(m[n, k], ref[n, k].copy()) for n, k in nonzero) < 1e-3   # (a copy: the cached reference is read-only)
    # the unrotated angles are the components' own peaks, and the degenerate pairs behave: y = 0 gives |cos| times the peak of x,
    # x = y leaves nothing at 135 degrees
    assert np.array_equal(m[1, :, 90], np.zeros(3 + P, np.float32))
    assert np.array_equal(m[2, :, 135], np.zeros(3 + P, np.float32))
    c, _ = R.angle_table(np.float32)
    assert np.array_equal(m[1], m[1, :, :1] * np.abs(c))


@pytest.mark.parametrize("T", [257, 4064])
def test_gmrotdpp_and_response_spectrum_against_the_restatement(T):
    from tqdne_amd import ground_motion as GM
    x, y, per, ref, emu = _case(T, 7)
    top = ref.max(-1)
    xd, yd = torch.from_numpy(x.copy()).to(_dev()), torch.from_numpy(y.copy()).to(_dev())
    worst = 0.0
    for kind in ("gmrotd", "rotd"):
        for q in (0, 16, 50, 84, 100):
            out = GM.gmrotdpp_with_pg(xd, yd, DT, per, percentile=q, kind=kind)
            want = R.gmrotdpp_with_pg(None, None, DT, per, q, kind=kind, peaks=ref)
            assert sorted(out) == ["Acceleration", "PGA", "PGD", "PGV"]
            assert all(v.is_cuda and v.dtype == torch.float32 for v in out.values())
            assert out["PGA"].shape == (3,) and out["Acceleration"].shape == (3, 7)
            got = np.concatenate([np.stack([out[k].cpu().numpy() for k in ("PGA", "PGV", "PGD")], -1), out["Acceleration"].cpu().numpy()], -1)
            ref_g = np.concatenate([np.stack([want[k] for k in ("PGA", "PGV", "PGD")], -1), want["Acceleration"]], -1)
            e = float((np.abs(got - ref_g) / top).max())
            worst = max(worst, e)
            assert e <= FACTOR * emu, (kind, q, e, emu)
            assert rel_err(got, ref_g) < 1e-3
            if kind == "gmrotd":
                sa = GM.parallel_processing_sa(xd, yd, DT, per, q)
                assert torch.equal(sa, out["Acceleration"])
    sa_x = GM.response_spectrum(xd, DT, per)
    want = R.response_spectrum(x.astype(np.float64), DT, per)
    assert sa_x.is_cuda and sa_x.shape == (3, 7)
    e = float((np.abs(sa_x.cpu().numpy() - want) / want).max())
    print(f"T {T}: combined measures worst {worst:.2e}, response_spectrum {e:.2e}, fp32 emulation {emu:.2e} (bar {FACTOR * emu:.2e})")
    assert e <= FACTOR * emu and rel_err(sa_x.cpu().numpy(), want) < 1e-3
    assert np.array_equal(sa_x.cpu().numpy(), gpu_peaks(x, np.zeros_like(x), per)[:, 3:, 0])


@pytest.mark.parametrize("P", [7, 70])
def test_waveforms_are_independent_and_launches_repeat_bit_for_bit(P):
    x, y = R.make_waveforms(5, 257, seed=11)
    per = _periods(P)
    m = gpu_peaks(x, y, per)
    assert np.array_equal(gpu_peaks(x, y, per), m)                           # two launches
    assert np.array_equal(gpu_peaks(x[::-1], y[::-1], per), m[::-1])         # the batch reversed
    for i in range(5):                                                       # every row alone
        assert np.array_equal(gpu_peaks(x[i:i + 1], y[i:i + 1], per), m[i:i + 1]), i


@pytest.mark.parametrize("P", [7, 70])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_sample_poisons_its_waveform_only(bad, P):
    x, y = R.make_waveforms(5, 257, seed=12)
    per = _periods(P)
    clean = gpu_peaks(x, y, per)
    assert np.isfinite(clean).all()
    for comp, row, t in ((0, 3, 100), (1, 0, 0), (0, 4, 256), (1, 2, 255)):   # first, last and last-but-one samples included
        xb, yb = x.copy(), y.copy()
        (xb, yb)[comp][row, t] = bad
        m = gpu_peaks(xb, yb, per)
        assert np.isnan(m[row]).all(), (comp, row, t)
        others = [i for i in range(5) if i != row]
        assert np.array_equal(m[others], clean[others]), (comp, row, t)
    from tqdne_amd import ground_motion as GM
    xb = x.copy()
    xb[1, 7] = bad
    out = GM.gmrotdpp_with_pg(xb, y, DT, per, 50)
    ok = GM.gmrotdpp_with_pg(x, y, DT, per, 50)
    for k in out:
        assert np.isnan(out[k][1]).all() and np.array_equal(np.delete(out[k], 1, 0), np.delete(ok[k], 1, 0))


def test_host_inputs_come_back_as_host_arrays_and_leading_dimensions_are_kept():
    from tqdne_amd import ground_motion as GM
    x, y = R.make_waveforms(6, 65, seed=13)
    per = _periods(7)
    m = gpu_peaks(x, y, per)
    mn = GM.rotd_peaks(x.reshape(2, 3, 65), y.reshape(2, 3, 65), DT, per)
    assert isinstance(mn, np.ndarray) and mn.dtype == np.float32 and mn.shape == (2, 3, 10, 180) and np.array_equal(mn.reshape(6, 10, 180), m)
    mt = GM.rotd_peaks(torch.from_numpy(x), torch.from_numpy(y), DT, list(per))
    assert isinstance(mt, torch.Tensor) and not mt.is_cuda and np.array_equal(mt.numpy(), m)
    md = GM.rotd_peaks(torch.from_numpy(x).to(_dev()).reshape(3, 2, 65), torch.from_numpy(y).to(_dev()).reshape(3, 2, 65), DT, np.array(per))
    assert md.is_cuda and md.shape == (3, 2, 10, 180) and np.array_equal(md.cpu().numpy().reshape(6, 10, 180), m)
    out = GM.gmrotdpp_with_pg(x.reshape(2, 3, 65), y.reshape(2, 3, 65), DT, per)
    assert all(isinstance(v, np.ndarray) for v in out.values()) and out["PGV"].shape == (2, 3) and out["Acceleration"].shape == (2, 3, 7)
    sa = GM.parallel_processing_sa(x, y, DT, per, 50)
    assert isinstance(sa, np.ndarray) and sa.shape == (6, 7) and np.array_equal(sa, out["Acceleration"].reshape(6, 7))
    one = GM.response_spectrum(x[0], DT, per)
    assert isinstance(one, np.ndarray) and one.shape == (7,)
    # the tables are cached by (periods, dt, damping, device)
    n = len(GM._TABLES)
    GM.rotd_peaks(x, y, DT, per)
    assert len(GM._TABLES) == n
    GM.rotd_peaks(x, y, DT, per, damping=0.1)
    assert len(GM._TABLES) == n + 1


def test_refusals_name_the_limit():
    from tqdne_amd import ground_motion as GM
    z = torch.zeros(2, 16, device=_dev())
    with pytest.raises(ValueError, match="T >= 2"):
        GM.rotd_peaks(z[:, :1], z[:, :1], DT, [1.0])
    with pytest.raises(ValueError, match="periods"):
        GM.rotd_peaks(z, z, DT, [1.0, 0.0])
    with pytest.raises(ValueError, match="periods"):
        GM.gmrotdpp_with_pg(z, z, DT, [-0.5])
    with pytest.raises(ValueError, match="equal shapes"):
        GM.rotd_peaks(z, z[:, :15], DT, [1.0])
    with pytest.raises(ValueError, match="equal shapes"):
        GM.parallel_processing_sa(z, z[:1], DT, [1.0], 50)
