"""The duration kernels (csrc_duration/duration.hip, tqdne_amd/duration.py) against the float64 restatement of tests/_duration_ref.py
and, on the fixture's inputs, against the reference's own results.  tqd_arias and tqd_gradient are called through the C ABI: the input
rows are the channel views 0 and 1 of an (R, 3, T + pad) tensor that is NaN elsewhere (pad 5: rows at odd addresses, the
sample-by-sample loads; pad 4: 16-byte loads where T allows), every output sits between guard bands that are checked afterwards.

The kernel gives one wave to a row and, with C = ceil(T / 64), the samples l C ... (l + 1) C - 1 to lane l.  The lengths are those at
which that can go wrong: T = 2, 3 (one or two lanes busy), 63, 64, 65 (C = 1, 1, 2: the last lanes empty at 65), 127, 128, 129, 1000
(C = 16, a partial last chunk), 4064 (the reference's length, C = 64, 32 empty samples in the last chunk), 4097 (C = 65).

Bounds.  Energy: |energy - exact| <= (T + 8) 2^-52 exact, exact = math.fsum of the restatement's float64 terms: a sum of n positive
terms in any order is within (n - 1) u of exact, forming the terms adds a few u, the factor 2 is the margin.  Peak: exact.  Husid
curve: |h - h64| <= 2^-24 h64 + (T + 8) 2^-52.  Crossings: equal to the restatement's on rows whose restatement keeps cum[n] and
cum[n-1] at least 1e-6 of the total from the threshold (asserted first, never skipped); spike rows are analytic, no tolerance.
Gradient: |g - g64| <= 4 * 2^-24 |g64| + 1e-37 (three roundings to first order)."""

import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _duration_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 256                # guard elements either side of every output
ROWS = [1, 3, 5, 65, 130]
LENGTHS = [2, 3, 63, 64, 65, 127, 128, 129, 1000, 4064, 4097]
FRACTIONS = [0.95, 0.05, 0.5, 1.0, 0.0, 0.75, 0.2, 0.333]   # F = 8, unsorted
CROSS_ROWS = 4         # rows of every sweep case whose crossings are held to the restatement's (their margin is asserted)
SEED = 23             # chosen on the CPU: the restatement's crossing margin on the CROSS_ROWS rows of every case is 1.08e-5
U = 2.0 ** -52
WAVE = 64


def _dev():
    return torch.device("cuda:0")


def _lib():
    from tqdne_amd import _lib_duration
    return _lib_duration.load()


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _channel_views(x, y, pad):
    """(R, T) float32 rows -> the (R, 3, T + pad) tensor, NaN but for the first T samples of channels 0 (x) and 1 (y)"""
    Rn, T = x.shape
    big = torch.full((Rn, 3, T + pad), float("nan"), device=_dev())
    big[:, 0, :T] = torch.from_numpy(np.array(x)).to(_dev())
    if y is not None:
        big[:, 1, :T] = torch.from_numpy(np.array(y)).to(_dev())
    return big


def _guarded(n, dtype, fill):
    return torch.full((G + n + G,), fill, device=_dev(), dtype=dtype)


def _unguard(buf, n, fill):
    same = (lambda t: torch.isnan(t).all()) if fill != fill else (lambda t: (t == fill).all())
    assert same(buf[:G]) and same(buf[G + n:]), "a guard band was written"
    return buf[G:G + n].cpu().numpy()


def c_arias(x, y=None, step=0.01, fractions=FRACTIONS, want_husid=True, pad=5):
    """-> energy (R,), peak2 (R,), index (R, F), husid (R, T) or None"""
    Rn, T = x.shape
    F = len(fractions)
    big = _channel_views(x, y, pad)
    before = big.clone()
    ld = 3 * (T + pad)
    energy, peak2 = _guarded(Rn, torch.float64, float("nan")), _guarded(Rn, torch.float64, float("nan"))
    index = _guarded(Rn * F, torch.int32, -777)
    curve = _guarded(Rn * T, torch.float32, float("nan")) if want_husid else None
    fr = (ctypes.c_double * F)(*fractions)
    rc = _lib().tqd_arias(big.data_ptr(), big.data_ptr() + 4 * (T + pad) if y is not None else None, energy.data_ptr() + 8 * G,
                          peak2.data_ptr() + 8 * G, index.data_ptr() + 4 * G, curve.data_ptr() + 4 * G if want_husid else None, Rn, T,
                          ld, ld, step, fr, F, _stream())
    assert rc == 0, rc
    out = (_unguard(energy, Rn, float("nan")), _unguard(peak2, Rn, float("nan")), _unguard(index, Rn * F, -777).reshape(Rn, F),
           _unguard(curve, Rn * T, float("nan")).reshape(Rn, T) if want_husid else None)
    assert torch.equal(big.view(torch.int32), before.view(torch.int32)), "the input was written"
    return out


def c_gradient(x, dt=0.01, pad=5, gap=3):
    Rn, T = x.shape
    big = _channel_views(x, None, pad)
    before = big.clone()
    out = _guarded(Rn * (T + gap), torch.float32, float("nan"))
    rc = _lib().tqd_gradient(big.data_ptr(), out.data_ptr() + 4 * G, Rn, T, 3 * (T + pad), T + gap, dt, _stream())
    assert rc == 0, rc
    body = _unguard(out, Rn * (T + gap), float("nan")).reshape(Rn, T + gap)
    assert np.isnan(body[:, T:]).all(), "between the output rows was written"
    assert torch.equal(big.view(torch.int32), before.view(torch.int32)), "the input was written"
    return body[:, :T]


@functools.lru_cache(None)
def _pairs(T):
    x, y = R.make_pairs(max(ROWS), T, seed=SEED)
    x.setflags(write=False), y.setflags(write=False)
    return x, y


@functools.lru_cache(None)
def _ref(T, two, step=0.01):
    """the restatement of the sweep's rows, computed once: (cum (R, T), exact total (R,), peak2 (R,))"""
    x, y = _pairs(T)
    yy = y if two else None
    out = R.cumulative(x, yy, step), R.exact_total(x, yy, step), R.squares(x, yy).max(-1)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def _fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "duration.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _assert_crossings_within_rounding(index, cum, total, T):
    """every row, whatever its margin: the kernel's crossing n has cum64[n] >= thr - e and cum64[n-1] < thr + e, with
    e = 2 (T + 8) u total covering both sums' distance from the exact one"""
    e = 2 * (T + 8) * U * total
    for j, f in enumerate(FRACTIONS):
        n = index[:, j]
        assert ((n >= 0) & (n < T)).all()
        thr = f * total
        rows = np.arange(len(n))
        assert (cum[rows, n] >= thr - e).all(), (T, f)
        prev = np.where(n > 0, cum[rows, np.maximum(n - 1, 0)], -np.inf)
        assert (prev < thr + e).all(), (T, f)


# ---- the sweep: energy, peak, curve, crossings, batch independence --------------------------------------------------------

@pytest.mark.parametrize("two", [False, True], ids=["one_component", "two_components"])
@pytest.mark.parametrize("T", LENGTHS)
def test_sweep_against_the_float64_restatement(T, two):
    x, y = _pairs(T)
    yy = y if two else None
    cum, exact, peak = _ref(T, two)
    total = cum[:, -1]
    inner = [f for f in FRACTIONS if 0.0 < f < 1.0]
    margin = R.crossing_margin(cum[:CROSS_ROWS], inner)
    print(f"T={T}: crossing margin of the restatement on {CROSS_ROWS} rows {margin:.2e}")
    assert margin >= 1e-6      # the seed is chosen for this; a failure here is a failure of the test
    want_idx = R.crossings(cum, FRACTIONS)
    full = None
    for pad in (5, 4):
        energy, peak2, index, curve = c_arias(x, yy, pad=pad)
        err = np.abs(energy - exact) / exact
        print(f"T={T} pad={pad}: energy error / bound {float(err.max() / ((T + 8) * U)):.3f}")
        assert (err <= (T + 8) * U).all()
        assert np.array_equal(_bits(peak2), _bits(peak))
        h64 = cum / total[:, None]
        assert (np.abs(curve - h64) <= 2.0 ** -24 * h64 + (T + 8) * U).all()
        assert (curve[:, 0] == 0).all() and (curve[:, -1] == 1).all() and (np.diff(curve, axis=-1) >= 0).all()
        assert np.array_equal(index[:CROSS_ROWS], want_idx[:CROSS_ROWS])
        _assert_crossings_within_rounding(index, cum, total, T)
        assert (index[:, FRACTIONS.index(0.0)] == 0).all() and (index[:, FRACTIONS.index(1.0)] <= T - 1).all()
        if full is None:
            full = (energy, peak2, index, curve)
        else:   # 16-byte loads and sample-by-sample loads: the same sums in the same order
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(full, (energy, peak2, index, curve)))
    # a row alone and in smaller batches against the same row inside R = 130; the same call twice; no curve asked for
    again = c_arias(x, yy)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(full, again))
    for Rn in ROWS[:-1]:
        part = c_arias(x[:Rn], yy[:Rn] if two else None)
        assert all(np.array_equal(_bits(a[:Rn]), _bits(b)) for a, b in zip(full, part)), Rn
    for r in (64, 129):
        one = c_arias(x[r:r + 1], yy[r:r + 1] if two else None)
        assert all(np.array_equal(_bits(a[r:r + 1]), _bits(b)) for a, b in zip(full, one)), r
    bare = c_arias(x, yy, want_husid=False)
    assert bare[3] is None and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(full[:3], bare[:3]))


@pytest.mark.parametrize("T", [65, 4064])
def test_every_number_of_fractions_and_the_step(T):
    x, y = _pairs(T)
    x, y = x[:5], y[:5]
    full = c_arias(x, y)
    for F in range(1, 9):
        part = c_arias(x, y, fractions=FRACTIONS[:F])
        assert part[2].shape == (5, F) and np.array_equal(part[2], full[2][:, :F])
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((full[0], full[1], full[3]), (part[0], part[1], part[3])))
    # the step scales the energy and leaves the crossings where they are (a power of two: bit for bit)
    scaled = c_arias(x, y, step=0.01 * 4)
    assert np.array_equal(_bits(scaled[0]), _bits(4 * full[0])) and np.array_equal(scaled[2], full[2])
    other = c_arias(x, y, step=0.01 * T / (T - 1))
    exact = R.exact_total(x, y, 0.01 * T / (T - 1))
    assert (np.abs(other[0] - exact) <= (T + 8) * U * exact).all()


# ---- spike rows: analytic ---------------------------------------------------------------------------------------------

def _spike_positions(T):
    C = -(-T // WAVE)
    seams = [k for l in range(1, WAVE) if l * C < T for k in (l * C - 1, l * C)]
    return sorted(set([0, 1, T - 2, T - 1] + seams) & set(range(T)))


@pytest.mark.parametrize("two", [False, True], ids=["one_component", "two_components"])
@pytest.mark.parametrize("T", LENGTHS)
def test_spike_rows_cross_where_the_arithmetic_says(T, two):
    """all energy at one index k: the terms that end at k and at k + 1 are the same number a, cum is 0 before k, a at k and 2 a from
    k + 1 on (k = 0 has no term ending at it, k = T - 1 none after it): every value exact in any order"""
    ks = _spike_positions(T)
    assert {0, T - 1} <= set(ks) and (T < 4 or len(ks) >= 4)
    x = np.zeros((len(ks), T), np.float32)
    y = np.zeros((len(ks), T), np.float32)
    for r, k in enumerate(ks):
        x[r, k] = 3.0 if r % 2 else -3.0
        if two:
            y[r, k] = 4.0
    fr = [0.5, 0.95, 0.05, 1.0, 0.0, 0.51, 0.49, 2.0 ** -40]
    energy, peak2, index, curve = c_arias(x, y if two else None, step=0.0101, fractions=fr)
    s = 25.0 if two else 9.0
    a = (0.0 + s) * (0.5 * 0.0101)
    for r, k in enumerate(ks):
        levels = np.zeros(T)     # cum in units of a
        if k >= 1:
            levels[k:] += 1
        if k + 1 <= T - 1:
            levels[k + 1:] += 1
        assert energy[r] == levels[-1] * a and peak2[r] == s
        want = [int(np.flatnonzero(levels >= f * levels[-1])[0]) for f in fr]
        assert list(index[r]) == want, (T, k, list(index[r]), want)
        if 1 <= k <= T - 2:   # the rule in words: k up to a half, k + 1 above it
            assert want == [k, k + 1, k, k + 1, 0, k + 1, k, k]
        assert np.array_equal(curve[r], (levels / levels[-1]).astype(np.float32))


# ---- edge rows --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("two", [False, True], ids=["one_component", "two_components"])
@pytest.mark.parametrize("T", [2, 65, 4064])
def test_zero_and_non_finite_rows_and_their_neighbours(T, two):
    x, y = _pairs(T)
    x, y = np.array(x[:11]), np.array(y[:11])
    clean = c_arias(x, y if two else None)
    x2, y2 = x.copy(), y.copy()
    x2[1] = 0.0
    y2[1] = 0.0
    x2[3, 0], x2[5, T - 1], x2[7, T // 2] = np.nan, np.inf, -np.inf
    bad = [3, 5, 7]
    if two:
        y2[9, T // 3] = np.nan
        bad.append(9)
    energy, peak2, index, curve = c_arias(x2, y2 if two else None)
    assert energy[1] == 0 and peak2[1] == 0 and (index[1] == -1).all() and np.isnan(curve[1]).all()
    assert np.isnan(energy[bad]).all() and np.isnan(peak2[bad]).all() and (index[bad] == -1).all() and np.isnan(curve[bad]).all()
    keep = [r for r in range(11) if r != 1 and r not in bad]
    for a, b in zip(clean, (energy, peak2, index, curve)):
        assert np.array_equal(_bits(a[keep]), _bits(b[keep]))
    bare = c_arias(x2, y2 if two else None, want_husid=False)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((energy, peak2, index), bare[:3]))


# ---- gradient ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", LENGTHS)
def test_gradient_is_numpys_float32_formula(T):
    x = _pairs(T)[0]
    for dt in (0.01, 0.02):
        g64 = R.gradient(x, dt)
        g = c_gradient(x, dt)
        assert (np.abs(g - g64) <= 4 * 2.0 ** -24 * np.abs(g64) + 1e-37).all()
        want = np.gradient(x, dt, axis=-1)
        print(f"T={T} dt={dt}: {int((_bits(g) == _bits(want)).sum())} of {g.size} elements bit-equal to numpy.gradient on float32")
        for Rn in (1, 3):
            assert np.array_equal(_bits(c_gradient(x[:Rn], dt)), _bits(g[:Rn]))
    assert np.array_equal(_bits(c_gradient(x, 0.01, pad=4, gap=0)), _bits(c_gradient(x, 0.01)))


def test_gradient_propagates_non_finite_samples_as_numpy_does():
    T = 129
    x = np.array(_pairs(T)[0][:6])
    x[1, 0], x[2, T - 1], x[3, 64], x[4, 1] = np.nan, np.inf, np.nan, -np.inf
    g = c_gradient(x)
    with np.errstate(invalid="ignore"):
        want = np.gradient(x, 0.01, axis=-1)
    assert np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(np.isinf(g), np.isinf(want))
    assert np.isfinite(g[[0, 5]]).all() and np.isnan(g[3, [63, 65]]).all() and np.isfinite(g[3, 64])


# ---- the Python surface -----------------------------------------------------------------------------------------------

def _fixture_on_gpu(T):
    fx = _fx()
    return fx, torch.from_numpy(fx[f"w{T}"]).to(_dev()), fx[f"time{T}"]


@pytest.mark.parametrize("T", [257, 1000, 4064])
def test_fixture_crossings_are_the_references_and_shaking_duration(T):
    from tqdne_amd import duration as D
    fx, w, time = _fixture_on_gpu(T)
    step = (time[-1] - time[0]) / (T - 1)
    fracs = [p / 100 for p in fx["percents"].ravel()]
    cum = R.cumulative(fx[f"w{T}"][:, 1], fx[f"w{T}"][:, 0], step)
    assert R.crossing_margin(cum, fracs) >= 1e-6
    for k, (lo, hi) in enumerate(fx["percents"]):
        for tag in ("raw", "norm"):
            Ia, t0, t1, d = D.significant_duration(w[:, 1], w[:, 0], time=time, lower_percent=int(lo), upper_percent=int(hi),
                                                   normalize=tag == "norm")
            assert all(v.is_cuda and v.dtype == torch.float64 and v.shape == (len(w),) for v in (Ia, t0, t1, d))
            idx = fx[f"{tag}_idx{T}"][:, k]
            assert np.array_equal(t0.cpu().numpy(), time[0] + idx[:, 0] * step) and np.array_equal(t1.cpu().numpy(), time[0] + idx[:, 1] * step)
            got = np.stack([t0.cpu().numpy(), t1.cpu().numpy(), d.cpu().numpy()], -1)
            assert (np.abs(got - fx[f"{tag}_dur{T}"][:, k]) <= 1e-6 * np.abs(fx[f"{tag}_dur{T}"][:, k])).all()
            assert (np.abs(Ia.cpu().numpy() - fx[f"{tag}_Ia{T}"]) <= 1e-6 * fx[f"{tag}_Ia{T}"]).all()
    a, b = D.shaking_duration(w, w.flip(0))
    assert a.is_cuda and b.is_cuda and torch.equal(b, a.flip(0))
    want = fx[f"norm_dur{T}"][:, 0, 2]
    assert (np.abs(a.cpu().numpy() - want) <= 1e-6 * want).all()
    c, _ = D.shaking_duration(w, w, lower_percent=20, upper_percent=75)
    assert (np.abs(c.cpu().numpy() - fx[f"norm_dur{T}"][:, 1, 2]) <= 1e-6 * fx[f"norm_dur{T}"][:, 1, 2]).all()
    single = D.significant_duration(w[0, 0], time=time)
    assert all(v.shape == () for v in single)
    got = np.array([float(v) for v in single])
    want = np.concatenate([[fx[f"single_Ia{T}"]], fx[f"single_dur{T}"]])
    assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all()


@pytest.mark.parametrize("T", [257, 4064])
def test_fused_route_equals_the_pieces(T):
    from tqdne_amd import duration as D
    fx, w, time = _fixture_on_gpu(T)
    step = (time[-1] - time[0]) / (T - 1)
    # the float32 curve the pieces compare moves a crossing only inside 2^-24 of the total: the margin asserted here is 1e-6
    assert R.crossing_margin(R.cumulative(fx[f"w{T}"][:, 0], None, step), [0.05, 0.95]) >= 1e-6
    x = w[:, 0]
    Ia, cum = D.calculate_arias_intensity(time, x)
    assert Ia.is_cuda and cum.is_cuda and Ia.dtype == cum.dtype == torch.float64 and cum.shape == x.shape
    t0, t1, d = D.calculate_signal_duration(time, cum, Ia)
    fIa, f0, f1, fd = D.significant_duration(x, time=time)
    assert torch.equal(fIa, Ia)
    for fused, piece in ((f0, t0), (f1, t1)):   # the pieces read time[n], the fused route forms t0 + n step: the same n
        n_fused, n_piece = np.rint(fused.cpu().numpy() / step), np.searchsorted(time, piece.cpu().numpy())
        assert np.array_equal(n_fused, n_piece) and np.array_equal(time[n_piece], piece.cpu().numpy())
        assert np.allclose(fused.cpu().numpy(), piece.cpu().numpy(), rtol=1e-12, atol=0)
    assert np.allclose(fd.cpu().numpy(), d.cpu().numpy(), rtol=1e-11, atol=0)
    exact = np.pi / (2 * 9.81) * R.exact_total(fx[f"w{T}"][:, 0], None, step)
    assert (np.abs(Ia.cpu().numpy() - exact) <= (T + 12) * U * exact).all()
    c64 = np.pi / (2 * 9.81) * R.cumulative(fx[f"w{T}"][:, 0], None, step)
    assert (np.abs(cum.cpu().numpy() - c64) <= (2.0 ** -24 + (T + 12) * U) * c64[:, -1:]).all()
    h = D.husid(x, time=time)
    assert h.dtype == torch.float32 and torch.equal(h.double() * Ia[..., None], cum)
    assert torch.equal(D.husid(w[:, 1], w[:, 0], dt=step), D.husid(w[:, 1], w[:, 0], time=time))
    g = D.compute_time_derivative(w)
    assert g.is_cuda and g.dtype == torch.float32 and g.shape == w.shape
    g64 = R.gradient(fx[f"w{T}"], 0.01)
    assert (np.abs(g.cpu().numpy() - g64) <= 4 * 2.0 ** -24 * np.abs(g64) + 1e-37).all()
    # edge rows through the surface: NaN times
    z = w.clone()
    z[0] = 0.0
    z[1, 0, 5] = float("nan")
    Ia, t0, t1, d = D.significant_duration(z[:, 1], z[:, 0], dt=0.01, normalize=True)
    assert torch.isnan(Ia[:2]).all() and torch.isnan(t0[:2]).all() and torch.isnan(t1[:2]).all() and torch.isnan(d[:2]).all()
    assert torch.isfinite(d[2:]).all()
    assert float(D.significant_duration(z[0, 0], dt=0.01)[0]) == 0.0


def test_dispatch_and_views():
    from tqdne_amd import duration as D
    from tqdne_amd.conditioning import _rows
    T = 257
    fx, dense, time = _fixture_on_gpu(T)
    w = fx[f"w{T}"]
    big = torch.full((3, 2, T + 5), float("nan"), device=_dev())
    big[:, :, :T] = dense
    calls = {"significant_duration": lambda a: D.significant_duration(a[:, 1], a[:, 0], dt=0.01),
             "husid": lambda a: D.husid(a[:, 1], a[:, 0], dt=0.01), "compute_time_derivative": D.compute_time_derivative,
             "shaking_duration": lambda a: D.shaking_duration(a, a)}
    tup = lambda v: v if isinstance(v, tuple) else (v,)
    for name, call in calls.items():
        host = tup(call(w))
        assert all(isinstance(v, np.ndarray) for v in host), name
        cpu = tup(call(torch.from_numpy(w)))
        assert all(isinstance(v, torch.Tensor) and not v.is_cuda and np.array_equal(v.numpy(), h) for v, h in zip(cpu, host)), name
        gpu = tup(call(dense))
        assert all(v.is_cuda and v.shape == h.shape for v, h in zip(gpu, host)), name
        assert all(np.allclose(v.cpu().numpy(), h, rtol=1e-5, atol=1e-6) for v, h in zip(gpu, host)), name
        view = tup(call(big[:, :, :T]))
        assert all(torch.equal(a, b) for a, b in zip(view, gpu)), name
    for view, want_ld in ((big[:, 1, :T], 2 * (T + 5)), (big[:, :, :T], T + 5), (dense[:, 0], 2 * T), (big[2, 0, :T], T)):
        rows, Rn, Tn, ld = _rows(view)
        assert rows.data_ptr() == view.data_ptr() and (Rn, Tn, ld) == (view.numel() // T, T, want_ld)   # no copy
    assert torch.isnan(big[:, :, T:]).all()
    # a view that does not collapse to one row stride is copied, not misread; float64 input is narrowed once; leading dimensions
    odd = dense[::2, :, ::2]
    assert torch.equal(D.husid(odd[:, 0], dt=0.01), D.husid(odd[:, 0].contiguous(), dt=0.01))
    assert torch.equal(D.husid(dense.double(), dt=0.01), D.husid(dense, dt=0.01))
    assert all(v.shape == (3, 2) for v in D.significant_duration(dense, dt=0.01))
    r = D.calculate_resultant_horizontal(dense[:, 1], dense[:, 0])
    assert r.is_cuda and np.allclose(r.cpu().numpy(), fx["resultant257"], rtol=1e-6)


def test_chain_condition_stream_feeds_the_duration():
    from tqdne_amd import conditioning as C, duration as D
    T = 1000
    fx, w, _ = _fixture_on_gpu(T)
    on_gpu = C.condition_stream(w)
    on_host = C.condition_stream(fx[f"w{T}"]).astype(np.float32)
    got = D.significant_duration(on_gpu[:, 1], on_gpu[:, 0], dt=0.01, normalize=True)
    want = D.significant_duration(on_host[:, 1], on_host[:, 0], dt=0.01, normalize=True)
    assert all(v.is_cuda for v in got) and all(isinstance(v, np.ndarray) for v in want)
    assert np.allclose(got[0].cpu().numpy(), want[0], rtol=1e-4)
    assert np.allclose(got[3].cpu().numpy(), want[3], atol=0.0201)   # (the two filters differ by 1e-7: a sample at either end)


def test_refusals_of_the_gpu_route():
    from tqdne_amd import duration as D
    T = 257
    _, w, time = _fixture_on_gpu(T)
    bent = time.copy()
    bent[100] += 1e-8
    for bad in (bent, time[::-1].copy(), np.cumsum(np.linspace(0.005, 0.02, T))):
        with pytest.raises(ValueError, match="uniform"):
            D.significant_duration(w[:, 0], time=bad)
        with pytest.raises(ValueError, match="uniform"):
            D.husid(w[:, 0], time=bad)
        with pytest.raises(ValueError, match="uniform"):
            D.calculate_arias_intensity(bad, w[:, 0])
    with pytest.raises(ValueError, match="exactly one"):
        D.significant_duration(w[:, 0])
    with pytest.raises(ValueError, match="exactly one"):
        D.husid(w[:, 0], time=time, dt=0.01)
    with pytest.raises(ValueError, match="GPU"):
        D.significant_duration(w[:, 0], w[:, 1].cpu(), dt=0.01)
    with pytest.raises(ValueError, match="shapes"):
        D.significant_duration(w[:, 0], w[:2, 1], dt=0.01)
    with pytest.raises(ValueError, match="T >= 2"):
        D.compute_time_derivative(w[:, :, :1])
    with pytest.raises(ValueError, match="fractions"):
        D._arias_gpu(w[:, 0], None, 0.01, [0.5] * 9, False)
    assert D.significant_duration(w[:0, 0], dt=0.01)[0].shape == (0,)
