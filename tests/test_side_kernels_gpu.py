"""Direct parity of the side kernels (GPU): sampler state, EDM / consistency scalars, noise injection, losses, VAE bottleneck,
embedding MLPs, the small-GEMM job list and the backward plumbing -- every entry point of include/tqdne_hip.h that the suite used to
reach only through a whole model.  Each kernel is called through ctypes and held against the same formula in float64 on the CPU,
formed from the very float32 inputs the kernel gets (oracle/ where it states the formula, else the header comment), at the sizes
that reach the kernel's tail, its second grid-stride trip, its NULL-argument forms and every path of its launcher.

Every output is a slice out of the middle of a NaN-filled device tensor with GUARD elements either side: the bands must come back
bit-unchanged, and every input must equal the clone taken before the call.

Bars (none is a measurement): 1e-5 is the suite's bar for the exact-fp32 kernels (stem / head, test_colsum, test_linear); 2e-6 is
tests/test_representation.py's bar for fp32 results of a handful of roundings; the fp64 sampler state is held elementwise to
1e-14 * (|x| + |d dt|), about 45 times the worst case 4 * 2^-53 of its four fp64 operations with or without FMA contraction."""

import math

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

GUARD = 64
BAR_F32 = 1e-5       # exact-fp32 kernels with a reduction or a transcendental inside
BAR_FEW = 2e-6       # fp32 results of a handful of roundings
BAR_F64 = 1e-14      # fp64 sampler state, relative to the magnitudes that enter the sum
BAR_SAME = 1e-6      # the same loss twice (atomic adds of a few partial sums in another order)
TWO_TRIPS = 524288 + 37   # ew_grid caps the grid at 2048 workgroups of 256 threads (tq_mse_loss: 64 of 1024, 8 strides): 37 elements of a second trip


def dev():
    return torch.device("cuda:0")


def lib():
    from tqdne_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    """the tensor's bit patterns as integers (NaN compares equal to itself, -0.0 differs from 0.0)"""
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def p(t, offset=0):
    """device address (of element ``offset``) of a tensor or an Out; None stays None"""
    if t is None:
        return None
    t = t.view if isinstance(t, Out) else t
    return t.data_ptr() + offset * t.element_size()


class Out:
    """n output elements in the middle of a NaN-filled device tensor (``fill``: the values the kernel finds there)."""

    def __init__(self, n, dtype=torch.float32, fill=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev())
        self.view = self.buf[GUARD:GUARD + n]
        if fill is not None:
            self.view.copy_(torch.as_tensor(fill, dtype=dtype).reshape(-1))
        self.before = self.bands()
        self.prefill = bits(self.view).clone()

    def bands(self):
        v = bits(self.buf)
        return torch.cat([v[:GUARD], v[GUARD + self.n:]]).clone()

    def bands_intact(self):
        return torch.equal(self.bands(), self.before)

    def cpu(self, *shape):
        r = self.view.cpu()
        return r.reshape(*shape) if shape else r


class Case:
    """the device tensors of one call: inputs with their clones, outputs with their guard bands"""

    def __init__(self):
        self.ins, self.outs = [], []

    def inp(self, t):
        d = t.contiguous().to(dev())
        self.ins.append((d, d.clone()))
        return d

    def out(self, n, dtype=torch.float32, fill=None):
        o = Out(n, dtype, fill)
        self.outs.append(o)
        return o

    def verify(self):
        torch.cuda.synchronize()
        for i, (d, c) in enumerate(self.ins):
            assert torch.equal(bits(d), bits(c)), f"input {i} was written"
        for i, o in enumerate(self.outs):
            assert o.bands_intact(), f"guard band of output {i} was written"


def ok(rc):
    assert rc == 0, f"library call returned {rc}"


def gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 1009 * int(s) for i, s in enumerate(seed)) + 7)


def max_rel(a, b):
    """largest element-wise relative error, without a floor: used where the kernel's result is relatively accurate wherever the
    reference is small.  c_noise = log(sigma) / 4 vanishes at sigma = 1, but both sides take the logarithm of the SAME float32 sigma
    and logf is accurate to an ulp or two of its result there too (it is not formed as a difference), so a draw next to 1 does not
    lose the bar; the consistency model's c_out vanishes at sigma_min, where sigma - sigma_min of two nearby floats is exact."""
    a, b = a.double(), b.double()
    return float(((a - b).abs() / b.abs()).max())


def log_uniform_sigma(n, g):
    lo, hi = math.log(0.002), math.log(80.0)
    return (torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo).exp().float()


# ============================================================================================================================
# Heun sampler state
# ============================================================================================================================
SAMPLER_N = [1, 255, 257, TWO_TRIPS]
EDM_PAIR, LATE_PAIR, LAST_PAIR = (80.0, 57.6), (0.0047, 0.002), (0.002, 0.0)


def sigma_vector(case, s, s_next, coef=0.0):
    """sigma, sigma_next and coef as the sampler passes them: device scalars at an offset into a longer fp32 vector"""
    sv = torch.tensor([7.0, s, s_next, 3.0, coef, 11.0], dtype=torch.float32)
    return sv, case.inp(sv)


def heun_inputs(n, s, g):
    x = torch.randn(n, generator=g, dtype=torch.float64) * max(s, 1.0)
    den = torch.randn(n, generator=g, dtype=torch.float32)
    return x, den


def euler_ref(x, den, sv):
    sd = sv[1].double()
    dt = (sv[2] - sv[1]).double()   # float32(s_next) - float32(s) in float32, then widened (the header)
    d = (x - den.double()) / sd
    return d, x + d * dt, dt


def state_err(got, ref, scale):
    """|got - ref| in units of the bar's magnitude ``scale`` (elementwise), worst element"""
    return float(((got - ref).abs() / scale).max())


@pytest.mark.parametrize("n", SAMPLER_N)
def test_sampler_init(n):
    g = gen(n, 1)
    c = Case()
    z = torch.randn(n, generator=g, dtype=torch.float64)
    sv, svd = sigma_vector(c, 80.0, 57.6)
    zd = c.inp(z)
    x, x32 = c.out(n, torch.float64), c.out(n)
    ok(lib().tq_sampler_init(p(zd), p(svd, 1), p(x), p(x32), n, stream()))
    c.verify()
    ref = z * sv[1].double()
    e = state_err(x.cpu(), ref, ref.abs().clamp_min(1e-300))
    print(f"sampler_init n={n}: {e:.2e}")
    assert e <= BAR_F64
    assert torch.equal(bits(x32.cpu()), bits(x.cpu().float()))


@pytest.mark.parametrize("pair", [EDM_PAIR, LATE_PAIR, LAST_PAIR])
@pytest.mark.parametrize("n", SAMPLER_N)
def test_heun_euler(n, pair):
    g = gen(n, 2, int(pair[0] * 1000))
    c = Case()
    x, den = heun_inputs(n, pair[0], g)
    sv, svd = sigma_vector(c, *pair)
    xd, dend = c.inp(x), c.inp(den)
    dcur, xn, x32 = c.out(n, torch.float64), c.out(n, torch.float64), c.out(n)
    ok(lib().tq_heun_euler(p(xd), p(dend), p(svd, 1), p(svd, 2), p(dcur), p(xn), p(x32), n, stream()))
    c.verify()
    d, r, dt = euler_ref(x, den, sv)
    e_x = state_err(xn.cpu(), r, x.abs() + (d * dt).abs())
    e_d = state_err(dcur.cpu(), d, (x.abs() + den.double().abs()) / sv[1].double())
    print(f"heun_euler n={n} sigma {pair[0]} -> {pair[1]}: x_next {e_x:.2e} d_cur {e_d:.2e}")
    assert e_x <= BAR_F64 and e_d <= BAR_F64
    assert torch.equal(bits(x32.cpu()), bits(xn.cpu().float()))


@pytest.mark.parametrize("pair", [EDM_PAIR, LATE_PAIR])
@pytest.mark.parametrize("n", SAMPLER_N)
def test_heun_correct_separate_and_aliased(n, pair):
    """x_out as a buffer of its own and x_out = x, as _HeunRun.advance calls it: the same bits"""
    g = gen(n, 3, int(pair[0] * 1000))
    x, den = heun_inputs(n, pair[0], g)
    sv = torch.tensor([7.0, pair[0], pair[1], 3.0], dtype=torch.float32)
    dcur, xn, dt = euler_ref(x, den, sv)          # the state an Euler step leaves ...
    den2 = den + 0.1 * pair[1] * torch.randn(n, generator=g, dtype=torch.float32)   # ... and a second evaluation near the first
    dp = (xn - den2.double()) / sv[2].double()
    slope = 0.5 * dcur + 0.5 * dp
    ref = x + dt * slope

    c = Case()
    svd = c.inp(sv)
    xd, xnd, den2d, dcurd = c.inp(x), c.inp(xn), c.inp(den2), c.inp(dcur)
    xo, x32 = c.out(n, torch.float64), c.out(n)
    ok(lib().tq_heun_correct(p(xd), p(xnd), p(den2d), p(dcurd), p(svd, 1), p(svd, 2), p(xo), p(x32), n, stream()))
    c.verify()
    e = state_err(xo.cpu(), ref, x.abs() + (dt * slope).abs())
    print(f"heun_correct n={n} sigma {pair[0]} -> {pair[1]}: {e:.2e}")
    assert e <= BAR_F64
    assert torch.equal(bits(x32.cpu()), bits(xo.cpu().float()))
    assert float((xo.cpu() - (x + dt * dcur)).abs().max()) > 0 or n == 1   # (the second slope took part)

    a = Case()
    svd = a.inp(sv)
    xnd, den2d, dcurd = a.inp(xn), a.inp(den2), a.inp(dcur)
    xa, x32a = a.out(n, torch.float64, fill=x), a.out(n)
    ok(lib().tq_heun_correct(p(xa), p(xnd), p(den2d), p(dcurd), p(svd, 1), p(svd, 2), p(xa), p(x32a), n, stream()))
    a.verify()
    assert torch.equal(bits(xa.cpu()), bits(xo.cpu())), "x_out aliasing x changes the result"
    assert torch.equal(bits(x32a.cpu()), bits(x32.cpu()))


@pytest.mark.parametrize("s", [EDM_PAIR[0], LATE_PAIR[0]])
@pytest.mark.parametrize("n", SAMPLER_N)
def test_heun_churn(n, s):
    g = gen(n, 4, int(s * 1000))
    s_noise = 1.003
    s32 = torch.tensor(s, dtype=torch.float32)
    shat = s32 + (2 ** 0.5 - 1) * s32
    coef = (shat ** 2 - s32 ** 2).sqrt()          # fp32, as the reference forms it from its 0-dim tensors
    c = Case()
    x = torch.randn(n, generator=g, dtype=torch.float64) * s
    unit = torch.randn(n, generator=g, dtype=torch.float64)
    sv, svd = sigma_vector(c, s, s, float(coef))
    xd, ud = c.inp(x), c.inp(unit)
    xh, x32 = c.out(n, torch.float64), c.out(n)   # (x_hat is a buffer of its own in the sampler)
    ok(lib().tq_heun_churn(p(xd), p(ud), p(svd, 4), s_noise, p(xh), p(x32), n, stream()))
    c.verify()
    inc = (unit * s_noise) * sv[4].double()
    e = state_err(xh.cpu(), x + inc, x.abs() + inc.abs())
    print(f"heun_churn n={n} sigma {s}: {e:.2e}")
    assert e <= BAR_F64
    assert torch.equal(bits(x32.cpu()), bits(xh.cpu().float()))


# ============================================================================================================================
# per-sample scalars
# ============================================================================================================================
SIGMA_DATA = 0.5
SIGMA_MIN = float(np.float32(0.002))   # the value the kernel receives


def edm_scalar_refs(sig):
    from oracle import edm as E
    pp = E.EDMParams(sigma_data=SIGMA_DATA)
    s = sig.double()
    return [E.c_in(pp, s), E.c_out(pp, s), E.c_skip(pp, s), E.c_noise(pp, s), E.loss_weight(pp, s)]


@pytest.mark.parametrize("stride", [1, 0])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_edm_scalars_all_outputs_and_each_null(B, stride):
    g = gen(B, stride, 5)
    sig = log_uniform_sigma(B if stride else 1, g)
    refs = edm_scalar_refs(sig.expand(B))
    names = ["c_in", "c_out", "c_skip", "c_noise", "lweight"]

    def run(null=None):
        c = Case()
        sd = c.inp(torch.cat([torch.full((3,), 9.0), sig, torch.full((2,), 9.0)]))
        outs = [None if i == null else c.out(B) for i in range(5)]
        ok(lib().tq_edm_scalars(p(sd, 3), stride, SIGMA_DATA, *[p(o) for o in outs], B, stream()))
        c.verify()
        return [None if o is None else o.cpu() for o in outs]

    full = run()
    worst = 0.0
    for name, got, ref in zip(names, full, refs):
        e = max_rel(got, ref)
        worst = max(worst, e)
        assert e <= BAR_FEW, f"{name}: {e:.3e}"
    print(f"edm_scalars B={B} stride={stride}: {worst:.2e}")
    for null in range(5):
        part = run(null)
        for i in range(5):
            if i != null:
                assert torch.equal(bits(part[i]), bits(full[i])), f"{names[i]} changes when {names[null]} is NULL"


def cm_scalar_refs(s64):
    """c_out = sigma_data (sigma - sigma_min) / sqrt(sigma_data^2 + sigma^2) and c_skip = sigma_data^2 / ((sigma - sigma_min)^2 +
    sigma_data^2), read off oracle/consistency.py's forward, which returns c_out * net + c_skip * sample: a network of ones on a
    sample of zeros gives c_out, a network of zeros on a sample of ones gives c_skip"""
    from oracle import consistency as OC
    B = s64.numel()
    zero, one = torch.zeros(B, 1, 1, dtype=torch.float64), torch.ones(B, 1, 1, dtype=torch.float64)
    kw = dict(sigma_min=SIGMA_MIN, sigma_data=SIGMA_DATA)
    c_out = OC.forward(lambda x, s, cnd: one, zero, s64, **kw).reshape(B)
    c_skip = OC.forward(lambda x, s, cnd: zero, one, s64, **kw).reshape(B)
    return c_out, c_skip


def run_cm_scalars(sig, B, stride):
    c = Case()
    sd = c.inp(torch.cat([torch.full((3,), 9.0), sig, torch.full((2,), 9.0)]))
    co, cs = c.out(B), c.out(B)
    ok(lib().tq_cm_scalars(p(sd, 3), stride, SIGMA_DATA, SIGMA_MIN, p(co), p(cs), B, stream()))
    c.verify()
    return co.cpu(), cs.cpu()


@pytest.mark.parametrize("stride", [1, 0])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_cm_scalars_and_boundary_condition(B, stride):
    """every case: parity on random sigmas (with one boundary sample among them where there is room), then a launch whose sigmas
    all equal sigma_min, where c_skip == 1 and c_out == 0 must hold exactly: f(x, sigma_min) = x"""
    g = gen(B, stride, 6)
    sig = log_uniform_sigma(B if stride else 1, g)
    if stride and B > 1:
        sig[B - 1] = SIGMA_MIN
    got_co, got_cs = run_cm_scalars(sig, B, stride)
    s64 = sig.expand(B).double()
    co_ref, cs_ref = cm_scalar_refs(s64)
    inner = s64 != SIGMA_MIN
    assert bool(inner.any())
    e = max(max_rel(got_co[inner], co_ref[inner]), max_rel(got_cs[inner], cs_ref[inner]))
    print(f"cm_scalars B={B} stride={stride}: {e:.2e}")
    assert e <= BAR_FEW
    edge_co, edge_cs = run_cm_scalars(torch.full((B if stride else 1,), SIGMA_MIN), B, stride)
    for name, co, cs in (("among random sigmas", got_co[~inner], got_cs[~inner]), ("sigma_min everywhere", edge_co, edge_cs)):
        assert bool((cs == 1.0).all()) and bool((co == 0.0).all()), f"boundary condition at sigma == sigma_min ({name})"


# ============================================================================================================================
# per-sample elementwise
# ============================================================================================================================
def held(got, ref, bar):
    """norm-wise error against the output's largest entry, with rel_err's element-wise criterion asserted inside"""
    e = rel_err(got, ref)
    assert e <= bar, f"{e:.3e} > {bar:g}"
    return e


@pytest.mark.parametrize("per", [1, 257, 16384 + 5])
@pytest.mark.parametrize("B", [1, 3])
def test_edm_noise_inject(B, per):
    from oracle import edm as E
    g = gen(B, per, 7)
    pm, ps = float(np.float32(-1.2)), float(np.float32(1.2))
    y, nz, eps = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g), torch.randn(B, generator=g)
    c = Case()
    yd, nd, ed = c.inp(y), c.inp(nz), c.inp(eps)
    sg, x = c.out(B), c.out(B * per)
    ok(lib().tq_edm_noise_inject(p(yd), p(nd), p(ed), pm, ps, p(sg), p(x), B, per, stream()))
    c.verify()
    s_ref = E.sigma_of_eps(E.EDMParams(P_mean=pm, P_std=ps), eps.double())
    e_s = max_rel(sg.cpu(), s_ref)
    e_x = held(x.cpu(B, per), y.double() + nz.double() * s_ref[:, None], BAR_FEW)
    print(f"edm_noise_inject B={B} per={per}: sigma {e_s:.2e} x {e_x:.2e}")
    assert e_s <= BAR_FEW


@pytest.mark.parametrize("per", [1, 2047, 2049, 5000])
@pytest.mark.parametrize("B", [1, 3])
def test_axpy_sigma(B, per):
    g = gen(B, per, 8)
    x, nz, sig = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g), log_uniform_sigma(B, g)
    c = Case()
    xd, nd, sd = c.inp(x), c.inp(nz), c.inp(sig)
    out = c.out(B * per)
    ok(lib().tq_axpy_sigma(p(xd), p(nd), p(sd), p(out), B, per, stream()))
    c.verify()
    e = held(out.cpu(B, per), x.double() + nz.double() * sig.double()[:, None], BAR_FEW)
    print(f"axpy_sigma B={B} per={per}: {e:.2e}")


@pytest.mark.parametrize("per", [1, 2047, 2049, 5000])
@pytest.mark.parametrize("B", [1, 3])
def test_scale_add2(B, per):
    from oracle import diffusion as D
    g = gen(B, per, 9)
    _, abar = D.schedule()
    t = torch.randint(0, 1000, (B,), generator=g).numpy()
    a, cc = torch.from_numpy(np.sqrt(abar[t])).float(), torch.from_numpy(np.sqrt(1.0 - abar[t])).float()
    x, y = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g)
    c = Case()
    xd, yd, ad, cd = c.inp(x), c.inp(y), c.inp(a), c.inp(cc)
    out = c.out(B * per)
    ok(lib().tq_scale_add2(p(xd), p(yd), p(ad), p(cd), p(out), B, per, stream()))
    c.verify()
    # (the oracle takes sqrt(abar) in float64, the kernel its float32 rounding: 6e-8 of the 2e-6)
    e = held(out.cpu(B, per), D.add_noise(x.double(), y.double(), t, abar), BAR_FEW)
    print(f"scale_add2 B={B} per={per}: {e:.2e}")


@pytest.mark.parametrize("eps_pred", [1, 0])
@pytest.mark.parametrize("n", [1, 1023, 1025, 4100])
def test_ddpm_step(n, eps_pred):
    from oracle import diffusion as D
    g = gen(n, eps_pred, 10)
    _, abar = D.schedule()
    t, prev = 500, 480
    abar_t, abar_p = abar[t], abar[prev]
    alpha_t = abar_t / abar_p
    beta_t = 1.0 - alpha_t
    coef_x0 = np.sqrt(abar_p) * beta_t / (1.0 - abar_t)
    coef_xt = np.sqrt(alpha_t) * (1.0 - abar_p) / (1.0 - abar_t)
    sigma = np.sqrt(max((1.0 - abar_p) / (1.0 - abar_t) * beta_t, 1e-20))
    x, mo, z = 2 * torch.randn(n, generator=g), 2 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    x[0], mo[0] = 3.0, -2.5        # an element that is clipped in both prediction types, whatever n
    ptype = "epsilon" if eps_pred else "sample"
    x0 = (x.double() - np.sqrt(1.0 - abar_t) * mo.double()) / np.sqrt(abar_t) if eps_pred else mo.double()
    assert float(x0.abs().max()) > 1.0
    worst = 0.0
    for clip in (0.0, 1.0):
        for noise in (True, False):
            c = Case()
            xd, md = c.inp(x), c.inp(mo)
            zd = c.inp(z) if noise else None
            out = c.out(n)
            ok(lib().tq_ddpm_step(p(xd), p(md), p(zd), p(out), n, eps_pred, float(np.sqrt(1.0 - abar_t)),
                                  float(1.0 / np.sqrt(abar_t)), clip, float(coef_x0), float(coef_xt), float(sigma), stream()))
            c.verify()
            zz = z.double() if noise else torch.zeros(n, dtype=torch.float64)
            ref = D.ancestral_step(x.double(), mo.double(), t, prev, abar, z=zz, prediction_type=ptype, clip=clip)
            worst = max(worst, held(out.cpu(), ref, BAR_FEW))
    print(f"ddpm_step n={n} {ptype}: {worst:.2e}")


@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("shape", [(2, 3, 2, 7), (3, 3, 3, 4064)])
def test_concat_scale(shape, scaled):
    B, C0, C1, T = shape
    g = gen(B, C0, C1, T, 11)
    x, cs, sc = torch.randn(B, C0, T, generator=g), torch.randn(B, C1, T, generator=g), torch.rand(B, generator=g) + 0.5
    c = Case()
    xd, cd = c.inp(x), c.inp(cs)
    sd = c.inp(sc) if scaled else None
    out = c.out(B * (C0 + C1) * T)
    ok(lib().tq_concat_scale(p(xd), p(sd), p(cd), p(out), B, C0, C1, T, stream()))
    c.verify()
    got = out.cpu(B, C0 + C1, T)
    xs = x.double() * sc.double()[:, None, None] if scaled else x.double()
    e = held(got, torch.cat([xs, cs.double()], 1), BAR_FEW)
    print(f"concat_scale {shape} scale={'given' if scaled else 'NULL'}: {e:.2e}")
    assert torch.equal(bits(got[:, C0:].contiguous()), bits(cs)), "the conditioning signal is copied, not computed"
    if not scaled:
        assert torch.equal(bits(got[:, :C0].contiguous()), bits(x))


# ============================================================================================================================
# losses: every summand is non-negative, so the fp32 accumulation cannot cancel
# ============================================================================================================================
GARBAGE = 12345.678


def loss_runs(call, n_grad):
    """the loss with the gradient output given (twice into the same, garbage-filled loss_out) and NULL; the gradient"""
    c = Case()
    loss, grad = c.out(1, fill=[GARBAGE]), c.out(n_grad)
    call(c, loss, grad)
    c.verify()
    first = float(loss.cpu())
    call(c, loss, grad)
    c.verify()
    second = float(loss.cpu())
    c2 = Case()
    loss2 = c2.out(1, fill=[-GARBAGE])
    call(c2, loss2, None)
    c2.verify()
    return first, second, float(loss2.cpu()), grad.cpu()


def check_loss(name, runs, ref_loss, ref_grad):
    first, second, nograd, grad = runs
    e_l = abs(first - ref_loss) / abs(ref_loss)
    e_again = abs(second - first) / abs(first)
    e_null = abs(nograd - first) / abs(first)
    e_g = rel_err(grad.reshape(ref_grad.shape), ref_grad)
    print(f"{name}: loss {e_l:.2e} again {e_again:.2e} without gradient {e_null:.2e} gradient {e_g:.2e}")
    assert e_l <= BAR_F32, f"loss {first!r} against {ref_loss!r}"
    assert e_again <= BAR_SAME, "loss_out is not zeroed inside the call"
    assert e_null <= BAR_SAME, "the loss depends on whether the gradient is asked for"
    assert e_g <= BAR_FEW


@pytest.mark.parametrize("per", [1, 300, 4096 + 7, 12288])
@pytest.mark.parametrize("B", [1, 5])
def test_edm_loss(B, per):
    from oracle import edm as E
    g = gen(B, per, 12)
    pred, y = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g)
    lw = E.loss_weight(E.EDMParams(sigma_data=SIGMA_DATA), log_uniform_sigma(B, g).double()).float()

    def call(c, loss, grad):
        pd, yd, wd = c.inp(pred), c.inp(y), c.inp(lw)
        ok(lib().tq_edm_loss(p(pd), p(yd), p(wd), p(loss), p(grad), B, per, stream()))

    d = pred.double() - y.double()
    w = lw.double()[:, None]
    check_loss(f"edm_loss B={B} per={per}", loss_runs(call, B * per), float((w * d * d).mean()), 2.0 * w * d / (B * per))


@pytest.mark.parametrize("per", [1, 2049, 5000])
@pytest.mark.parametrize("B", [1, 3])
def test_pseudo_huber_loss(B, per):
    g = gen(B, per, 13)
    target = torch.randn(B, per, generator=g)
    pred = target + 0.05 * torch.randn(B, per, generator=g)    # teacher and student are close, as in training
    wgt = torch.rand(B, generator=g) * 20 + 0.5                # 1 / (sigma_{t+1} - sigma_t) > 0
    cc = float(np.float32(0.00054 * math.sqrt(per)))           # the trainer's c, as the kernel receives it

    def call(c, loss, grad):
        pd, td, wd = c.inp(pred), c.inp(target), c.inp(wgt)
        ok(lib().tq_pseudo_huber_loss(p(pd), p(td), p(wd), cc, p(loss), p(grad), B, per, stream()))

    d = pred.double() - target.double()
    w = wgt.double()[:, None]
    root = (d * d + cc * cc).sqrt()
    check_loss(f"pseudo_huber B={B} per={per}", loss_runs(call, B * per), float((w * (root - cc)).mean()), w * d / root / (B * per))


@pytest.mark.parametrize("n", [1, 257, TWO_TRIPS])
def test_mse_loss(n):
    """tq_mse_loss runs at most 64 workgroups of 1024 threads, eight grid strides per trip, so that the order of their atomic adds
    stays inside the 1e-6 two calls are held to; 524288 + 37 is one full trip of that grid and 37 elements of a second"""
    g = gen(n, 14)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)

    def call(c, loss, grad):
        ad, bd = c.inp(a), c.inp(b)
        ok(lib().tq_mse_loss(p(ad), p(bd), p(loss), p(grad), n, stream()))

    d = a.double() - b.double()
    check_loss(f"mse_loss n={n}", loss_runs(call, n), float((d * d).mean()), 2.0 * d / n)


# ============================================================================================================================
# VAE bottleneck
# ============================================================================================================================
VAE_SHAPES = [(2, 3, 5), (3, 16, 130), (2, 16, 16400)]   # the last: 524800 elements, a second grid-stride trip


def vae_inputs(B, L, T):
    g = gen(B, L, T, 15)
    enc = 0.5 * torch.randn(B, 2 * L, T, generator=g)    # KL terms >= 0, their sum far from zero
    return enc, torch.randn(B, L, T, generator=g), torch.randn(B, L, T, generator=g)


def vae_forward64(enc, eps):
    L = enc.shape[1] // 2
    mean, ls = enc[:, :L], enc[:, L:]
    z = mean + eps * ls.exp()
    kl = (0.5 * (mean ** 2 + (2 * ls).exp() - 2 * ls - 1).sum(1)).mean()
    return z, kl


@pytest.mark.parametrize("shape", VAE_SHAPES)
def test_vae_reparam_fwd(shape):
    B, L, T = shape
    enc, eps, _ = vae_inputs(B, L, T)
    z_ref, kl_ref = vae_forward64(enc.double(), eps.double())
    zs = []
    for with_kl in (True, False):
        c = Case()
        ed, pd = c.inp(enc), c.inp(eps)
        z = c.out(B * L * T)
        kl = c.out(1, fill=[GARBAGE]) if with_kl else None
        ok(lib().tq_vae_reparam_fwd(p(ed), p(pd), p(z), p(kl), B, L, T, stream()))
        c.verify()
        zs.append(z.cpu(B, L, T))
        e_z = held(zs[-1], z_ref, BAR_F32)
        if with_kl:
            e_kl = abs(float(kl.cpu()) - float(kl_ref)) / float(kl_ref)
            print(f"vae_reparam_fwd {shape}: z {e_z:.2e} kl {e_kl:.2e}")
            assert e_kl <= BAR_F32
    assert torch.equal(bits(zs[0]), bits(zs[1])), "z depends on whether the KL term is asked for"


@pytest.mark.parametrize("kl_weight", [1e-6, 0.5])
@pytest.mark.parametrize("shape", VAE_SHAPES)
def test_vae_reparam_bwd(shape, kl_weight):
    B, L, T = shape
    enc, eps, dz = vae_inputs(B, L, T)
    e64 = enc.double().requires_grad_(True)
    z, kl = vae_forward64(e64, eps.double())
    ((z * dz.double()).sum() + float(np.float32(kl_weight)) * kl).backward()
    c = Case()
    ed, pd, dd = c.inp(enc), c.inp(eps), c.inp(dz)
    denc = c.out(B * 2 * L * T)
    ok(lib().tq_vae_reparam_bwd(p(ed), p(pd), p(dd), p(denc), kl_weight, B, L, T, stream()))
    c.verify()
    e = held(denc.cpu(B, 2 * L, T), e64.grad, BAR_F32)
    print(f"vae_reparam_bwd {shape} kl_weight={kl_weight}: {e:.2e}")


# ============================================================================================================================
# embedding
# ============================================================================================================================
PI32 = torch.tensor(math.pi, dtype=torch.float32)
TWO32 = torch.tensor(2.0, dtype=torch.float32)


def fourier_ref(t, W):
    """the argument in float32 in the header's order ((t W) 2) pi -- multiplications only: the kernel's bits -- then sin | cos of
    that float32 value in float64"""
    arg = (((t[:, None] * W[None, :]) * TWO32) * PI32).double()
    return torch.cat([arg.sin(), arg.cos()], 1)


@pytest.mark.parametrize("B,half", [(3, 16), (5, 512), (1, 1)])
def test_fourier_features(B, half):
    g = gen(B, half, 16)
    W = 16 * torch.randn(half, generator=g)
    t = torch.rand(B, generator=g) * 4 - 2
    if B == 3:
        t[0] = 0.0
    c = Case()
    td, Wd = c.inp(t), c.inp(W)
    out = c.out(B * 2 * half)
    ok(lib().tq_fourier_features(p(td), p(Wd), p(out), B, half, stream()))
    c.verify()
    got = out.cpu(B, 2 * half)
    e = float((got.double() - fourier_ref(t, W)).abs().max())
    print(f"fourier_features B={B} half={half}: {e:.2e} (absolute)")
    assert e <= 1e-6     # outputs in [-1, 1]: about 8 ulp of 1 for sinf / cosf built without fast-math
    if B == 3:
        assert bool((got[0, :half] == 0).all()) and bool((got[0, half:] == 1).all())


def silu64(v):
    return v * torch.sigmoid(v)


@pytest.mark.parametrize("B,mc,ncond", [(1, 32, 0), (3, 32, 1), (2, 64, 5), (2, 96, 4), (5, 128, 80), (2, 256, 0)])
def test_embed_fwd(B, mc, ncond):
    """every branch of gemv_rows: scalar rows (ncond 1, 5), float4 rows with one lane per output (mc 32, 64; ncond 4) and with four
    lanes per output (mc 96, 128, 256; ncond 80; every E x E layer)"""
    g = gen(B, mc, ncond, 17)
    E = 4 * mc
    rn = lambda *s: torch.randn(*s, generator=g)
    t = torch.rand(B, generator=g) * 4 - 2
    fw = 16 * rn(mc // 2)
    w0, b0, w2, b2 = rn(E, mc) / math.sqrt(mc), 0.1 * rn(E), rn(E, E) / math.sqrt(E), 0.1 * rn(E)
    if ncond:
        cond = rn(B, ncond)
        cw0, cb0, cw2, cb2 = rn(E, ncond) / math.sqrt(ncond), 0.1 * rn(E), rn(E, E) / math.sqrt(E), 0.1 * rn(E)
    four = fourier_ref(t, fw)
    h0 = four @ w0.double().T + b0.double()
    emb_ref = silu64(h0) @ w2.double().T + b2.double()
    if ncond:
        c0 = cond.double() @ cw0.double().T + cb0.double()
        emb_ref = emb_ref + silu64(c0) @ cw2.double().T + cb2.double()
    results = []
    for with_hidden in (True, False):
        c = Case()
        dv = [c.inp(v) for v in (t, fw, w0, b0, w2, b2)]
        cv = [c.inp(v) for v in (cond, cw0, cb0, cw2, cb2)] if ncond else [None] * 5
        emb, semb = c.out(B * E), c.out(B * E)
        hid = c.out(B * 2 * E) if with_hidden else None
        ok(lib().tq_embed_fwd(p(dv[0]), p(cv[0]), p(dv[1]), p(dv[2]), p(dv[3]), p(dv[4]), p(dv[5]), p(cv[1]), p(cv[2]), p(cv[3]),
                              p(cv[4]), p(emb), p(semb), p(hid), B, mc, ncond, stream()))
        c.verify()
        got_e, got_s = emb.cpu(B, E), semb.cpu(B, E)
        e_e, e_s = held(got_e, emb_ref, BAR_F32), held(got_s, silu64(emb_ref), BAR_F32)
        results.append((got_e, got_s))
        if with_hidden:
            h = hid.cpu(B, 2, E)
            e_h = held(h[:, 0], h0, BAR_F32)
            if ncond:
                e_h = max(e_h, held(h[:, 1], c0, BAR_F32))
            print(f"embed_fwd B={B} mc={mc} ncond={ncond}: emb {e_e:.2e} silu_emb {e_s:.2e} hidden {e_h:.2e}")
    assert torch.equal(bits(results[0][0]), bits(results[1][0])) and torch.equal(bits(results[0][1]), bits(results[1][1])), \
        "emb depends on whether the pre-activations are asked for"


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,E,N", [(1, 128, 1), (17, 128, 65), (5, 256, 200), (16, 508, 64)])   # the last: more than 64 KB of LDS
def test_linear_fwd(B, E, N, with_bias):
    g = gen(B, E, N, 18)
    x, w, bias = torch.randn(B, E, generator=g), torch.randn(N, E, generator=g) / math.sqrt(E), torch.randn(N, generator=g)
    c = Case()
    xd, wd = c.inp(x), c.inp(w)
    bd = c.inp(bias) if with_bias else None
    out = c.out(B * N)
    ok(lib().tq_linear_fwd(p(xd), p(wd), p(bd), p(out), B, E, N, stream()))
    c.verify()
    ref = x.double() @ w.double().T + (bias.double() if with_bias else 0.0)
    e = held(out.cpu(B, N), ref, BAR_F32)
    print(f"linear_fwd B={B} E={E} N={N} bias={'given' if with_bias else 'NULL'}: {e:.2e}")


# ============================================================================================================================
# the small-GEMM job list
# ============================================================================================================================
def dsilu64(u):
    s = torch.sigmoid(u)
    return s * (1 + u * (1 - s))


# (M, N, K), A layout, B layout, pre_b, U, extra columns of C
GEMM_JOBS = [
    ((33, 31, 65), "mk", "kn", 0, False, 5),
    ((33, 31, 65), "km", "nk", 1, True, 3),
    ((1, 70, 3), "ones", "kn", 0, False, 2),    # the bias gradient: a row of ones with sam = 0
    ((64, 32, 32), "km", "kn", 1, False, 0),
    ((5, 5, 1), "mk", "nk", 0, True, 1),
    ((33, 31, 65), "mk", "nk", 0, True, 7),
]


def build_gemm_operands():
    """host operands of GEMM_JOBS with their float64 products, once for the joint launch and the single-job launches"""
    g = gen(19)
    ops = []
    for (M, N, K), la, lb, pre_b, with_u, extra in GEMM_JOBS:
        o = dict(M=M, N=N, K=K, pre_b=pre_b, ldc=N + extra)
        if la == "ones":
            o["A"], o["sam"], o["sak"] = torch.ones(K), 0, 1
            A = torch.ones(M, K, dtype=torch.float64)
        elif la == "mk":                           # row-major with a padded leading dimension: sak == 1
            lda = K + 3
            st = torch.randn(M, lda, generator=g)
            o["A"], o["sam"], o["sak"] = st, lda, 1
            A = st[:, :K].double()
        else:                                      # stored (K, lda >= M): sam == 1, sak = lda
            lda = M + 2
            st = torch.randn(K, lda, generator=g)
            o["A"], o["sam"], o["sak"] = st, 1, lda
            A = st[:, :M].T.double()
        if lb == "kn":                             # row-major (K, ldb >= N): sbn == 1
            ldb = N + 1
            st = torch.randn(K, ldb, generator=g)
            o["B"], o["sbk"], o["sbn"] = st, ldb, 1
            Bm = st[:, :N].double()
        else:                                      # stored (N, ldb >= K): sbk == 1
            ldb = K + 2
            st = torch.randn(N, ldb, generator=g)
            o["B"], o["sbk"], o["sbn"] = st, 1, ldb
            Bm = st[:, :K].T.double()
        ref = A @ (silu64(Bm) if pre_b else Bm)
        o["U"], o["ldu"] = None, 0
        if with_u:
            ldu = N + 4
            o["U"], o["ldu"] = torch.randn(M, ldu, generator=g), ldu
            ref = ref * dsilu64(o["U"][:, :N].double())
        o["ref"] = ref
        ops.append(o)
    return ops


def launch_gemm_jobs(ops):
    """one launch over ``ops`` in the given order; returns the (M, ldc) result of each, guard columns included, and the bits it held
    before the launch"""
    from tqdne_amd import _lib
    L = lib()
    c = Case()
    table = (_lib.TqGemmJob * len(ops))()
    outs, begin = [], 0
    for j, o in enumerate(ops):
        Ad, Bd = c.inp(o["A"]), c.inp(o["B"])
        Ud = c.inp(o["U"]) if o["U"] is not None else None
        Cd = c.out(o["M"] * o["ldc"])
        outs.append(Cd)
        jb = table[j]
        jb.A, jb.B, jb.C, jb.U = p(Ad), p(Bd), p(Cd), p(Ud)
        jb.M, jb.N, jb.K = o["M"], o["N"], o["K"]
        jb.sam, jb.sak, jb.sbk, jb.sbn, jb.ldc, jb.ldu = o["sam"], o["sak"], o["sbk"], o["sbn"], o["ldc"], o["ldu"]
        jb.pre_b, jb.tile_begin = o["pre_b"], begin
        begin += L.tq_gemm_tiles(o["M"], o["N"])
    td = c.inp(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8))
    ok(L.tq_gemm_f32_jobs(p(td), len(ops), begin, stream()))
    c.verify()
    return [(Cd.cpu(o["M"], o["ldc"]), Cd.prefill.cpu().reshape(o["M"], o["ldc"])) for Cd, o in zip(outs, ops)]


def test_gemm_f32_jobs_joint_launch_and_single_job_launches():
    ops = build_gemm_operands()
    joint = launch_gemm_jobs(ops)
    for j, (o, (got, before)) in enumerate(zip(ops, joint)):
        N = o["N"]
        e = held(got[:, :N], o["ref"], BAR_F32)
        print(f"gemm_f32_jobs job {j} {GEMM_JOBS[j][0]} A {GEMM_JOBS[j][1]} B {GEMM_JOBS[j][2]} pre_b={o['pre_b']} "
              f"U={'given' if o['U'] is not None else 'NULL'}: {e:.2e}")
        assert torch.equal(bits(got[:, N:].contiguous()), before[:, N:].contiguous()), f"job {j}: columns beyond N were written"
    # the same jobs in reversed table order, each as a launch of one job: only the job search differs
    for j in reversed(range(len(ops))):
        single = launch_gemm_jobs([ops[j]])[0][0]
        assert torch.equal(bits(single), bits(joint[j][0])), f"job {j} differs between the joint launch and a launch of its own"


# ============================================================================================================================
# backward plumbing, called directly
# ============================================================================================================================
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,T,C", [(2, 1, 4), (3, 129, 36)])
def test_pair_sum(B, T, C, accumulate):
    g = gen(B, T, C, 20)
    dup, dx0 = torch.randn(B, 2 * T, C, generator=g), torch.randn(B, T, C, generator=g)
    c = Case()
    dd = c.inp(dup)
    dx = c.out(B * T * C, fill=dx0)
    ok(lib().tq_pair_sum(p(dd), p(dx), B, T, C, accumulate, stream()))
    c.verify()
    ref = dup[:, 0::2] + dup[:, 1::2]
    if accumulate:
        ref = ref + dx0
    same = torch.equal(bits(dx.cpu(B, T, C)), bits(ref.contiguous()))
    print(f"pair_sum B={B} T={T} C={C} accumulate={accumulate}: {'bit-identical' if same else 'DIFFERENT'}")
    assert same


@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("T_in", [7, 8, 257])
def test_zero_stuff(T_in, C):
    B, T_out = 2, (T_in + 1) // 2
    g = gen(T_in, C, 21)
    dy = torch.randn(B, T_out, C, generator=g)
    c = Case()
    dd = c.inp(dy)
    out = c.out(B * T_in * C)
    ok(lib().tq_zero_stuff(p(dd), p(out), B, T_out, T_in, C, stream()))
    c.verify()
    ref = torch.zeros(B, T_in, C)
    ref[:, 0::2] = dy
    same = torch.equal(bits(out.cpu(B, T_in, C)), bits(ref))
    print(f"zero_stuff T_in={T_in} C={C}: {'bit-identical' if same else 'DIFFERENT'}")
    assert same


@pytest.mark.parametrize("C,T,B", [(32, 1, 1), (32, 1153, 3), (96, 127, 3), (160, 1153, 1), (768, 129, 1), (768, 1153, 3),
                                   (2048, 127, 3), (2048, 1153, 1)])
def test_gn_bwd_finalize(C, T, B):
    """the formulas of the comment above gn_bwd_finalize_kernel in float64: channels per block below and above 128, fewer and more
    slots than sub-sums, the four-slot body and its tail"""
    g = gen(C, T, B, 22)
    ns, G = (T + 127) // 128, C // 32
    gst = torch.randn(B, ns, C, 2, generator=g)
    mr = torch.stack([torch.randn(B, 32, generator=g), torch.rand(B, 32, generator=g) * 4.8 + 0.2], -1)
    gamma = torch.randn(C, generator=g)
    dg0, db0 = torch.randn(C, generator=g) + 2, torch.randn(C, generator=g) - 2
    c = Case()
    gd, md, gmd = c.inp(gst), c.inp(mr), c.inp(gamma)
    cA, cB, cC = c.out(B * C), c.out(B * C), c.out(B * C)
    dg, db = c.out(C, fill=dg0), c.out(C, fill=db0)
    ok(lib().tq_gn_bwd_finalize(p(gd), p(md), p(gmd), B, C, T, p(cA), p(cB), p(cC), p(dg), p(db), stream()))
    c.verify()
    S = gst.double().sum(1)                                   # (B, C, 2)
    S1, S2 = S[..., 0], S[..., 1]
    mean = mr[..., 0].double().repeat_interleave(G, 1)        # (B, C)
    rstd = mr[..., 1].double().repeat_interleave(G, 1)
    gm = gamma.double()[None]
    grp = lambda v: v.reshape(B, 32, G).sum(-1).repeat_interleave(G, 1)
    P1 = grp(gm * S1)
    P2 = rstd * grp(gm * (S2 - mean * S1))
    n = float(G * T)
    refs = [rstd * gm, -rstd ** 2 * P2 / n, rstd ** 2 * P2 * mean / n - rstd * P1 / n,
            dg0.double() + (rstd * (S2 - mean * S1)).sum(0), db0.double() + S1.sum(0)]
    gots = [cA.cpu(B, C), cB.cpu(B, C), cC.cpu(B, C), dg.cpu(), db.cpu()]
    errs = [held(got, ref, BAR_F32) for got, ref in zip(gots, refs)]
    print(f"gn_bwd_finalize C={C} T={T} B={B}: A {errs[0]:.2e} B {errs[1]:.2e} C {errs[2]:.2e} dgamma {errs[3]:.2e} dbeta {errs[4]:.2e}")
