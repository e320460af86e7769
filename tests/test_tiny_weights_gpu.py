"""The start a real run has: the zero_module tensors (each ResBlock's out conv, each attention block's proj_out, the final conv) are
KEPT where every golden and every other parity test re-draws them, and set to s * randn for s in {0, 1e-4, 1e-7, 1e-9} -- the
initial state, Adam after one step, and the first un-rectified RAdam steps at the upper and lower gradient scale.  One forward +
backward on the HIP path against oracle/unet.py in float64 on the CPU, from the same state dict and inputs, at the suite's bars:
forward rel_err < 1e-3, every parameter gradient through conftest.grad_err (1e-3 floored, GRAD_OWN_TOL on its own scale).

Two configurations: the micro UNet of tests/golden/micro_unet.npz (its configuration only; 32 / 64 channels, so its zero_module convs
run in bf16x3 whatever the scheme) and the same with 128 model channels, whose ResBlock and attention convs and their data gradients run
in the default fp16 + MX-fp6 scheme.  The default scheme runs in-process, TQDNE_CONV_SCHEME=bf16x3 in a fresh child process (it shows
that the reference side of the comparison is sound).

What those bars do not see: gradients below GRAD_OWN_FROM of the largest one are held to the floored metric only, and behind a conv
whose weights are ~s everything upstream in its block is s (s^2 with the final conv) times smaller -- while RAdam / Adam divide a
gradient by its own running scale, so its RELATIVE error is what the update sees.  Hence a third figure, asserted too: the worst error
on a tensor's OWN scale over the weight tensors (2-D and 3-D: sums of products; biases and GroupNorm affines in front of a normalisation
are sums that cancel, fp32 noise on their own scale in any scheme) whose reference gradient reaches OWN_FROM_S2 * s^2 of the largest one
(below that the tensor is exactly zero in exact arithmetic -- a projection in front of a one-channel GroupNorm group -- and the float64
reference holds rounding noise).  bf16x3 at every s, and the default scheme at s = 1e-4, must keep it below GRAD_OWN_TOL.  The default
scheme at s = 1e-7 and 1e-9 CANNOT: the data gradient through a conv whose weights are below fp16's normal range loses them
(include/tqdne_hip.h, TQ_WFMT_F16_MX6: weight operand) -- measured 9.2e-3 and 5.1e-2 on the 128-channel model (bf16x3: 2.4e-5) -- and is
held to what the bit-model predicts for that conv (model against exact, times the margin of 4) instead; DESIGN.md section 8 says so."""

import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import GRAD_OWN_TOL, cfg_of, grad_err, load_golden, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3
S_VALUES = (0.0, 1e-4, 1e-7, 1e-9)
CONFIGS = ("micro", "wide128")
OWN_FROM_S2 = 1e-3
ZERO_MODULE = (".out_layers.3.weight", ".out_layers.3.bias", ".proj_out.weight", ".proj_out.bias", "out.2.weight", "out.2.bias")


def _cfg(which):
    _, d = load_golden("micro_unet.npz")
    cfg = dict(cfg_of(d), dropout=0.0)
    if which == "wide128":
        cfg.update(model_channels=128, channel_mult=(1, 2), attention_resolutions=(2,))
    return cfg


def _state(cfg, s):
    from tqdne_amd import UNetModel
    torch.manual_seed(7)
    m = UNetModel(**cfg)
    g = torch.Generator().manual_seed(11)
    sd = {}
    for k, v in m.state_dict().items():
        v = v.clone()
        if k.endswith(ZERO_MODULE):
            assert torch.count_nonzero(v) == 0, k     # zero_module tensors of a fresh model
            v = s * torch.randn(v.shape, generator=g)
        sd[k] = v
    assert sum(k.endswith(ZERO_MODULE) for k in sd) >= 10
    return m, sd


def predicted_own_error(s):
    """error of the fp16 + MX-fp6 data gradient through a k = 5 conv of 128 channels whose weights are s * randn, by the bit-model:
    max|model - exact| / max|exact| on O(1) dy (the kernel scales dy into range whatever its size)"""
    import numpy as np
    from oracle import contraction as M
    rng = np.random.default_rng(0)
    w = (rng.standard_normal((128, 128, 5)) * s).astype(np.float32)
    dy = rng.standard_normal((1, 64, 128)).astype(np.float32)
    ex = M.dgrad_exact(dy, w)
    word = int(np.abs(dy).max().view(np.uint32))
    return float(np.abs(M.dgrad_model(dy, w, M.F16_MX6, word) - ex).max() / np.abs(ex).max())


def own_bar(s):
    from tqdne_amd import _lib
    if _lib.requested_scheme() == "f16mx6" and s in (1e-7, 1e-9):
        return 4 * predicted_own_error(s)
    return GRAD_OWN_TOL


def run_case(which, s):
    """figures of one case, asserted: (forward error, worst floored gradient error, worst own-scale error over all tensors)"""
    from oracle import unet as OU
    cfg = _cfg(which)
    m, sd = _state(cfg, s)
    m.load_state_dict(sd)
    dev = torch.device("cuda:0")
    m = m.to(dev).train()
    g = torch.Generator().manual_seed(41)
    B, T = 2, 256
    x = torch.randn(B, 3, T, generator=g)
    t = torch.randn(B, generator=g) * 0.5
    c = torch.randn(B, 5, generator=g)
    tgt = torch.randn(B, 3, T, generator=g)   # (y itself is ~s: its square alone would leave no gradient at s = 0)
    y = m(x.to(dev), t.to(dev), c.to(dev))
    (y - tgt.to(dev)).square().mean().backward()
    ref = {k: v.double().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
    yo = OU.unet_forward(ref, cfg, x.double(), t.double(), c.double())
    (yo - tgt.double()).square().mean().backward()
    yc = y.detach().cpu()
    assert torch.isfinite(yc).all()
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.requires_grad}
    assert len(grads) == len(sd) - 1 and all(torch.isfinite(v).all() for v in grads.values())
    gmax = max(float(v.grad.abs().max()) for v in ref.values() if v.grad is not None)
    if s == 0.0:
        # nothing but the final conv sees a gradient: exact zeros in the oracle are exact zeros here, the output is the final bias (0)
        assert float(yo.detach().abs().max()) == 0.0 and float(yc.abs().max()) == 0.0
        nz = 0
        for n, gv in grads.items():
            if float(ref[n].grad.abs().max()) == 0.0:
                assert float(gv.abs().max()) == 0.0, n
                nz += 1
        assert nz == len(grads) - 2, nz
        fwd = 0.0
    else:
        fwd = rel_err(yc, yo.detach())
        assert fwd < TOL, (which, s, fwd)
    worst, wname, own, oname, ofrac, nown = 0.0, "", 0.0, "", 0.0, 0
    for n, gv in grads.items():
        r = ref[n].grad
        e = grad_err(gv, r, gmax, n)
        if e > worst:
            worst, wname = e, n
        rmax = float(r.abs().max())
        if s > 0 and r.ndim >= 2 and rmax >= OWN_FROM_S2 * s * s * gmax:
            o = float((gv.double() - r).abs().max()) / rmax
            nown += 1
            if o > own:
                own, oname, ofrac = o, n, rmax / gmax
    bar = own_bar(s)
    print(f"TINY {which} s={s:g} scheme={os.environ.get('TQDNE_CONV_SCHEME', 'default')}: forward {fwd:.2e}; worst floored gradient "
          f"error {worst:.2e} ({wname}); worst own-scale error {own:.2e} ({oname}, {ofrac:.1e} of the largest gradient; {nown} of "
          f"{len(grads)} tensors; bar {bar:.2e})")
    assert worst < TOL, (which, s, worst, wname)
    assert own <= bar, (which, s, own, oname, bar)
    return fwd, worst, own


@pytest.mark.parametrize("s", S_VALUES)
@pytest.mark.parametrize("which", CONFIGS)
def test_true_start_default_scheme(which, s):
    run_case(which, s)


def test_true_start_bf16x3_in_a_fresh_process():
    """the same cases with TQDNE_CONV_SCHEME=bf16x3 (read when the library layer is imported: a child process)"""
    env = dict(os.environ, TQDNE_CONV_SCHEME="bf16x3", TQDNE_PARITY_LOG="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    done = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(done) == len(CONFIGS) * len(S_VALUES)


if __name__ == "__main__":
    out = [(w, s) + tuple(run_case(w, s)) for w in CONFIGS for s in S_VALUES]
    print(json.dumps(out))
