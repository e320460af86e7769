"""Kernels of different streams share compute units: the sampler integrates four sub-batches on four HIP streams, so every launch
of the plan can run next to any other one.  These tests run launches concurrently and demand bit-identical results.
(Round-2 finding: the first head-conv kernel returned wrong values in the last 16 positions of its tiles whenever an attention
kernel was co-resident; exclusive runs -- all earlier parity tests -- never showed it.)"""

import pytest
import torch

from conftest import rel_err
from test_hip_unet import perturbed_state

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def test_head_conv_next_to_attention_kernels():
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(0)
    B, T, H, D = 16, 512, 4, 64
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(dev())
    dout = torch.randn(B, T, H * D, generator=g).to(dev())
    hx = torch.randn(16, 4096, 64, generator=g).to(dev())
    hb = torch.randn(3, generator=g).to(dev())
    gs = (1 + 0.1 * torch.randn(16, 64, generator=g)).to(dev())
    gh = (0.1 * torch.randn(16, 64, generator=g)).to(dev())
    o_ref, lse = ops.attention(qkv, H, return_lse=True)
    aggressors = [lambda: ops.attention(qkv, H), lambda: ops.attention(qkv, H, workspace=False),
                  lambda: ops.attention_bwd(qkv, o_ref, dout, lse, H)]
    s_a, s_b = torch.cuda.Stream(dev()), torch.cuda.Stream(dev())
    for K in (5, 3, 1):
        hw = (0.1 * torch.randn(3, 64, K, generator=g)).to(dev())
        ref = ops.head_conv(hx, hw, hb, gs, gh).clone()
        cpu = torch.nn.functional.conv1d(torch.nn.functional.silu(hx.cpu() * gs.cpu()[:, None, :] + gh.cpu()[:, None, :]).permute(0, 2, 1),
                                         hw.cpu(), hb.cpu(), padding=K // 2)
        assert rel_err(ref.cpu(), cpu) < 1e-5
        torch.cuda.synchronize()
        for afn in aggressors:
            outs = []
            for _ in range(3):
                for _ in range(8):
                    with torch.cuda.stream(s_b):
                        afn()
                    with torch.cuda.stream(s_a):
                        outs.append(ops.head_conv(hx, hw, hb, gs, gh))
                torch.cuda.synchronize()
            assert all(torch.equal(o, ref) for o in outs), f"head conv k={K} changed its result next to a concurrent attention kernel"


def test_four_plans_on_four_streams_match_a_plan_alone():
    """the paper UNet forward of 16 samples on 4 plans / 4 streams at once, three times in a row: every intermediate activation,
    every statistic and the output must equal those of a plan that ran alone"""
    from tqdne_amd import LightningEDM, paper_1d_unet_config
    torch.manual_seed(0)
    edm = LightningEDM(paper_1d_unet_config(), {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0})
    edm.unet.load_state_dict(perturbed_state(edm.unet, 17))
    edm = edm.to(dev()).eval()
    T, h, L = 4096, 16, 4
    g = torch.Generator().manual_seed(1)
    x = (3.0 * torch.randn(h, 3, T, generator=g)).to(dev())
    cond = torch.randn(h, 5, generator=g).to(dev())
    sig = torch.full((h,), 2.0, device=dev())
    streams = [torch.cuda.current_stream(dev())] + [torch.cuda.Stream(dev()) for _ in range(L - 1)]

    def fwd(lane):
        with torch.no_grad():
            return edm._denoise_static(x, sig, 1, cond, infer=True, lane=lane)

    def tensors(eng):
        # (inference plans write only the q third of a qkv buffer: K and V go straight to the attention kernel's bf16 planes)
        qkv = {id(t["qkv"]) for kind, t in eng.tape if kind == "attn"}
        out = [("out", eng.out_nct)]
        for i, a in enumerate(eng.acts):
            out.append((f"act{i}", a.buf[:, :, : a.C // 3] if id(a) in qkv else a.buf))
            if a.stats is not None:
                out.append((f"act{i}.stats", a.stats))
        return out

    for lane in range(L):
        fwd(lane)
    torch.cuda.synchronize()
    ref = [t.clone() for _, t in tensors(edm.unet._engine(h, T, dev(), 0))]
    for it in range(6):
        for s in streams[1:]:
            s.wait_stream(streams[0])
        for _ in range(3):
            for lane, s in enumerate(streams):
                with torch.cuda.stream(s):
                    fwd(lane)
        torch.cuda.synchronize()
        for lane in range(L):
            for (name, t), r in zip(tensors(edm.unet._engine(h, T, dev(), lane)), ref):
                assert torch.equal(t, r), f"round {it}, lane {lane}: {name} differs from the run alone"


def test_sampler_lanes_are_deterministic_at_the_bench_batch():
    from oracle import edm as OE
    from tqdne_amd import LightningEDM, paper_1d_unet_config
    torch.manual_seed(0)
    edm = LightningEDM(paper_1d_unet_config(), {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}, num_sampling_steps=18)
    edm.unet.load_state_dict(perturbed_state(edm.unet, 17))
    edm = edm.to(dev()).eval()
    B, T = 64, 4096
    g = torch.Generator().manual_seed(1234)
    start = torch.randn(B, 3, T, generator=g, dtype=torch.float64)
    cond = torch.randn(B, 5, generator=g).to(dev())
    sig = OE.sampling_sigmas(OE.EDMParams(), 18)
    eps = (start * sig[0]).to(dev())
    s3 = sig[:4].to(dev())   # 3 Heun steps = 6 UNet evaluations per lane
    runs = [edm.sample_deterministically(eps, s3, None, cond, lanes=n).clone() for n in (4, 4, 1, 2)]
    assert torch.equal(runs[0], runs[1]), "two 4-lane integrations differ: a race between the lanes"
    assert torch.equal(runs[0], runs[2]) and torch.equal(runs[0], runs[3]), "lanes change the result"


def test_training_step_next_to_other_streams():
    """The data-parallel trainer starts the gradient all-reduce from inside the backward sweep: RCCL's kernels then share compute
    units with the weight- / data-gradient, GroupNorm-backward and attention-backward launches.  The 1-GPU box cannot run RCCL
    between two ranks, so other kernels play that part here: a second stream keeps attention kernels (the aggressors that exposed
    the head-conv fault) and streaming copies / reductions over an all-reduce-sized buffer in flight while the main stream runs
    the paper UNet's training step (dropout on).  Gradients written by plain stores must be bit-identical to the quiet run; the
    few that are accumulated by fp32 atomics (bias column sums, GroupNorm affine) to rounding."""
    from tqdne_amd import LightningEDM, ops, paper_1d_unet_config, rng
    from tqdne_amd.autograd import edm_loss_and_grads
    torch.manual_seed(0)
    edm = LightningEDM(paper_1d_unet_config(), {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0})
    edm.unet.load_state_dict(perturbed_state(edm.unet, 17))
    edm = edm.to(dev()).train()
    B, T = 8, 4096
    g = torch.Generator().manual_seed(5)
    x = (0.5 * torch.randn(B, 3, T, generator=g)).to(dev())
    cond = torch.randn(B, 5, generator=g).to(dev())
    eps, noise = torch.randn(B, generator=g).to(dev()), torch.randn(B, 3, T, generator=g).to(dev())
    qkv = torch.randn(16, 512, 768, generator=g).to(dev())
    dout = torch.randn(16, 512, 256, generator=g).to(dev())
    o_ref, lse = ops.attention(qkv, 4, return_lse=True)
    big = torch.randn(16 << 20, generator=g).to(dev())   # 64 MB: the flat gradient buffer's size
    big2 = torch.empty_like(big)

    def step():
        rng.seed_rank(3, 0)   # same dropout masks every time
        loss, flat = edm_loss_and_grads(edm, x, eps, noise, cond, lanes=1)
        bwd = edm.unet._engine(B, T, dev())._bwd
        return float(loss), flat[:bwd.n_grad].clone(), bwd

    loss0, g0, bwd = step()
    loss1, g1, _ = step()
    torch.cuda.synchronize()
    atomic = set()   # gradients accumulated with fp32 atomics: their bits depend on the arrival order even in a quiet run
    for name, p in edm.unet.named_parameters():
        o = bwd.offs[id(p)]
        if not torch.equal(g0[o:o + p.numel()], g1[o:o + p.numel()]):
            atomic.add(name)
    # by design (backward.hip): bias / embedding column sums, GroupNorm affine, embedding MLPs (fed by those sums), and the stem / head
    # weights (3-channel convs, accumulated over the batch with atomics)
    by_design = lambda n: (n.endswith(".bias") or ".in_layers.0." in n or ".out_layers.0." in n or ".norm." in n or n.startswith("out.0.")
                           or "emb" in n or "mlp" in n or n in ("input_blocks.0.0.weight", "out.2.weight"))
    assert all(by_design(n) for n in atomic), sorted(n for n in atomic if not by_design(n))[:8]
    atomic = {n for n, _ in edm.unet.named_parameters() if by_design(n)}   # (two quiet runs may agree by chance: judge all of them to rounding)
    side = torch.cuda.Stream(dev())
    aggressors = [lambda: ops.attention(qkv, 4), lambda: ops.attention_bwd(qkv, o_ref, dout, lse, 4),
                  lambda: big2.copy_(big), lambda: big2.add_(big), lambda: torch.sum(big)]
    for rep in range(3):
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(side):
            for _ in range(40):   # ~40 ms of foreign kernels: longer than the step
                for a in aggressors:
                    a()
        loss, gr, _ = step()
        torch.cuda.synchronize()
        assert loss == pytest.approx(loss0, rel=1e-6)
        worst = 0.0
        for name, p in edm.unet.named_parameters():
            o = bwd.offs[id(p)]
            a, b = gr[o:o + p.numel()], g0[o:o + p.numel()]
            if name in atomic:
                worst = max(worst, float((a - b).abs().max()) / max(float(b.abs().max()), 1e-4 * float(g0.abs().max())))
            else:
                assert torch.equal(a, b), f"round {rep}: gradient of {name} changed next to foreign kernels"
        assert worst < 1e-4, worst


def test_stochastic_sampler_lanes_are_bit_identical_and_match_the_oracle():
    """Round 5: the churned sampler (edm.py:198-230) on the lanes of the deterministic one.  Micro UNet, B = 32 (two lanes of 16), 4 steps
    with injected unit noises: lanes = 2 / 4 integrate exactly what one lane does, and that is the oracle's result; with the sampler's
    own draws (same torch seed) lanes and one lane agree as well (the noises are drawn for the whole batch in the one-lane order)."""
    from conftest import cfg_of, load_golden
    from oracle import edm as OE
    from tqdne_amd import LightningEDM
    sd, d = load_golden("micro_unet.npz")
    cfg = cfg_of(d)
    nsteps = 4
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}, num_sampling_steps=nsteps, deterministic_sampling=False)
    edm.unet.load_state_dict(sd)
    dev = torch.device("cuda:0")
    edm = edm.to(dev).eval()
    g = torch.Generator().manual_seed(77)
    B, T = 32, 256
    start = torch.randn(B, 3, T, generator=g, dtype=torch.float64)
    cond = torch.randn(B, 5, generator=g)
    churn = [torch.randn(B, 3, T, generator=g, dtype=torch.float64) for _ in range(nsteps)]
    sig = OE.sampling_sigmas(OE.EDMParams(), nsteps)
    eps = (start * sig[0]).to(dev)
    outs = {n: edm.sample_stochastically(eps, sig.to(dev), None, cond.to(dev), churn_noises=[c.to(dev) for c in churn], lanes=n).clone()
            for n in (1, 2, 4, 2)}
    # (2 and 4 lanes run the same tiles on every layer: bit-identical; the one-lane plan of this small shape has the device to itself and
    # takes the 32-position tile on its deep levels -- another association of the GroupNorm sums: equal to rounding)
    assert torch.equal(outs[2], outs[4])
    assert rel_err(outs[1].cpu(), outs[2].cpu()) < 1e-5
    net = OE.make_net({"unet." + k: v for k, v in sd.items()}, cfg)
    with torch.no_grad():
        ref = OE.sample_stochastic(OE.EDMParams(), net, start, churn, nsteps, cond=cond)
    e = rel_err(outs[2].cpu(), ref)
    print(f"stochastic sampler, 2 lanes x 16, {nsteps} steps vs oracle: {e:.2e}")
    assert e < 1e-3
    res = {}
    for n in (1, 2, 4):
        torch.manual_seed(5)
        res[n] = edm.sample_stochastically(eps, sig.to(dev), None, cond.to(dev), lanes=n).clone()
    assert torch.equal(res[2], res[4]) and rel_err(res[1].cpu(), res[2].cpu()) < 1e-5, "the lanes' draws must be the one-lane loop's draws"
    # round 6 (advisor): a step's noise is drawn when the first lane reaches the step and dropped after the last lane took its slice --
    # the same bits as the same draws made up front, and never more than one step alive at a time while the host enqueues
    torch.manual_seed(5)
    upfront = [torch.randn(B, 3, T, dtype=torch.float64, device=dev) for _ in range(nsteps)]
    assert torch.equal(edm.sample_stochastically(eps, sig.to(dev), None, cond.to(dev), churn_noises=upfront, lanes=2), res[2])
    peak = []
    cls = type(edm)._StepNoises
    orig = cls.take

    def take(self, *a):
        out = orig(self, *a)
        peak.append(len(self.live))
        return out
    cls.take = take
    try:
        torch.manual_seed(5)
        again = edm.sample_stochastically(eps, sig.to(dev), None, cond.to(dev), lanes=4)
    finally:
        cls.take = orig
    assert torch.equal(again, res[4]) and max(peak) <= 1 and len(peak) == 4 * nsteps
