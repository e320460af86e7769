"""Stems and heads of 17 ... 64 signal channels (csrc/boundary.hip), the parts that need no GPU: the limit query, the argument checks of
the two boundary entry points, the CPU oracle on the micro models the GPU tests hold the HIP path against, and the oracle against the
reference's recorded outputs for the 16 + 16 -> 16 signal-conditioned model (tests/golden/signal_channels.npz,
tools/make_signal_channel_goldens.py)."""
import pytest
import torch

from conftest import cfg_of, load_golden, rel_err

# the UNets of the GPU tests (tests/test_signal_channels_gpu.py): (in channels, out channels, k, T)
UNETS = {"a": (32, 16, 5, 200), "b": (17, 17, 3, 130), "c": (64, 64, 5, 64), "d": (24, 40, 5, 200)}


def unet_cfg(which):
    cin, cout, k, _ = UNETS[which]
    return dict(in_channels=cin, out_channels=cout, model_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(2,),
                num_heads=4, conv_kernel_size=k, dims=1, cond_features=5, dropout=0.0)


def ae_cfgs(signal=6, latent=16):
    """(encoder config, decoder config) of the micro autoencoder of the latent EDM test"""
    common = dict(model_channels=32, num_res_blocks=1, attention_resolutions=(), channel_mult=(1, 2), conv_kernel_size=3, dims=1,
                  dropout=0.0)
    return dict(common, in_channels=signal, out_channels=2 * latent), dict(common, in_channels=latent, out_channels=signal)


def test_the_limit_query_and_the_abi_number():
    from tqdne_amd import _lib
    lib = _lib.load()
    assert lib.tq_boundary_max_channels() == 64
    assert lib.tq_abi_version() == _lib.ABI_VERSION
    # the dedicated kernels keep their limit: the plans route 17 ... 64 signal channels around them
    assert lib.tq_stem_conv_lds_bytes(17, 32, 5) == 0 and lib.tq_head_conv_lds_bytes(32, 17, 5) == 0
    assert lib.tq_head_conv_bwd_lds_bytes(32, 17, 5) == 0


def test_boundary_entry_points_check_their_arguments_without_a_gpu():
    """TQ_ERR_ARG (-1) / TQ_ERR_SHAPE (-2) before anything touches the device"""
    from tqdne_amd import _lib
    lib = _lib.load()
    fake = 0x1000   # never dereferenced: every call below is rejected during validation
    n2b = lambda x=fake, sc=fake, cond=fake, out=fake, B=2, C0=16, C1=16, T=100, Cp=32: lib.tq_nct_to_btc(x, sc, cond, out, B, C0, C1, T, Cp, None)
    assert n2b(x=None) == -1 and n2b(out=None) == -1
    assert n2b(cond=None) == -1                      # C1 > 0 without a conditioning signal
    assert n2b(C1=0) == -1                           # ... and a conditioning signal with C1 = 0
    assert n2b(B=0) == -1 and n2b(T=0) == -1
    assert n2b(Cp=48) == -2                          # not a multiple of the 32-channel granule
    assert n2b(C0=20, C1=16) == -2                   # C0 + C1 > Cp
    assert n2b(C0=40, C1=25, Cp=96) == -2            # C0 + C1 > 64
    assert n2b(C0=65, C1=0, cond=None, Cp=96) == -2
    assert n2b(C0=0) == -2
    b2n = lambda v=fake, a=fake, s=fake, skip=fake, y=fake, B=2, T=100, Cp=32, c_off=0, C=17: lib.tq_btc_to_nct(v, a, s, skip, y, B, T, Cp, c_off, C, None)
    assert b2n(v=None) == -1 and b2n(y=None) == -1
    assert b2n(s=None) == -1 and b2n(skip=None) == -1   # the skip scale and its source come together
    assert b2n(B=0) == -1 and b2n(T=0) == -1
    assert b2n(Cp=40) == -2
    assert b2n(c_off=16) == -2                       # c_off + C > Cp
    assert b2n(C=65, Cp=96) == -2                    # more than 64 channels
    assert b2n(C=0) == -2 and b2n(c_off=-1) == -2


def _params(cfg, seed):
    from tqdne_amd import UNetModel
    from test_head_sizes_gpu import perturbed_state
    torch.manual_seed(0)
    return perturbed_state(UNetModel(**cfg), seed)


@pytest.mark.parametrize("which", sorted(UNETS))
def test_oracle_runs_the_micro_unets_forward_and_backward(which):
    from oracle import unet as OU
    cfg = unet_cfg(which)
    cin, cout, _, _ = UNETS[which]
    B, T = 2, 200
    g = torch.Generator().manual_seed(3)
    params = {k: v.clone().requires_grad_(k != "time_embed.W") for k, v in _params(cfg, 23).items()}
    x = torch.randn(B, cin, T, generator=g).requires_grad_(True)
    y = OU.unet_forward(params, cfg, x, 0.5 * torch.randn(B, generator=g), torch.randn(B, 5, generator=g))
    assert y.shape == (B, cout, T) and torch.isfinite(y).all()
    y.square().mean().backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    assert all(v.grad is not None and torch.isfinite(v.grad).all() for v in params.values() if v.requires_grad)


def test_oracle_runs_the_signal_conditioned_edm_and_consistency_model():
    from oracle import consistency as OC
    from oracle import edm as OE
    cfg = unet_cfg("a")
    B, T = 2, 200
    g = torch.Generator().manual_seed(4)
    params = {("unet." + k): v.clone().requires_grad_(k != "time_embed.W") for k, v in _params(cfg, 23).items()}
    sample, cs = (0.5 * torch.randn(B, 16, T, generator=g)).requires_grad_(True), torch.randn(B, 16, T, generator=g)
    cond, sigma = torch.randn(B, 5, generator=g), torch.tensor([0.4, 11.0])
    net = OE.make_net(params, cfg)
    y = OE.denoise(OE.EDMParams(), net, sample, sigma, cond_sample=cs, cond=cond)
    assert y.shape == sample.shape and torch.isfinite(y).all()
    y.square().mean().backward()
    assert torch.isfinite(sample.grad).all()
    lo = OE.loss_step(OE.EDMParams(), net, sample.detach(), torch.randn(B, generator=g), torch.randn(B, 16, T, generator=g), cond=cond,
                      cond_sample=cs)
    assert torch.isfinite(lo)
    with torch.no_grad():
        z = OC.forward(net, sample.detach(), sigma, cs, cond)
    assert z.shape == sample.shape and torch.isfinite(z).all()


def test_oracle_runs_the_wide_autoencoder_ends():
    from oracle import autoencoder as OA
    from tqdne_amd import Decoder, Encoder
    B, T = 2, 200
    g = torch.Generator().manual_seed(5)
    _, dec_cfg = ae_cfgs(signal=6, latent=32)
    enc_cfg, _ = ae_cfgs(signal=24, latent=16)
    torch.manual_seed(0)
    dec_sd = {("decoder." + k): v for k, v in Decoder(**dec_cfg).state_dict().items()}
    enc_sd = {("encoder." + k): v for k, v in Encoder(**enc_cfg).state_dict().items()}
    y = OA.decoder_forward(dec_sd, dec_cfg, torch.randn(B, 32, T // 2, generator=g))
    assert y.shape == (B, 6, T) and torch.isfinite(y).all()
    e = OA.encoder_forward(enc_sd, enc_cfg, torch.randn(B, 24, T, generator=g))
    assert e.shape == (B, 32, T // 2) and torch.isfinite(e).all()


def test_oracle_matches_the_references_recorded_outputs():
    """the reference's UNetModel on 32 input channels and its EDM.forward(sample, sigma, cond_sample, cond) with 16 + 16 channels;
    the bar of tests/test_oracle_golden.py"""
    from oracle import edm as OE
    from oracle import unet as OU
    sd, d = load_golden("signal_channels.npz")
    sd = {k: v.float() for k, v in sd.items()}
    cfg = cfg_of(d)
    f = lambda k: torch.from_numpy(d[k]).float()
    with torch.no_grad():
        y = OU.unet_forward(sd, cfg, f("unet:x"), f("unet:t"), f("cond"))
        den = OE.denoise(OE.EDMParams(), OE.make_net({("unet." + k): v for k, v in sd.items()}, cfg), f("edm:sample"), f("edm:sigma"),
                         cond_sample=f("edm:cond_sample"), cond=f("cond"))
    assert rel_err(y, d["unet:y"]) < 1e-6
    assert rel_err(den, d["edm:y"]) < 1e-6
