"""conv_resample=False (parameter-free resampling) and cond_emb_scale (Fourier projection of the one conditioning feature): what can be
held without a GPU -- constructors, state_dict schema and same-seed initialisation against the reference's recorded ones
(tests/golden/plain_resample.npz, tools/make_plain_resample_goldens.py), the refusals that stay, the argument checks of the three new
C entry points, and the dims=2 family on the CPU."""
import os
import sys

import pytest
import torch

from conftest import ROOT, cfg_of, load_golden, rel_err

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_plain_resample_goldens import recipe_state, tensor_fingerprint  # noqa: E402

TOL_2D = 2e-5   # tests/test_family2d.py: plain torch arithmetic on both sides


@pytest.fixture(scope="module")
def fx():
    return load_golden("plain_resample.npz")[1]


def seeds(d):
    return eval(str(d["seeds"]), {"__builtins__": {}}, {"dict": dict})


def assert_schema(module, d, tag):
    sd = module.state_dict()
    assert list(sd) == [str(k) for k in d[tag + ":keys"]]
    assert [" ".join(str(int(s)) for s in v.shape) for v in sd.values()] == [str(s) for s in d[tag + ":shapes"]]


def load_recipe(module, d, tag, seed):
    """the weights the reference ran with: rebuilt from the recipe, held to the fixture's fingerprints, loaded"""
    sd = recipe_state(module, seed)
    assert [tensor_fingerprint(v) for v in sd.values()] == [str(s) for s in d[tag + ":sha256"]]
    module.load_state_dict(sd)
    return module


def test_unet_without_resampling_convs_has_the_reference_schema(fx):
    from tqdne_amd import UNetModel
    from tqdne_amd.unet import DownsampleParams, UpsampleParams
    net = UNetModel(**cfg_of(fx, "cfg:unet"))
    assert_schema(net, fx, "unet")
    assert not [k for k in net.state_dict() if ".op." in k or ".conv." in k]
    plain = [m for m in net.modules() if isinstance(m, (DownsampleParams, UpsampleParams))]
    assert len(plain) == 4 and all(not m.use_conv and not list(m.parameters()) for m in plain)
    learned = UNetModel(**dict(cfg_of(fx, "cfg:unet"), conv_resample=True))
    assert len([k for k in learned.state_dict() if ".op." in k or ".conv." in k]) == 8   # (the default is what it was)
    load_recipe(net, fx, "unet", seeds(fx)["unet"])


def test_coders_without_resampling_convs_have_the_reference_schema(fx):
    from tqdne_amd import LightningAutoencoder
    ae = LightningAutoencoder(cfg_of(fx, "cfg:enc"), cfg_of(fx, "cfg:dec"), {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0})
    assert_schema(ae, fx, "ae")
    assert not [k for k in ae.state_dict() if ".op." in k or ".conv." in k]
    assert ae.encoder.time_scale == 4
    load_recipe(ae, fx, "ae", seeds(fx)["ae"])


def test_cond_emb_scale_schema_and_same_seed_initialisation(fx):
    from tqdne_amd import UNetModel
    cfg = cfg_of(fx, "cfg:cf")
    torch.manual_seed(int(fx["cf:init:seed"]))
    net = UNetModel(**cfg)
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in fx["cf:init:keys"]]
    mc = cfg["model_channels"]
    assert list(sd).index("cond_embed.W") == list(sd).index("cond_mlp.0.weight") - 1 == list(sd).index("time_mlp.2.bias") + 1
    assert tuple(net.cond_embed.W.shape) == (mc // 2,) and not net.cond_embed.W.requires_grad
    assert tuple(net.cond_mlp[0].weight.shape) == (4 * mc, mc)
    want = dict(zip((str(k) for k in fx["cf:init:keys"]), (str(s) for s in fx["cf:init:sha256"])))
    for k, v in sd.items():   # cond_embed.W is drawn between time_mlp and cond_mlp: everything behind it moves if it is not
        assert tensor_fingerprint(v) == want[k], k
    assert_schema(net, fx, "cf")
    load_recipe(net, fx, "cf", seeds(fx)["cf"])


def test_cond_emb_scale_takes_exactly_one_conditioning_feature(fx):
    from tqdne_amd import UNetModel
    cfg = cfg_of(fx, "cfg:cf")
    for dims in (1, 2):
        for feats in (5, None):
            with pytest.raises(NotImplementedError, match="reference"):
                UNetModel(**dict(cfg, dims=dims, cond_features=feats))


def test_options_that_stay_refused(fx):
    from tqdne_amd import UNetModel
    cfg = cfg_of(fx, "cfg:unet")
    for kw in (dict(use_scale_shift_norm=True), dict(use_causal_mask=True), dict(dims=3)):
        with pytest.raises(NotImplementedError):
            UNetModel(**dict(cfg, **kw))


def test_new_entry_points_check_their_arguments_without_a_gpu():
    from tqdne_amd import _lib
    lib = _lib.load()
    assert lib.tq_abi_version() == _lib.ABI_VERSION
    fake = 0x1000   # never dereferenced: every call below is rejected during validation
    for fn in (lib.tq_avg_pool2_fwd, lib.tq_nearest_up2_fwd):
        assert fn(None, fake, fake, 2, 8, 32, None) == -1
        assert fn(fake, None, fake, 2, 8, 32, None) == -1
        for T_in, C in ((8, 6), (8, 1028), (1, 32)):
            assert fn(fake, fake, fake, 2, T_in, C, None) == -2, (T_in, C)
            assert fn(fake, fake, None, 2, T_in, C, None) == -2, (T_in, C)
    assert lib.tq_avg_pool2_bwd(None, fake, 2, 8, 32, 0, None) == -1
    assert lib.tq_avg_pool2_bwd(fake, None, 2, 8, 32, 1, None) == -1
    for T_in, C in ((8, 6), (8, 1028), (1, 32)):
        assert lib.tq_avg_pool2_bwd(fake, fake, 2, T_in, C, 0, None) == -2, (T_in, C)
    assert {"tq_avg_pool2_fwd", "tq_nearest_up2_fwd", "tq_avg_pool2_bwd"} <= set(_lib.exported_symbols())


@pytest.mark.parametrize("tag", ["2d", "2dcf"])
def test_dims2_family_on_the_cpu(fx, tag):
    import warnings
    from tqdne_amd import UNetModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = UNetModel(**cfg_of(fx, "cfg:" + tag)).eval()
    assert_schema(net, fx, tag)
    assert not [k for k in net.state_dict() if ".op." in k or ".conv." in k]
    load_recipe(net, fx, tag, seeds(fx)["d2" if tag == "2d" else "d2cf"])
    cond = torch.from_numpy(fx["unet:cond"] if tag == "2d" else fx["cf:cond"])
    with torch.no_grad():
        y = net(torch.from_numpy(fx["2d:x"]).float(), torch.from_numpy(fx["unet:t"]), cond)
    assert rel_err(y, fx[tag + ":y"]) < TOL_2D


def test_dims2_coders_accept_plain_resampling():
    import warnings
    from tqdne_amd.autoencoder import Decoder, Encoder
    kw = dict(model_channels=32, channel_mult=(1, 2), attention_resolutions=(), num_res_blocks=1, dims=2, conv_resample=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc, dec = Encoder(1, out_channels=4, **kw).eval(), Decoder(2, out_channels=1, **kw).eval()
    assert not [k for k in list(enc.state_dict()) + list(dec.state_dict()) if ".op." in k or ".conv." in k]
    x = torch.randn(2, 1, 16, 12, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        e = enc(x)
        assert tuple(e.shape) == (2, 4, 8, 6)
        assert tuple(dec(e[:, :2]).shape) == (2, 1, 16, 12)
