"""1-D UNets wider than the paper's (tensors up to 1024 channels, 2048 concatenated into a conv, qkv projections up to 3072), the parts
that need no GPU: the width limits as the library reports them and the per-site scheme rule built on them, the wide-table translation
units (conv1d_fwd_wide*.hip: no scratch, LDS within what a workgroup may declare), and the CPU oracle on the two models the GPU tests
hold the HIP path against."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 163840   # bytes of LDS a gfx950 workgroup may declare

# the two models of the GPU tests (tests/test_wide_models_gpu.py): parameters, widest conv input / output
PAPER_X2 = dict(model_channels=128, channel_mult=(1, 2, 4, 4), num_res_blocks=2, num_heads=4, attention_resolutions=(8,), conv_kernel_size=5)
W1024 = dict(model_channels=128, channel_mult=(1, 2, 4, 8), num_res_blocks=1, num_heads=4, attention_resolutions=(8,), conv_kernel_size=3)


def wide_cfg(which):
    from tqdne_amd import tiny_1d_unet_config
    base = dict(tiny_1d_unet_config(), dropout=0.0)
    return dict(base, **{"paper_x2": PAPER_X2, "w1024": W1024}[which])


def test_limits_query_and_the_per_site_scheme_rule():
    from tqdne_amd import _lib
    lib = _lib.load()
    assert lib.tq_abi_version() == _lib.ABI_VERSION
    assert lib.tq_conv1d_max_cin(_lib.TQ_WFMT_F16_MX6, 0) >= 2048 and lib.tq_conv1d_max_cin(_lib.TQ_WFMT_BF16X3, 0) >= 2048
    assert lib.tq_conv1d_max_cin(_lib.TQ_WFMT_F16_MX6, 1024) >= 2048 and lib.tq_conv1d_max_cin(_lib.TQ_WFMT_F16_MX6, 128) >= 2048
    assert lib.tq_conv1d_max_cin(_lib.TQ_WFMT_F16_MX6, 64) == lib.tq_conv1d_gn_table_entries(0) == 1024   # the 64-channel tile: established table
    assert lib.tq_conv1d_max_cin(7, 0) == 0
    assert lib.tq_colsum_max_channels() >= 3072 and lib.tq_conv1d_max_cout() >= 3072
    assert lib.tq_conv1d_gn_table_entries(1) == 2048
    # the rule that picks a site's scheme: the fp16-range format for the widest output block ...
    if os.environ.get("TQDNE_CONV_SCHEME", "f16mx6") == "f16mx6" and _lib.WIDE_MX6:
        assert _lib.forward_wfmt(1024, [1024, 1024], k5_act=True) == _lib.TQ_WFMT_F16_MX6
        assert _lib.forward_wfmt(1024, [1024, 512], gn=True) == _lib.TQ_WFMT_F16_MX6
        # ... bf16x3 for that site only where no wide-table tile exists (128 does not divide C_out) ...
        assert _lib.forward_wfmt(576, [576, 576], k5_act=True) == _lib.TQ_WFMT_BF16X3
        assert _lib.forward_wfmt(576, [256, 256], k5_act=True) == _lib.forward_wfmt(576, [256, 0], k5_act=True)
        # ... and no width rule for launches without a GroupNorm prologue (a 1x1 skip conv of the concatenated block input)
        assert _lib.forward_wfmt(1024, [1024, 1024], gn=False) == _lib.TQ_WFMT_F16_MX6
    # narrow sites are untouched by the rule
    assert _lib.forward_wfmt(256, [256, 256], k5_act=True) == _lib.forward_wfmt(256, [256, 0], k5_act=True)


def test_gn_fold_limit_is_the_tiles_own():
    """the consumer-side GroupNorm fold needs 2 C + 64 doubles of the tile's staging buffers: each small tile has its own limit (the
    bf16x3 one of 128 output channels stops below 1024), the wide-table tiles do not fold"""
    from tqdne_amd import _lib
    lib = _lib.load()
    f = lib.tq_conv1d_gn_fold_max_cin
    assert f(_lib.TQ_WFMT_F16_MX6, 32, 256) == 1024 and f(_lib.TQ_WFMT_F16_MX6, 32, 64) == 0
    lims = [f(_lib.TQ_WFMT_BF16X3, 32, c) for c in (32, 64, 128, 256)]
    assert all(0 < a <= b for a, b in zip(lims, lims[1:])) and lims[-1] < 1024 and all(v % 32 == 0 for v in lims)
    assert f(_lib.TQ_WFMT_BF16X3, 0, 256) == 0 and f(_lib.TQ_WFMT_F16_MX8, 32, 256) == 0


@pytest.mark.parametrize("src", ["conv1d_fwd_wide.hip", "conv1d_fwd_wide_k13.hip"])
def test_wide_translation_units_use_no_scratch_and_fit_the_lds(tmp_path, src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from tqdne_amd import _lib
    lib = _lib.load()
    out = tmp_path / (src + ".s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-ignored-attributes", "-Wno-cuda-compat",
                    "-S", "--cuda-device-only", "-o", str(out), os.path.join(ROOT, "tqdne_amd", "csrc", src)],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    txt = out.read_text()
    seen = []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, meta = m.group(1), m.group(2)
        assert int(re.search(r"private_segment_fixed_size (\d+)", meta).group(1)) == 0, name   # no scratch
        static = int(re.search(r"group_segment_fixed_size (\d+)", meta).group(1))
        # conv1d_mfma_kernel<KT, STRIDE, UPS, WM, WN, EPI, ACT, FUSE, SCH, PW, TBW, NCB, GTW>
        a = re.search(r"conv1d_mfma_kernelILi(\d)ELi1ELi0ELi(\d)ELi1ELi0ELi(\d)ELb([01])ELi2ELb0ELi(\d)ELi2ELi(\d+)E", name)
        assert a, name
        kt, wm, act, fuse, tbw, gtw = (int(v) for v in a.groups())
        assert gtw == 2048, name   # nothing but wide-table tiles in these translation units
        c_out, t_tile = (256 if wm == 8 else 128), (32 if tbw == 2 else 0)
        dyn = lib.tq_conv1d_wide_lds_bytes(kt, t_tile, c_out)
        assert dyn >= 2 * 4 * 2048 and static + dyn <= LDS_LIMIT, (name, static, dyn)
        seen.append((kt, wm, tbw, act, fuse))
    if src == "conv1d_fwd_wide.hip":   # k = 5: three tiles x (GN | GN + SiLU | + dropout), the latter two with and without the fused skip conv
        assert len(seen) == len(set(seen)) == 2 * 5 + 4, sorted(seen)
    else:                               # k = 1, 3: two tiles x three prologues
        assert len(seen) == len(set(seen)) == 2 * 2 * 3, sorted(seen)


@pytest.mark.parametrize("which,nparam,cin_max,cout_max", [("paper_x2", 61961027, 1024, 1536), ("w1024", 75185091, 2048, 3072)])
def test_oracle_runs_the_wide_models(which, nparam, cin_max, cout_max):
    """the yardstick of the GPU tests: oracle forward + autograd on both wide models, and their widths"""
    from oracle import unet as OU
    from tqdne_amd import UNetModel
    cfg = wide_cfg(which)
    torch.manual_seed(0)
    m = UNetModel(**cfg)
    sd = m.state_dict()
    assert sum(p.numel() for p in m.parameters()) == nparam
    convs = [v.shape for k, v in sd.items() if v.ndim == 3]
    assert max(s[1] for s in convs) == cin_max and max(s[0] for s in convs) == cout_max
    g = torch.Generator().manual_seed(1)
    B, T = 2, 256
    x, t, c = torch.randn(B, 3, T, generator=g), torch.randn(B, generator=g) * 0.5, torch.randn(B, 5, generator=g)
    params = {k: v.clone().requires_grad_(v.is_floating_point() and k != "time_embed.W") for k, v in sd.items()}
    y = OU.unet_forward(params, cfg, x, t, c if cfg.get("cond_features") else None)
    assert y.shape == (B, cfg["out_channels"], T) and torch.isfinite(y).all()
    y.square().mean().backward()
    assert all(torch.isfinite(p.grad).all() for p in params.values() if p.requires_grad and p.grad is not None)
