"""Stem and head convs at every first-level width 32, 64, ... 1024 (csrc/ends_wide.hip), the parts that need no GPU: the limit
queries of the three entry points (new shapes supported, old answers unchanged, refusals kept), the new translation unit's kernel
metadata (no scratch, LDS within the limit), and the CPU oracle on the four models the GPU tests hold the HIP path against."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_wide_models_host import LDS_LIMIT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the four models of the GPU tests (tests/test_first_level_widths_gpu.py), on tiny_1d_unet_config() with dropout = 0
MODELS = {
    "mc96": dict(model_channels=96, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(2,), num_heads=3, conv_kernel_size=5),
    "mc160": dict(model_channels=160, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(2,), num_heads=5, conv_kernel_size=3),
    "mc256": dict(model_channels=256, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(2,), num_heads=4, conv_kernel_size=5),
    "mc1024": dict(model_channels=1024, channel_mult=(1,), num_res_blocks=1, attention_resolutions=(), num_heads=4, conv_kernel_size=5),
}
NPARAM = {"mc96": 4120467, "mc160": 8503923, "mc256": 29215107, "mc1024": 113336835}


def width_cfg(which):
    from tqdne_amd import tiny_1d_unet_config
    return dict(tiny_1d_unet_config(), dropout=0.0, **MODELS[which])


# tq_head_conv_lds_bytes before the chunked kernel existed, (C_in, C_out, k) -> bytes, for every shape it supported among
# C_in in {16, 32, 48, 64, 96, 128}, C_out in {1, 3, 6, 16}, k in {1, 3, 5}: (C_in + 128) k maxco floats, maxco = 4 | 16.  The four
# shapes it answered 0 for (C_in = 96 | 128, C_out = 6 | 16, k = 5: 80 and 70 KB) are new ground.
HEAD_LDS_BEFORE = {
    (16, 1, 1): 2304, (16, 1, 3): 6912, (16, 1, 5): 11520, (16, 3, 1): 2304, (16, 3, 3): 6912, (16, 3, 5): 11520,
    (16, 6, 1): 9216, (16, 6, 3): 27648, (16, 6, 5): 46080, (16, 16, 1): 9216, (16, 16, 3): 27648, (16, 16, 5): 46080,
    (32, 1, 1): 2560, (32, 1, 3): 7680, (32, 1, 5): 12800, (32, 3, 1): 2560, (32, 3, 3): 7680, (32, 3, 5): 12800,
    (32, 6, 1): 10240, (32, 6, 3): 30720, (32, 6, 5): 51200, (32, 16, 1): 10240, (32, 16, 3): 30720, (32, 16, 5): 51200,
    (48, 1, 1): 2816, (48, 1, 3): 8448, (48, 1, 5): 14080, (48, 3, 1): 2816, (48, 3, 3): 8448, (48, 3, 5): 14080,
    (48, 6, 1): 11264, (48, 6, 3): 33792, (48, 6, 5): 56320, (48, 16, 1): 11264, (48, 16, 3): 33792, (48, 16, 5): 56320,
    (64, 1, 1): 3072, (64, 1, 3): 9216, (64, 1, 5): 15360, (64, 3, 1): 3072, (64, 3, 3): 9216, (64, 3, 5): 15360,
    (64, 6, 1): 12288, (64, 6, 3): 36864, (64, 6, 5): 61440, (64, 16, 1): 12288, (64, 16, 3): 36864, (64, 16, 5): 61440,
    (96, 1, 1): 3584, (96, 1, 3): 10752, (96, 1, 5): 17920, (96, 3, 1): 3584, (96, 3, 3): 10752, (96, 3, 5): 17920,
    (96, 6, 1): 14336, (96, 6, 3): 43008, (96, 16, 1): 14336, (96, 16, 3): 43008,
    (128, 1, 1): 4096, (128, 1, 3): 12288, (128, 1, 5): 20480, (128, 3, 1): 4096, (128, 3, 3): 12288, (128, 3, 5): 20480,
    (128, 6, 1): 16384, (128, 6, 3): 49152, (128, 16, 1): 16384, (128, 16, 3): 49152,
}


def _queries():
    from tqdne_amd import _lib
    lib = _lib.load()
    assert lib.tq_abi_version() == _lib.ABI_VERSION
    return lib.tq_head_conv_lds_bytes, lib.tq_head_conv_bwd_lds_bytes, lambda c, co, k: lib.tq_stem_conv_lds_bytes(co, c, k)


def test_every_first_level_width_is_supported():
    """every C in 32, 64, ... 1024 x k in (1, 3, 5) x 1 / 3 / 6 / 16 signal channels: head forward, head backward and stem report a
    non-zero LDS size within what a workgroup may declare (no device needed)"""
    for q in _queries():
        for C in range(32, 1025, 32):
            for k in (1, 3, 5):
                for co in (1, 3, 6, 16):
                    assert 0 < q(C, co, k) <= LDS_LIMIT, (C, co, k)
    head_fwd = _queries()[0]
    assert head_fwd(256, 3, 5) > 0   # (0 before the chunked kernel)
    # the chunked head forward leaves room for two workgroups per compute unit
    assert all(head_fwd(C, co, k) <= 64 * 1024 for C in range(160, 1025, 32) for co in range(1, 17) for k in (1, 3, 5))


def test_refusals_are_unchanged():
    for q in _queries():   # (width, signal channels, taps)
        assert q(1056, 3, 5) == 0 and q(256, 17, 5) == 0 and q(256, 3, 7) == 0 and q(256, 0, 5) == 0
    head_fwd, head_bwd, _ = _queries()
    assert head_fwd(40, 3, 5) == 0 and head_fwd(1000, 3, 5) == 0 and head_bwd(1000, 3, 5) == 0


def test_head_query_is_unchanged_for_the_shapes_that_worked():
    from tqdne_amd import _lib
    lib = _lib.load()
    for (cin, cout, k), want in HEAD_LDS_BEFORE.items():
        assert lib.tq_head_conv_lds_bytes(cin, cout, k) == want, (cin, cout, k)


def test_new_translation_unit_uses_no_scratch_and_fits_the_lds(tmp_path):
    """kernel metadata of csrc/ends_wide.hip only: private segment 0 for every kernel; static + the largest dynamic LDS its launchers ask for
    within the limit"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    head_fwd, head_bwd, stem = _queries()
    out = tmp_path / "ends_wide.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-ignored-attributes", "-Wno-cuda-compat",
                    "-S", "--cuda-device-only", "-o", str(out), os.path.join(ROOT, "tqdne_amd", "csrc", "ends_wide.hip")],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    # the widest shapes none of the first kernels take, so the queries answer for the kernels of this translation unit
    dyn = {"stem_wide_kernel": max(stem(992, 16, k) for k in (1, 3, 5)),
           "head_wide_fwd_kernel": max(head_fwd(992, co, k) for co in range(1, 17) for k in (1, 3, 5)),
           "head_wide_bwd_kernel": max(head_bwd(992, co, k) for co in range(1, 17) for k in (1, 3, 5)),
           "rows_sum_kernel": 0}
    seen = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        name, meta = m.group(1), m.group(2)
        assert int(re.search(r"private_segment_fixed_size (\d+)", meta).group(1)) == 0, name   # no scratch
        static = int(re.search(r"group_segment_fixed_size (\d+)", meta).group(1))
        kind = [k for k in dyn if k in name]
        assert len(kind) == 1, name
        assert static + dyn[kind[0]] <= LDS_LIMIT, (name, static, dyn[kind[0]])
        seen[kind[0]] = seen.get(kind[0], 0) + 1
    # stem: k = 1, 3, 5; head forward: 3 tap counts x 1, 2, 3, 4, 6, 8 output channels per launch; head backward: 3 x up to 4, 8, 16
    assert seen == {"stem_wide_kernel": 3, "head_wide_fwd_kernel": 18, "head_wide_bwd_kernel": 9, "rows_sum_kernel": 1}, seen


@pytest.mark.parametrize("which", list(MODELS))
def test_oracle_runs_the_four_models(which):
    """the yardstick of the GPU tests: oracle forward + autograd, finite, on each model at B = 2, T = 200"""
    from oracle import unet as OU
    from tqdne_amd import UNetModel
    cfg = width_cfg(which)
    torch.manual_seed(0)
    m = UNetModel(**cfg)
    sd = m.state_dict()
    assert sum(p.numel() for p in m.parameters()) == NPARAM[which]
    assert sd["input_blocks.0.0.weight"].shape[0] == sd["out.2.weight"].shape[1] == cfg["model_channels"]
    g = torch.Generator().manual_seed(1)
    B, T = 2, 200
    x, t, c = torch.randn(B, 3, T, generator=g), torch.randn(B, generator=g) * 0.5, torch.randn(B, 5, generator=g)
    params = {k: v.clone().requires_grad_(v.is_floating_point() and k != "time_embed.W") for k, v in sd.items()}
    y = OU.unet_forward(params, cfg, x, t, c if cfg.get("cond_features") else None)
    assert y.shape == (B, cfg["out_channels"], T) and torch.isfinite(y).all()
    y.square().mean().backward()
    assert all(torch.isfinite(p.grad).all() for p in params.values() if p.requires_grad and p.grad is not None)
