"""Attention for every head size up to 256, the parts that need no GPU: the tile rule and argument checks of the new entry points, the
resources of their kernels (compiled to gfx950 assembly), and the oracle against the reference's own output for a micro UNet whose
attention runs at head sizes 8 and 16 (tests/golden/head_size_unet.npz, tools/make_head_size_goldens.py)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, cfg_of, rel_err

LDS_LIMIT = 163840   # bytes of LDS one workgroup may declare on gfx950


def load_head_size_unet():
    """weights (stored as the fp16-representable values the reference ran with), config and the recorded runs"""
    z = np.load(os.path.join(GOLDEN, "head_size_unet.npz"), allow_pickle=False)
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    data = {k: z[k] for k in z.files if not k.startswith("w:")}
    return sd, data, cfg_of(data)


def test_tile_rule():
    from tqdne_amd import _lib
    lib = _lib.load()
    assert [lib.tq_attention_head_tile(d) for d in (8, 16, 48, 96, 128, 136, 256)] == [32, 32, 64, 128, 128, 256, 256]
    assert [lib.tq_attention_head_tile(d) for d in (0, 4, 12, 264, 512, -8)] == [0] * 6
    for d in range(8, 257, 8):
        t = lib.tq_attention_head_tile(d)
        assert t in (32, 64, 128, 256) and t >= d and (t == 32 or t // 2 < d)
        assert lib.tq_attention_hd_workspace_bytes(2, 100, 3, d) == 8 * 2 * 3 * 100 * (t + 4) * 4
        assert all(0 < lib.tq_attention_hd_lds_bytes(d, p) <= LDS_LIMIT for p in (0, 1, 2))
    assert lib.tq_attention_hd_lds_bytes(12, 0) == 0 and lib.tq_attention_hd_lds_bytes(512, 2) == 0
    assert lib.tq_attention_hd_lds_bytes(64, 3) == 0
    assert lib.tq_attention_hd_workspace_bytes(2, 100, 3, 12) == 0
    assert _lib.ABI_VERSION == lib.tq_abi_version()


def test_new_entry_points_check_their_arguments_without_a_gpu():
    from tqdne_amd import _lib
    lib = _lib.load()
    fake = 0x1000   # never dereferenced: every call below is rejected during validation
    assert lib.tq_attention_fwd_hd(None, fake, None, None, 2, 128, 4, 48, None) == -1
    assert lib.tq_attention_fwd_hd(fake, None, None, None, 2, 128, 4, 48, None) == -1
    for i in range(6):
        ptrs = [fake] * 6
        ptrs[i] = None
        assert lib.tq_attention_bwd_hd(*ptrs, None, 2, 128, 4, 48, None) == -1, i
    for d in (12, 512, 0, 264):
        assert lib.tq_attention_fwd_hd(fake, fake, None, None, 2, 128, 4, d, None) == -2, d
        assert lib.tq_attention_fwd_hd(fake, fake, fake, fake, 2, 128, 4, d, None) == -2, d
        assert lib.tq_attention_bwd_hd(*[fake] * 6, None, 2, 128, 4, d, None) == -2, d
    for shape in ((0, 128, 4), (2, 0, 4), (2, 128, 0)):
        assert lib.tq_attention_fwd_hd(fake, fake, None, None, *shape, 48, None) == -2
        assert lib.tq_attention_bwd_hd(*[fake] * 6, None, *shape, 48, None) == -2
    # the established entry point keeps its contract
    assert lib.tq_attention_fwd(fake, fake, None, None, 2, 128, 4, 48, None) == -2


def test_new_kernels_use_no_scratch_and_fit_the_lds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from tqdne_amd import _lib
    lib = _lib.load()
    out = tmp_path / "attention_hd.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", "-o", str(out), os.path.join(ROOT, "tqdne_amd", "csrc", "attention_hd.hip")],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    txt = out.read_text()
    static_lds = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, meta = m.group(1), m.group(2)
        assert int(re.search(r"private_segment_fixed_size (\d+)", meta).group(1)) == 0, name   # no spills at all
        static_lds[name] = int(re.search(r"group_segment_fixed_size (\d+)", meta).group(1))
    # (the PAD = true instantiations of the shared first-generation kernels, csrc/attention_g1.hpp)
    passes = {0: "attention_kernel", 1: "attention_bwd_dq_kernel", 2: "attention_bwd_dkv_kernel"}
    seen = 0
    for tile in (32, 64, 128, 256):
        for p, stem in passes.items():
            names = [n for n in static_lds if re.search(rf"\d+{stem}ILi{tile}ELb1EE", n)]
            assert len(names) == 1, (tile, stem, sorted(static_lds))
            dyn = lib.tq_attention_hd_lds_bytes(tile, p)
            assert 0 < dyn and static_lds[names[0]] + dyn <= LDS_LIMIT, (names[0], static_lds[names[0]], dyn)
            seen += 1
    assert seen == 12 and len(static_lds) == 12 + 4 + 1   # + one combine kernel per tile + the delta kernel


@pytest.mark.parametrize("T", [200, 196])
def test_oracle_reproduces_the_reference_at_head_sizes_8_and_16(T):
    from oracle import unet as U
    sd, d, cfg = load_head_size_unet()
    inputs, middle, outputs, _ = U.unet_layout(cfg)
    widths = {l[2] for blk in inputs + [middle] + outputs for l in blk if l[0] == "attn"}
    assert {w // cfg["num_heads"] for w in widths} == {8, 16}
    with torch.no_grad():
        y = U.unet_forward(sd, cfg, torch.from_numpy(d[f"T{T}:x"]), torch.from_numpy(d[f"T{T}:t"]), torch.from_numpy(d[f"T{T}:cond"]))
    assert torch.equal(y, torch.from_numpy(d[f"T{T}:y"]))
