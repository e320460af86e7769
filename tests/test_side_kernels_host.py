"""Argument checks of the side kernels' entry points, without a GPU: a NULL required pointer or a non-positive size is answered with
TQ_ERR_ARG / TQ_ERR_SHAPE before the device is touched.  The pointers below are never dereferenced: every call in this file is
rejected in validation, none reaches a launch.  Companion of tests/test_side_kernels_gpu.py."""

import pytest

ARG, SHAPE = -1, -2
FAKE = 0x1000


def lib():
    from tqdne_amd import _lib
    return _lib.load()


def variants(good, pointers, sizes, bad_size=0):
    """``good`` with each required pointer in turn NULL, then with each size in turn non-positive"""
    for i in pointers:
        a = list(good)
        a[i] = None
        yield a, f"argument {i} NULL"
    for i in sizes:
        a = list(good)
        a[i] = bad_size
        yield a, f"argument {i} = {bad_size}"


# name -> (valid-looking arguments without the stream, indices of the required pointers, of the int sizes, of the size_t sizes);
# every rejection of these entry points is TQ_ERR_ARG (include/tqdne_hip.h, "EDM / sampler elementwise")
ELEMENTWISE = {
    "tq_heun_euler": ([FAKE] * 7 + [100], range(7), [], [7]),
    "tq_heun_correct": ([FAKE] * 8 + [100], range(8), [], [8]),
    "tq_sampler_init": ([FAKE] * 4 + [100], range(4), [], [4]),
    "tq_heun_churn": ([FAKE, FAKE, FAKE, 1.003, FAKE, FAKE, 100], [0, 1, 2, 4, 5], [], [6]),
    "tq_edm_scalars": ([FAKE, 1, 0.5, FAKE, FAKE, FAKE, FAKE, FAKE, 4], [0], [8], []),
    "tq_cm_scalars": ([FAKE, 1, 0.5, 0.002, FAKE, FAKE, 4], [0, 4, 5], [6], []),
    "tq_edm_noise_inject": ([FAKE, FAKE, FAKE, -1.2, 1.2, FAKE, FAKE, 2, 100], [0, 1, 2, 5, 6], [7, 8], []),
    "tq_edm_loss": ([FAKE, FAKE, FAKE, FAKE, FAKE, 2, 100], [0, 1, 2, 3], [5, 6], []),
    "tq_axpy_sigma": ([FAKE, FAKE, FAKE, FAKE, 2, 100], range(4), [4, 5], []),
    "tq_pseudo_huber_loss": ([FAKE, FAKE, FAKE, 0.01, FAKE, FAKE, 2, 100], [0, 1, 2, 4], [6, 7], []),
    "tq_scale_add2": ([FAKE] * 5 + [2, 100], range(5), [5, 6], []),
    "tq_ddpm_step": ([FAKE, FAKE, FAKE, FAKE, 100, 1, 0.9, 1.1, 1.0, 0.1, 0.9, 0.05], [0, 1, 3], [], [4]),
    "tq_mse_loss": ([FAKE, FAKE, FAKE, FAKE, 100], [0, 1, 2], [], [4]),
    "tq_vae_reparam_fwd": ([FAKE, FAKE, FAKE, FAKE, 2, 4, 16], [0, 1, 2], [4, 5, 6], []),
    "tq_vae_reparam_bwd": ([FAKE, FAKE, FAKE, FAKE, 1e-6, 2, 4, 16], [0, 1, 2, 3], [5, 6, 7], []),
    "tq_concat_scale": ([FAKE, FAKE, FAKE, FAKE, 2, 3, 3, 16], [0, 2, 3], [4, 5, 6, 7], []),
    "tq_fourier_features": ([FAKE, FAKE, FAKE, 2, 16], [0, 1, 2], [3, 4], []),
    "tq_gemm_f32_jobs": ([FAKE, 2, 4], [0], [1, 2], []),
    "tq_pair_sum": ([FAKE, FAKE, 2, 16, 8, 0], [0, 1], [2, 3, 4], []),
    "tq_zero_stuff": ([FAKE, FAKE, 2, 8, 16, 8], [0, 1], [2, 3, 4, 5], []),
}


@pytest.mark.parametrize("name", sorted(ELEMENTWISE))
def test_null_pointers_and_empty_sizes_are_rejected(name):
    good, pointers, int_sizes, sizet_sizes = ELEMENTWISE[name]
    fn = getattr(lib(), name)
    for args, what in variants(good, pointers, list(int_sizes) + list(sizet_sizes), 0):   # (n == 0 for the size_t kernels)
        assert fn(*args, None) == ARG, f"{name}: {what}"
    for args, what in variants(good, [], int_sizes, -1):
        assert fn(*args, None) == ARG, f"{name}: {what}"


def test_optional_pointers_alone_do_not_excuse_a_missing_required_one():
    """the nullable arguments (gradient outputs, kl_out, scale, noise, bias, hidden) given, a required one missing"""
    L = lib()
    assert L.tq_edm_loss(FAKE, FAKE, FAKE, None, FAKE, 2, 100, None) == ARG             # dpred without loss_out
    assert L.tq_pseudo_huber_loss(FAKE, FAKE, FAKE, 0.01, None, FAKE, 2, 100, None) == ARG
    assert L.tq_mse_loss(FAKE, FAKE, None, FAKE, 100, None) == ARG
    assert L.tq_vae_reparam_fwd(FAKE, FAKE, None, FAKE, 2, 4, 16, None) == ARG          # kl_out without z
    assert L.tq_ddpm_step(FAKE, FAKE, FAKE, None, 100, 1, 0.9, 1.1, 1.0, 0.1, 0.9, 0.05, None) == ARG
    assert L.tq_concat_scale(None, FAKE, FAKE, FAKE, 2, 3, 3, 16, None) == ARG
    assert L.tq_pair_sum(FAKE, FAKE, 2, 16, 6, 1, None) == ARG                         # channels not a multiple of 4
    assert L.tq_zero_stuff(FAKE, FAKE, 2, 8, 16, 6, None) == ARG
    assert L.tq_pair_sum(FAKE, FAKE, 2, 16, -4, 0, None) == ARG                        # a negative multiple of 4
    assert L.tq_zero_stuff(FAKE, FAKE, 2, 8, 16, -4, None) == ARG


def test_clipped_optimizer_steps_reject_a_negative_clip_value():
    L = lib()
    assert L.tq_adam_ema_step_clipped(FAKE, 3, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.0, 1.0, 1.0, None, None, -1.0, None) == ARG
    assert L.tq_radam_ema_step_clipped(FAKE, 3, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.0, 1.0, None, None, -1.0, None) == ARG


def test_embed_fwd_argument_checks():
    L = lib()
    good = [FAKE] * 14 + [2, 32, 4]
    for i in (0, 2, 3, 4, 5, 6, 11, 12):                       # t, fourier_w, time MLP, emb, silu_emb
        a = list(good)
        a[i] = None
        assert L.tq_embed_fwd(*a, None) == ARG, f"argument {i} NULL"
    for i in (1, 7, 8, 9, 10):                                  # cond and its MLP: required when ncond > 0
        a = list(good)
        a[i] = None
        assert L.tq_embed_fwd(*a, None) == ARG, f"argument {i} NULL with ncond > 0"
    for B, mc, ncond in [(0, 32, 4), (-1, 32, 4), (2, 0, 4), (2, 33, 4), (2, 32, -1)]:
        assert L.tq_embed_fwd(*good[:14], B, mc, ncond, None) == SHAPE, (B, mc, ncond)


def test_linear_fwd_argument_checks_and_its_lds_limit():
    L = lib()
    for i in (0, 1, 3):
        a = [FAKE] * 4
        a[i] = None
        assert L.tq_linear_fwd(*a, 4, 128, 64, None) == ARG
    for B, E, N in [(0, 128, 64), (4, 0, 64), (4, 128, 0), (-1, 128, 64)]:
        assert L.tq_linear_fwd(FAKE, FAKE, FAKE, FAKE, B, E, N, None) == SHAPE
    # 64 (E + 1) + 16 E floats of LDS: 164096 bytes at E = 512, 256 above the launcher's 160 KB; E = 508 (162816 bytes) is the
    # widest layer the GPU file runs
    assert L.tq_linear_fwd(FAKE, FAKE, FAKE, FAKE, 16, 512, 64, None) == SHAPE
    assert L.tq_linear_fwd(FAKE, FAKE, None, FAKE, 16, 512, 64, None) == SHAPE


def test_gn_bwd_finalize_argument_checks():
    L = lib()
    good = [FAKE, FAKE, FAKE, 2, 64, 128, FAKE, FAKE, FAKE, FAKE, FAKE]
    for i in (0, 1, 2, 6, 7, 8, 9, 10):
        a = list(good)
        a[i] = None
        assert L.tq_gn_bwd_finalize(*a, None) == ARG, f"argument {i} NULL"
    for B, C, T in [(2, 48, 128), (0, 64, 128), (2, 0, 128), (2, 64, 0), (2, -32, 128)]:   # 48: not a multiple of the 32 groups
        a = list(good)
        a[3:6] = B, C, T
        assert L.tq_gn_bwd_finalize(*a, None) == SHAPE, (B, C, T)


def test_gemm_tiles():
    L = lib()
    assert L.tq_gemm_tiles(1, 1) == 1
    assert L.tq_gemm_tiles(32, 32) == 1
    assert L.tq_gemm_tiles(33, 31) == 2
    assert L.tq_gemm_tiles(0, 5) == 0
    assert L.tq_gemm_tiles(1, 70) == 3 and L.tq_gemm_tiles(64, 32) == 2 and L.tq_gemm_tiles(5, 5) == 1   # the GPU file's job table
