/* tqdne_hip.h -- C ABI of libtqdne_hip.so: the MI355X (gfx950) kernels behind the tqdne 1-D EDM hot path.
 *
 * The reference (highfem/tqdne) has no FFI / plugin interface: its hot path is ordinary PyTorch modules
 * (SURVEY.md section 8b).  These entry points are what a maintainer of the reference would bind (ctypes, see
 * INTEGRATION.md) to replace the ATen op chains cited on each function.  Conventions:
 *   - device pointers only, caller-owned memory, nothing allocated or synchronised inside;
 *   - all work is enqueued on the given HIP stream (graph-capture safe);
 *   - return 0 on success, a TQ_ERR_* code (negative) for bad arguments, or a hipError_t (>0) from the launch;
 *   - re-entrant, no mutable global state: safe for one process per GPU and for several streams.
 * Layouts: activations (B, T, C) fp32, C contiguous; network input/output (B, C, T) fp32 as in the reference;
 * per-channel partial statistics (B, nslots, C, 2) fp32 with nslots = ceil(T / 128) and {sum, sum of squares};
 * GroupNorm folded to per-(b, c) scale/shift (B, C) fp32:  norm(x) = scale * x + shift.
 *   RANGE of the partial statistics: the sums are fp32 and un-shifted ({sum y, sum y^2}; backward {sum g, sum g*x}), combined in fp64, so
 *   variance and S2 - mean*S1 cancel once a group's mean is far from zero.  Every emitted entry is within (n + 1) 2^-24 sum|terms| of
 *   the exact sum of its n rows (each producer, tests/test_groupnorm_gpu.py); what that costs downstream is stated at tq_gn_finalize.
 */
#ifndef TQDNE_HIP_H
#define TQDNE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define TQ_ABI_VERSION 9

#define TQ_ERR_ARG (-1)   /* null / inconsistent pointer arguments */
#define TQ_ERR_SHAPE (-2) /* unsupported shape */

/* flags of TqConvDesc.flags */
#define TQ_CONV_GN 1       /* apply gscale/gshift (folded GroupNorm32) to the input */
#define TQ_CONV_SILU 2     /* apply SiLU to the (normalised) input */
#define TQ_CONV_EMB 4      /* add emb[b, co] to the output (ResBlock time embedding, unet.py:141) */
#define TQ_CONV_RES 8      /* add res[b, t, co] to the output (residual, unet.py:143 / blocks.py:145) */
#define TQ_CONV_STATS 16   /* emit per-channel partial statistics of the output */
#define TQ_CONV_DROPOUT 32 /* training-mode dropout on the activated input (unet.py:101) */
/* TQ_CONV_POLY2 (tq_conv1d_fwd, stride 1, ktaps 3, no upsample): the launch is BOTH phases of "nearest x2 upsampling, then conv k = 5"
 * (Upsample.forward, blocks.py:56-66) written as one k = 3 conv over the un-upsampled input -- even outputs see the taps
 * (w0+w1, w2+w3, w4), odd outputs (w0, w1+w2, w3+w4), 3/5 of the multiply-adds.  C_out = 2*C: output channel block [p*C, (p+1)*C)
 * is phase p and is stored to row 2t+p of a (B, 2*T_out, C) tensor; bias / emb / res are indexed by the real channel / row;
 * statistics: 2*ceil(T_out/128) slots of C channels (slot = 2*tile + p; with TQ_CONV_STATS T_out must be a multiple of 128 or leave
 * more than 64 rows in its last tile, so that this equals the ceil(2*T_out/128) slots of the (B, 2*T_out, C) tensor). */
#define TQ_CONV_POLY2 64
/* TQ_CONV_CH_TILES (round 6): a hint of launch-bound plans (a grid far below the chip): where a conv has an input-stationary form with one
 * workgroup per position tile (the qkv projection: C_out >= 512 over 128 / 256 input channels) take the channel-tiled form instead --
 * C_out / 256 times the workgroups (a 16-sample plan alone on the device at T = 512: 64 -> 192; 37 -> 21 us).  Same numbers.  With the
 * device full (B = 64, or four 16-sample lanes) the input-stationary form is the faster one (+0.7 % of a sample with this flag). */
#define TQ_CONV_CH_TILES 128
/* TQ_CONV_WIDE_TABLE: take the wide-table instantiation of the fp16 + MX-fp6 forward tiles (the one built for more than 1024
 * concatenated input channels, see tq_conv1d_max_cin) for a launch of at most 1024 as well.  Same numbers, bit for bit: a switch for
 * tests and A/B timing.  Launches that are not in TQ_WFMT_F16_MX6 with a TQ_CONV_GN prologue ignore it; TQ_ERR_SHAPE where no wide tile
 * is built (128 does not divide C_out, TqConvDesc.gn_fold set). */
#define TQ_CONV_WIDE_TABLE 256

/* TqConvDesc.wfmt: how the fp32 product x * w is contracted on the matrix cores (= format of the packed weights).
 * BF16X3: both operands split into bf16 hi + lo, three bf16 MFMA products; fp32 range, ~2^-16 relative (pack modes 0 / 1).
 *   RANGE, both operands: that of fp32 -- the error against exact arithmetic is 7e-6 ... 9e-6 of the output for weights of typical
 *   magnitude 6e-2 down to 6e-11 and activations of 1e3 down to 1e-6 (measured; tests/test_contraction_gpu.py, range sweep).
 * F16_MX8: per 64 channels two fp16 MFMAs plus one block-scaled fp8 MFMA carrying both first-order corrections; ~2^-15 relative at
 * 2/3 of the MFMA cycles; the activation operand has fp16 RANGE (|x| > 65504 overflows to inf / NaN in the output, relative precision lost below 6e-5).  Built
 * for stride-1 forward launches (tq_conv1d_fwd, tq_conv1d_fwd_skip, tq_conv1d_fwd_qkv) with 128 | C_out and 64 | every source's
 * channels (pack mode 2).
 *   RANGE: the corrections are e4m3 with UNIFORM scales, so the ~2^-15 holds for O(1) operands only.  Activation operand: |x| <= 448
 *   (beyond it the x w_l correction clamps: 3e-4 of the output at |x| ~ 1e3) and typical |x| >= ~0.1 (x_l 2^12 falls below e4m3's
 *   normal range: 1.5e-4 at 1e-3, 2e-3 at 1e-5, 2e-2 at 1e-6).  WEIGHT operand (stored as fp16(w), e4m3(w) and e4m3(w_l 2^12), no
 *   scale): typical |w| >= ~2e-2 and |w| <= 448 -- at typical |w| = 6e-5 the x_l w correction is gone (4e-4), at 6e-7 the error is
 *   3e-2, at 6e-8 0.3, below that the output is zero.  |w| >= 65520 becomes inf. */
#define TQ_WFMT_BF16X3 0
#define TQ_WFMT_F16_MX8 1
/* F16_MX6: as F16_MX8 with e2m3 (fp6) correction operands and per-lane E8M0 block scales (one per 16 channels): 12 instead of 16
 * MFMA passes per 64 channels and corrections that do not clamp; same shapes, same fp16 RANGE of the activation operand (pack
 * mode 3).  Round 6: additionally 64 | C_out for the k = 5 launches with a TQ_CONV_GN | TQ_CONV_SILU prologue (tq_conv1d_fwd,
 * tq_conv1d_fwd_skip: the 64-channel ResBlock convs; tile of 64 channels x 128 positions).
 *   RANGE (measured on the kernels and reproduced by the bit-model oracle/contraction.py; error against exact arithmetic relative to
 *   the largest output).  Both operands' main part is a plain fp16 value with no scale; the block scales only serve the corrections,
 *   which can restore what fp16's ROUNDING lost (11 -> ~15 bits) but not what its SUBNORMAL range lost.  Inside the envelope the
 *   error is 1.1e-5 ... 1.5e-5:
 *     activation operand: |x| <= 65504 (beyond: inf / NaN in the output), typical |x| >= 1e-3.  Below: 7e-5 at 1e-5, 7e-4 at 1e-6.
 *     WEIGHT operand (pack modes 3 / 5 store fp16(w) un-scaled): |w| < 65520 (beyond: inf), typical |w| >= ~5e-5 (weight rms 5.6e-5:
 *     1.3e-5).  Below: 1.2e-3 at rms 5.6e-7, 1.1e-2 at 5.6e-8, 3.6e-2 at 5.6e-9 and smaller (fp16(w) is zero there, the e2m3
 *     corrections are all that is left).  One hot channel (x 1e3) inside a 16-block or 2 % of x 30 outliers on either operand stay
 *     at 2e-5.
 *   Zero-initialised convs (zero_module) pass through the range below the envelope during the first optimizer steps: their forward
 *   output is then small against the residual path it is added to, but the DATA GRADIENT through them (pack mode 5, below) carries
 *   the same relative error into everything upstream -- see TqConvBwdDesc.wfmt. */
#define TQ_WFMT_F16_MX6 2

/* ABI 7.  Consumer-side GroupNorm fold (TqConvDesc.gn_fold; optional, NULL = off): the launch forms the folded coefficients of ITS OWN
 * prologue (TQ_CONV_GN) from the partial statistics of its (up to two, concatenated) source tensors -- every workgroup folds its sample,
 * the arithmetic of tq_gn_finalize, bit-identical coefficients -- and WRITES them to the gscale / gshift arguments of the call (and
 * mean_rstd), where the weight / data gradients of the same conv read them later.  Replaces the tq_gn_finalize launch in front of the
 * conv in launch-bound plans.  Built for the small tile (t_tile = 32: tq_conv1d_fwd, tq_conv1d_fwd_skip); other launches return TQ_ERR_SHAPE.
 * Host pointer, read at launch. */
typedef struct TqGnFold {
    const float* stats0;   /* (B, ceil(T_in / slot0), C_in0, 2) partial statistics of source 0 */
    const float* stats1;   /* (B, ceil(T_in / slot1), C_in1, 2) or NULL */
    int32_t slot0, slot1;  /* positions per statistics slot of each source: 128 (0 = 128) or 32 */
    const float* gamma;    /* (C_in0 + C_in1) affine parameters of the GroupNorm */
    const float* beta;
    float* mean_rstd;      /* (B, 32, 2) out, nullable */
} TqGnFold;

typedef struct TqConvDesc {
    int32_t B, T_in, T_out;
    int32_t C_in0, C_in1; /* channels of the two concatenated sources (C_in1 = 0: single source) */
    int32_t C_out;
    int32_t ktaps, stride, pad;
    int32_t upsample; /* 1: input is read through nearest x2 upsampling (T_out = 2*T_in) */
    int32_t flags;
    int32_t emb_stride; /* floats between consecutive samples in emb */
    uint32_t dropout_site;
    float dropout_p;
    uint64_t dropout_seed;
    int32_t C_skip0, C_skip1; /* tq_conv1d_fwd_skip only: channels of the fused 1x1 skip conv's (concatenated) input; else 0 */
    int32_t wfmt;             /* TQ_WFMT_*: format of packed_w = contraction scheme of this launch */
    /* Range guard of the fp16-range scheme (optional, NULL = off): with TQ_CONV_STATS the epilogue sets *range_flag = 1 when a
     * channel's sum of squares over one 128-position slot reaches (65504 / 2)^2, i.e. when max|y| of the written tensor MAY exceed
     * half of the fp16 range (max|y| <= sqrt(sum y^2)), or is not finite.  The caller polls the flag and moves the launches that
     * read such a tensor un-normalised (fused 1x1 skip convs, up-sampling convs) to TQ_WFMT_BF16X3.  Device pointer, never reset
     * by the library. */
    int32_t* range_flag;
    const void* reserved1;   /* reserved, must be NULL: a non-NULL value returns TQ_ERR_ARG */
    /* ABI 5.  Positions per workgroup along T: 0 = the default tiles (128 / 256); 32 = the small tile for launch-bound batches (a
     * launch of the default tiling with far fewer workgroups than compute units: four times the workgroups, a quarter of the work
     * each).  Built for tq_conv1d_fwd / tq_conv1d_fwd_skip with ktaps 5, stride 1, no upsampling, TQ_CONV_GN | TQ_CONV_SILU, in
     * TQ_WFMT_BF16X3 and TQ_WFMT_F16_MX6 (128 | C_out); other launches return TQ_ERR_SHAPE.  With TQ_CONV_STATS the partial
     * statistics then have one slot per 32 positions: stats_partial is (B, ceil(T_out / 32), C, 2), and tq_gn_finalize must be told
     * (its slot arguments).  Convolution results are bit-identical to the default tiles'; the statistics are the same sums in another
     * association order. */
    int32_t t_tile;
    int32_t reserved2;
    const TqGnFold* gn_fold; /* ABI 7: consumer-side GroupNorm fold (see TqGnFold), NULL = off */
} TqConvDesc;

/* flags of TqConvBwdDesc.flags: which stages the FORWARD conv applied to its input */
#define TQ_BWD_GN 1       /* forward input was GroupNorm-folded (gscale/gshift given) */
#define TQ_BWD_SILU 2     /* forward applied SiLU: multiply by silu'(gscale*x+gshift) */
#define TQ_BWD_DROPOUT 4  /* forward applied dropout: re-generate the same mask */
#define TQ_BWD_ACCUM 8    /* add to dx instead of overwriting (tensor consumed by several ops) */
#define TQ_BWD_STATS 16   /* emit per-channel partial sums {sum g, sum g*x} for the GroupNorm backward.  Not together with
                           * TQ_BWD_ACCUM (TQ_ERR_ARG): the sums would be taken of the accumulated tensor, not of g. */

typedef struct TqConvBwdDesc {
    int32_t B, T;
    int32_t C_dy;         /* channels of the incoming gradient (= forward C_out) */
    int32_t C_dx0, C_dx1; /* channel split of the produced gradient (= forward C_in0, C_in1) */
    int32_t ktaps;        /* stride-1 "same" convs only; strided / upsampled ones are composed with tq_zero_stuff / tq_pair_sum */
    int32_t flags;
    uint32_t dropout_site;
    float dropout_p;
    uint64_t dropout_seed;
    /* ABI 5.  Contraction scheme of the data gradient: TQ_WFMT_BF16X3 (0: fp32 range, packed_w_t from pack mode 1) or
     * TQ_WFMT_F16_MX6 (packed_w_t from pack mode 5; 64 | C_dy and 64 | C_dx0 + C_dx1): dy is staged times the exact power of two
     * that brings max|dy| into [2^13, 2^14) -- gradients are far below fp16's normal range otherwise -- and the accumulators are
     * multiplied by its inverse, so the result has the accuracy of the forward scheme (~2^-15 relative) at half the MFMA cycles of
     * bf16x3.  RANGE: dy is un-limited (it is scaled; samples of one batch that differ by 1e-6 in scale under the shared maximum still
     * come out at 1.1e-5 of their own largest entry).  The WEIGHT operand is NOT scaled and has the envelope of TQ_WFMT_F16_MX6 above:
     * typical |w| >= ~5e-5; measured error of the data gradient relative to its largest entry 1.2e-3 at weight rms 5.6e-7, 1.1e-2 at
     * 5.6e-8, 4e-2 at 5.6e-9 and below, whatever the size of dy (TQ_WFMT_BF16X3: 8e-6 throughout).  dy_amax: DEVICE pointer to a TQ_AMAX_WORDS block as tq_colsum(..., amax_out) / tq_gn_bwd_apply_colsum fill it for the same
     * dy (the maximum over its TQ_AMAX_WAYS words = IEEE bit pattern of max|dy|; any upper bound within a factor 8 will do); required for
     * TQ_WFMT_F16_MX6. */
    int32_t wfmt;
    int32_t reserved;
    const uint32_t* dy_amax;
} TqConvBwdDesc;

int tq_abi_version(void);

/* ---- weights -------------------------------------------------------------------------------------------- */
/* Pack a torch Conv1d weight (C_out, C_in, K) fp32 into per-lane MFMA fragments.
 * mode 0: forward operand, TQ_WFMT_BF16X3; mode 1: data-gradient operand (transposed + tap-flipped), TQ_WFMT_BF16X3;
 * mode 2: forward operand, TQ_WFMT_F16_MX8; mode 3: forward operand, TQ_WFMT_F16_MX6; mode 5 (ABI 5): data-gradient operand,
 * TQ_WFMT_F16_MX6.  (mode 4 is a plain copy job of tq_pack_jobs.) */
size_t tq_conv_weight_pack_bytes(int C_out, int C_in, int K, int mode);
int tq_pack_conv_weight(const float* w, int C_out, int C_in, int K, int mode, void* packed, hipStream_t stream);
int tq_conv_tile_co(int C_out);
/* Width limits, asked of the library (no device needed; hosts plan with these instead of repeating constants).
 *   tq_conv1d_max_cin(wfmt, C_out): the most concatenated input channels C_in0 + C_in1 a stride-1 forward launch with a TQ_CONV_GN
 *     prologue takes in that scheme on the tile chosen for C_out (C_out = 0: on its widest tile); 0 where the scheme has no tile.  TQ_WFMT_F16_MX6 keeps the folded GroupNorm coefficients of a sample in an LDS table:
 *     1024 entries in the established tiles, 2048 in the wide-table tiles (the 256- and 128-channel tiles of 128 positions and the small
 *     tile, k in {1, 3, 5}; chosen by the library when C_in0 + C_in1 > 1024).  TQ_WFMT_BF16X3 reads them from global memory: no table, the
 *     value is the widest shape the suite covers.  TQ_WFMT_F16_MX8 has the 1024-entry table only.  Launches WITHOUT a prologue (fused skip
 *     sources, resampling convs, data gradients incl. TqConvBwdDesc.C_dy) read no table and have no such limit.
 *   tq_conv1d_gn_fold_max_cin(wfmt, t_tile, C_out): the most channels for which a launch of that tile accepts TqConvDesc.gn_fold
 *     (the fold's scratch must fit the tile's staging buffers, and the wide-table tiles do not fold); 0 = this tile never folds.
 *   tq_conv1d_max_cout(): the most output channels a plan may give a conv (3072: the qkv projection of a 1024-channel attention block,
 *     the widest shape the suite covers; the kernels themselves tile C_out).
 *   tq_colsum_max_channels(): the most channels of tq_colsum / tq_gn_bwd_apply_colsum (chunks of <= 1024 channels over the grid). */
int tq_conv1d_max_cin(int wfmt, int C_out);
int tq_conv1d_max_cout(void);
size_t tq_conv1d_wide_lds_bytes(int ktaps, int t_tile, int C_out); /* dynamic LDS of the wide-table tile of a launch; 0 = no such tile */
int tq_conv1d_gn_table_entries(int wide); /* entries of the coefficient table: 0 the established tiles (1024), 1 the wide-table tiles (2048) */
int tq_conv1d_gn_fold_max_cin(int wfmt, int t_tile, int C_out);
int tq_colsum_max_channels(void);
/* All (re)packs of a plan in one launch (what a training step re-does after every optimizer update: torch parameters ->
 * forward / transposed fragments, plus the gather of the ResBlocks' embedding projections into their concatenated buffers,
 * unet.py:91-97).  jobs: a DEVICE array, block_begin = running sum of tq_pack_job_blocks over the preceding jobs.
 * mode 0..3 as tq_pack_conv_weight; mode 4: copy C_out floats src -> dst. */
typedef struct TqPackJob {
    const void* src;
    void* dst;
    int32_t C_out, C_in, K, mode;
    int32_t block_begin;
    int32_t reserved;
} TqPackJob;
int tq_pack_job_blocks(int C_out, int C_in, int K, int mode);
int tq_pack_jobs(const TqPackJob* jobs_device, int njobs, int total_blocks, hipStream_t stream);

/* ---- fused convolution ---------------------------------------------------------------------------------- */
/* Replaces GroupNorm32 -> SiLU -> Dropout -> Conv1d(k in {1,3,5}) -> +emb -> +residual, the channel concat and the
 * nearest-x2 upsample of tqdne/unet.py:86-102,131-143,396 and tqdne/blocks.py:56-66,92-101,127-145.
 * Constraints: C_in0, C_in1, C_out multiples of 32; stride 1 ("same" padding, pad = k/2) or stride 2 (k=3, pad=1). */
int tq_conv1d_fwd(const TqConvDesc* desc, const float* x0, const float* x1, const float* gscale, const float* gshift,
                  const void* packed_w, const float* bias, const float* emb, const float* residual, float* y,
                  float* stats_partial, hipStream_t stream);

/* Same, with the ResBlock's 1x1 skip convolution fused in (unet.py:112,143): y = conv_k(f(x)) + W_skip * x_skip + biases.
 * packed_w holds tq_pack_conv_weight(main, mode 0) immediately followed by tq_pack_conv_weight(skip 1x1, mode 0).
 * Built for k = 5 with GN + SiLU (+ dropout) prologues. */
int tq_conv1d_fwd_skip(const TqConvDesc* desc, const float* x0, const float* x1, const float* gscale, const float* gshift,
                       const void* packed_w_main_then_skip, const float* bias, const float* emb, const float* skip_x0,
                       const float* skip_x1, const float* skip_bias, float* y, float* stats_partial, hipStream_t stream);

/* Inference form of the AttentionBlock's qkv projection (blocks.py:127-145): 1x1 conv of GN(x) whose K and V output channels are
 * written directly as the pre-split planes tq_attention_fwd_presplit streams (K pre-scaled by D^-1/4: bf16 hi / lo; V in
 * `v_format`, which both calls of the pair must be given alike), q as fp32 into qkv (B, T, 3 H D) (its K / V part is left
 * untouched).  kv_planes: tq_attention_workspace_bytes(B, T, H, D) bytes whose rows t >= T (padding to a multiple of 64) must be
 * zero.  desc: ktaps 1, single source, C_out = 3 H D, flags none or TQ_CONV_GN.
 * v_format (ABI 6; was the environment variable TQDNE_ATTN_VF16 read inside the library):
 *   TQ_KV_V_F16: V as fp16 hi / lo planes, which the attention kernel multiplies by ONE fp16 softmax weight -- two products instead
 *     of three, 1.4e-4 of the output scale.  fp16 RANGE: with desc->range_flag set the epilogue raises it when |v| reaches half of
 *     the fp16 range (or is not finite), exactly like the fp16-range conv schemes; the caller repeats with TQ_KV_V_BF16;
 *   TQ_KV_V_BF16: bf16 hi / lo V, three products, fp32 range. */
#define TQ_KV_V_BF16 0
#define TQ_KV_V_F16 1
int tq_conv1d_fwd_qkv(const TqConvDesc* desc, const float* x, const float* gscale, const float* gshift, const void* packed_w,
                      const float* bias, float* qkv, void* kv_planes, int H, int D, int v_format, hipStream_t stream);

/* Data gradient of tq_conv1d_fwd (stride 1): g = (W^T * dy) chained through the forward prologue (dropout, SiLU,
 * folded GN scale); packed_w_t from tq_pack_conv_weight(mode 1).  x0/x1/gscale/gshift are the FORWARD conv's inputs.
 * Autograd counterpart of the ATen conv/SiLU/dropout backward chain Lightning runs for edm.py:136 training_step. */
int tq_conv1d_bwd_data(const TqConvBwdDesc* desc, const float* dy, const void* packed_w_t, const float* x0, const float* x1,
                       const float* gscale, const float* gshift, float* dx0, float* dx1, float* gstats_partial,
                       hipStream_t stream);

/* Weight gradient of tq_conv1d_fwd: dw (C_out, C_in, K) fp32 (overwritten) = sum_{b,t} dy * xhat, xhat recomputed from the
 * FORWARD conv's inputs exactly as the forward prologue does (same desc, incl. dropout seed).  workspace: >=
 * tq_conv1d_bwd_weight_workspace(desc) bytes of scratch (partial slabs of the (b,t) splits). */
size_t tq_conv1d_bwd_weight_workspace(const TqConvDesc* desc);
int tq_conv1d_bwd_weight(const TqConvDesc* desc, const float* dy, const float* x0, const float* x1, const float* gscale,
                         const float* gshift, float* dw, void* workspace, size_t ws_bytes, hipStream_t stream);
/* Same, with the column sums of dy fused in (the bias gradient and, per sample, the gradient of the broadcast time embedding,
 * unet.py:141): colsum_bc[b * bc_stride + co] += sum_t dy[b, t, co], colsum_c[co] (and colsum_c2[co]) += sum_{b,t} dy -- each
 * nullable, accumulated with atomics into buffers the caller has zeroed.  Saves the separate pass of tq_colsum over dy. */
int tq_conv1d_bwd_weight_colsum(const TqConvDesc* desc, const float* dy, const float* x0, const float* x1, const float* gscale,
                                const float* gshift, float* dw, void* workspace, size_t ws_bytes, float* colsum_bc, int bc_stride,
                                float* colsum_c, float* colsum_c2, hipStream_t stream);

/* How a weight-gradient launch of `desc` is tiled and split (additive at ABI 8; needs no launch -- the slots of the split come from the
 * device's occupancy where there is one and from the MI355X figures otherwise).  Filled by the functions the launch and
 * tq_conv1d_bwd_weight_workspace plan with, so a test can name the kernel form and the split regime a case runs in.
 *   form             TQ_WGRAD_*: the kernel form.  Four waves and a 128-output-channel tile with input chunks of 32 (C32: k = 3 / 5, and
 *                    k = 1 sources that are not whole 64-channel chunks), 64 (C64: k = 1, 64 | C_in0, C_in1) or 128 channels (C128:
 *                    k = 1, stride 1, 128 | C_in0, C_in1); W8: eight waves on a 64-channel input tile (k = 3 / 5, 64 | C_in0, C_in1,
 *                    128 | C_out); H64: four waves on a 64-output-channel tile (k = 3 / 5, stride 1, no upsampling, 64 | C_in0, C_in1,
 *                    C_out == 64).  A launch that carries fused column sums (with_colsum != 0: colsum_bc or colsum_c given) never takes
 *                    W8 / H64.
 *   n_cotiles        output-channel tiles (of 128 channels; 64 in H64), the last one may be partial
 *   n_cichunks       input-channel chunks of the form's width over C_in0 + C_in1
 *   n_ttiles         64-position units per sample, ceil(T_out / 64)
 *   n_units          B * n_ttiles: the (b, t) reduction in units
 *   n_splits         slabs of the workspace = workgroups per (output tile, input chunk); split s reduces the units
 *                    [s * units_per_split, min(n_units, (s + 1) * units_per_split)), so the last one may be shorter
 *   units_per_split  units of a full split
 *   xcd_order        1: workgroups are numbered so that the input-chunk workgroups of one (split, output tile) pair share an XCD
 *                    (8 | n_splits * n_cotiles, and TQDNE_WGRAD_XCD=0 not set); 0: the plain order
 * The grid is n_splits * n_cotiles * n_cichunks workgroups; the workspace of a launch is n_splits * ktaps * C_out * (C_in0 + C_in1)
 * floats, and tq_conv1d_bwd_weight_workspace is the larger of the with_colsum = 0 / 1 figures.
 * NULL desc / out: TQ_ERR_ARG; a shape the launch refuses (channels not multiples of 32, ktaps outside {1, 3, 5}, stride 2 with
 * ktaps != 3, upsampling with ktaps 1) or B, T_in, T_out < 1: TQ_ERR_SHAPE, *out untouched. */
#define TQ_WGRAD_C32 0
#define TQ_WGRAD_C64 1
#define TQ_WGRAD_C128 2
#define TQ_WGRAD_W8 3
#define TQ_WGRAD_H64 4
typedef struct TqWgradPlan {
    int32_t form;
    int32_t n_cotiles, n_cichunks, n_ttiles;
    int32_t n_units, n_splits, units_per_split;
    int32_t xcd_order;
} TqWgradPlan;
int tq_conv1d_bwd_weight_plan(const TqConvDesc* desc, int with_colsum, TqWgradPlan* out);

/* First conv of the network: (B, C_in<=16, T) fp32 input (this kernel's limit; the plans route stems of 17 ... 64 signal channels
 * through tq_nct_to_btc + tq_conv1d_fwd, see the boundary section below), scaled per sample by in_scale[b] (EDM c_in, edm.py:107;
 * NULL = 1), k taps "same" -> (B, T, C_out) channels-last + bias (+ partial statistics (B, ceil(T / 128), C_out, 2)).  unet.py:233.
 * C_out: every multiple of 32 up to 1024 (channel-tiled kernel, csrc/ends_wide.hip) besides the powers of two 4 ... 1024 whose
 * weights fit one workgroup's LDS (the first kernel, unchanged for those); k in {1, 3, 5}; any B, T >= 1. */
/* LDS bytes tq_stem_conv_fwd needs for a shape; 0 = unsupported shape.  Needs no device. */
size_t tq_stem_conv_lds_bytes(int C_in, int C_out, int ktaps);
int tq_stem_conv_fwd(const float* x_nct, const float* in_scale, const float* w, const float* bias, float* y,
                     float* stats_partial, int B, int C_in, int T, int C_out, int ktaps, hipStream_t stream);

/* Last conv: GroupNorm32+SiLU (folded scale/shift) -> conv k "same" to C_out<=16 (this kernel's limit; heads of 17 ... 64 signal
 * channels run as tq_conv1d_fwd + tq_btc_to_nct, see the boundary section below) -> (B, C_out, T) output,
 * then out = c_out[b] * conv + c_skip[b] * skip_src[b, co, t]  (EDM / consistency preconditioning, edm.py:111-113,
 * consistency_model.py:78); c_out/c_skip/skip_src NULL = plain conv output.  unet.py:355-357,398. */
/* C_in: 16 | C_in <= 128 where the first kernels' LDS tile fits 64 KB (unchanged for those shapes), and every multiple of 32 up to
 * 1024 (csrc/ends_wide.hip: the reduction over C_in walks chunks of <= 128 channels inside the workgroup; input read once; fp32 FMA;
 * no atomics; <= 64 KB of LDS); C_out <= 16; k in {1, 3, 5}; any B, T >= 1; with or without the prologue / the epilogue. */
/* LDS bytes tq_head_conv_fwd needs for a shape; 0 = unsupported shape.  Needs no device. */
size_t tq_head_conv_lds_bytes(int C_in, int C_out, int ktaps);
int tq_head_conv_fwd(const float* x, const float* gscale, const float* gshift, const float* w, const float* bias,
                     const float* c_out, const float* c_skip, const float* skip_src, float* y_nct, int B, int T, int C_in,
                     int C_out, int ktaps, hipStream_t stream);

/* ---- GroupNorm32 statistics -> folded scale/shift ---------------------------------------------------------- */
/* The normalised tensor is the channel concat of up to two sources whose per-channel partial statistics were
 * emitted by their producers.  Writes scale/shift (B, C0+C1) and mean/rstd (B, 32, 2).  nn.py:11-13,90-105. */
/* slot0 / slot1 (ABI 5): positions per statistics slot of each source -- 128 (0 = default) or 32 (a tensor written by a
 * TqConvDesc.t_tile = 32 launch); stats_i is (B, ceil(T / slot_i), C_i, 2). */
/* RANGE (measured on the kernels, tests/test_groupnorm_gpu.py::test_chain_under_mean_std_regimes; worst of four shapes and two
 * producers; max|error| / max|float64| per tensor; in parentheses a CPU emulation of fp32 slot sums taken sequentially, the least
 * accurate order, on the same inputs).  By |group mean| / group std of the normalised tensor:
 *     ratio   scale*x + shift       dx (whole backward chain)   dgamma
 *       0     8.1e-8 (1.9e-7)       1.2e-7 (2.1e-7)             1.2e-7 (2.8e-7)
 *       3     1.5e-6 (3.6e-6)       2.1e-6 (3.2e-6)             1.7e-6 (2.4e-6)
 *      10     1.8e-5 (5.3e-5)       1.2e-5 (3.7e-5)             1.7e-5 (3.0e-5)
 *      30     1.3e-4 (3.1e-4)       1.4e-4 (2.7e-4)             9.4e-5 (5.4e-4)
 *     100     1.5e-3 (3.2e-3)       1.2e-3 (3.2e-3)             1.2e-3 (2.7e-3)
 * i.e. ~ratio^2 * 2^-24 * 2: inside 1e-3 up to a ratio of 30, beyond it around 100 (dbeta is a plain sum: 1.3e-7 throughout).  A group
 * with sum y^2 / n <= mean^2 (constant, or statistics that do not belong together) gets variance 0: rstd = 1 / sqrt(eps). */
int tq_gn_finalize(const float* stats0, int C0, const float* stats1, int C1, int B, int T, const float* gamma,
                   const float* beta, float* gscale, float* gshift, float* mean_rstd, int slot0, int slot1, hipStream_t stream);

/* GroupNorm32 backward, step 1: per-channel partial sums {sum g, sum g*x} (from tq_conv1d_bwd_data / tq_head_conv_bwd_ws)
 * + saved mean/rstd + gamma -> coefficients with dx = A*g + Bc*x + Cc, and dgamma/dbeta (atomically added: zero them first). */
int tq_gn_bwd_finalize(const float* gstats_partial, const float* mean_rstd, const float* gamma, int B, int C, int T,
                       float* coef_a, float* coef_b, float* coef_c, float* dgamma, float* dbeta, hipStream_t stream);
/* step 2, per concat source (channels [c_offset, c_offset+C_src) of the coefficients):
 * dx (+)= A*g + Bc*x + Cc (+ r);  r = gradient arriving over the residual path (NULL: none). */
int tq_gn_bwd_apply(const float* g, const float* x, const float* r, const float* coef_a, const float* coef_b,
                    const float* coef_c, float* dx, int B, int T, int C_src, int C_total, int c_offset, int accumulate,
                    hipStream_t stream);
/* step 2 with the column sums of the tensor it writes fused in (ABI 5): what tq_colsum(dx, ...) would add to colsum_bc / colsum_c /
 * colsum_c2 / amax_out afterwards, from the values while they are in registers (`dx` must then be COMPLETE after this launch: the
 * last writer of an accumulated gradient).  All four outputs NULL = tq_gn_bwd_apply. */
int tq_gn_bwd_apply_colsum(const float* g, const float* x, const float* r, const float* coef_a, const float* coef_b,
                           const float* coef_c, float* dx, int B, int T, int C_src, int C_total, int c_offset, int accumulate,
                           float* colsum_bc, int bc_stride, float* colsum_c, float* colsum_c2, uint32_t* amax_out,
                           hipStream_t stream);
/* out_bc[b*bc_stride + c] += bscale[b] * sum_t dy[b,t,c];  out_c[c], out_c2[c] += sum_{b,t} (...)  (each optional; bias and
 * embedding gradients: two biases fed by the same tensor are served by one pass).  4 | C <= tq_colsum_max_channels(): up to 1024
 * channels are one column per thread; wider tensors (the output gradient of a qkv projection, 3 C) are dealt over the grid in
 * near-equal chunks of <= 1024 channels, each formed exactly as a launch on that column slice would form it. */
/* Small fp32 GEMMs of the embedding-MLP backward (unet.py:91-97,210-227,383-388; the autograd of blocks.py:15-26): one launch runs
 * a list of independent products  C (M x N) = A (M x K) * f(B) (K x N) [* silu'(U)]  with strided operands
 * A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn] (a stride of 1 marks the contiguous direction), f = SiLU when pre_b,
 * U (M x N, row stride ldu) optional.  The job table lives in device memory; tile_begin = running sum of tq_gemm_tiles(M, N). */
typedef struct TqGemmJob {
    const float* A;
    const float* B;
    float* C;
    const float* U;
    int32_t M, N, K;
    int32_t sam, sak, sbk, sbn, ldc, ldu;
    int32_t pre_b;
    int32_t tile_begin;
} TqGemmJob;
int tq_gemm_tiles(int M, int N);
int tq_gemm_f32_jobs(const TqGemmJob* jobs_device, int njobs, int total_tiles, hipStream_t stream);
/* GaussianFourierProjection features (blocks.py:15-26): out (B, 2 half) = [sin(2 pi t W) | cos(2 pi t W)] */
int tq_fourier_features(const float* t, const float* W, float* out, int B, int half, hipStream_t stream);

/* amax_out (ABI 5, nullable): a block of TQ_AMAX_WORDS uint32 that receives the bit pattern of max|dy| by atomic max -- zero it first.
 * The maximum is SPREAD over TQ_AMAX_WAYS words TQ_AMAX_STRIDE apart (one per 128-byte line; a workgroup updates word (its index mod
 * TQ_AMAX_WAYS): atomics on one address serialise at ~11 ns each); the maximum of those words is max|dy|.  Non-negative floats order
 * like their bit patterns; a NaN in dy is recorded as +inf, so a poisoned tensor stays visible.  Feeds TqConvBwdDesc.dy_amax. */
#define TQ_AMAX_WAYS 16
#define TQ_AMAX_STRIDE 32
#define TQ_AMAX_WORDS (TQ_AMAX_WAYS * TQ_AMAX_STRIDE)
int tq_colsum(const float* dy, int B, int T, int C, float* out_bc, int bc_stride, float* out_c, float* out_c2,
              const float* bscale, uint32_t* amax_out, hipStream_t stream);
/* gradient plumbing of the strided / upsampled convs: out[b,u,:] = (u even) ? dy[b,u/2,:] : 0 for u < T_in;
 * dx[b,t,:] (+)= d_up[b,2t,:] + d_up[b,2t+1,:] */
int tq_zero_stuff(const float* dy, float* out, int B, int T_out, int T_in, int C, hipStream_t stream);
int tq_pair_sum(const float* d_up, float* dx, int B, int T, int C, int accumulate, hipStream_t stream);
/* ABI 7.  Upsample (blocks.py:56-66) trained in its two-phase k = 3 form (TQ_CONV_POLY2 forward; data gradient = tq_conv1d_bwd_data with
 * ktaps 3 and C_dy = 2 C_out on the output gradient (B, 2T, C_out) read as (B, T, 2 C_out); weight gradient = tq_conv1d_bwd_weight of that
 * k = 3 conv): folds dw2 (2 C_out, C_in, 3) = [d even-phase taps | d odd-phase taps] back onto the conv's five taps, dw (C_out, C_in, 5)
 * (overwritten): dw0 = dA0 + dB0, dw1 = dA0 + dB1, dw2 = dA1 + dB1, dw3 = dA1 + dB2, dw4 = dA2 + dB2. */
int tq_upsample_poly_wgrad_fold(const float* dw2, float* dw, int C_out, int C_in, hipStream_t stream);
/* Backward of the stem and head convs.  Both ADD into dw (and db): zero them first.
 * workspace: tq_stem_head_bwd_workspace() bytes of scratch (own buffer per call site and stream): every workgroup's partial sums go
 * to its row of the scratch and a second small launch adds the rows into dw (db) -- the outputs share 30 cache lines, and atomics on
 * one LINE serialise at ~11 ns each (512 workgroups: 180 us, the whole time of these kernels).  workspace NULL or too small: the
 * workgroups add into dw (db) with atomics instead. */
size_t tq_stem_head_bwd_workspace(void);
/* stem conv weight gradient dw (C_out, C_in, K).  Keeps its limit of C_out C_in K <= 2048 weights (TQ_ERR_SHAPE beyond): the plans
 * form the gradient of a wider stem with tq_conv1d_bwd_weight on a 32-channel channels-last copy of the input (bf16x3 error bars),
 * whatever the first-level width. */
int tq_stem_conv_bwd_weight_ws(const float* dy, const float* x_nct, const float* in_scale, float* dw, int B, int C_in, int T,
                               int C_out, int ktaps, void* workspace, size_t ws_bytes, hipStream_t stream);
/* head conv backward: dF = c_out[b]*dpred; g_out (B,T,C_in) = (W^T*dF)*silu'(gscale*x+gshift) with GN partial sums
 * {sum g, sum g x} per channel and 128-position slot; dw, db as above.
 * C_in: the powers of two 8 ... 256 (first kernels, unchanged) and every multiple of 32 up to 1024 (csrc/ends_wide.hip: a grid
 * dimension over chunks of <= 128 input channels, exact fp32 like the first kernels); C_out <= 16; k in {1, 3, 5}.  The fixed
 * tq_stem_head_bwd_workspace() bytes serve every such shape: the chunked kernel launches no more workgroups per chunk than partial
 * rows of C_out C_in k + 16 floats fit the workspace it is given (25 at 1024 x 16 x 5). */
/* LDS bytes tq_head_conv_bwd_ws needs for a shape; 0 = unsupported shape.  Needs no device. */
size_t tq_head_conv_bwd_lds_bytes(int C_in, int C_out, int ktaps);
int tq_head_conv_bwd_ws(const float* dpred_nct, const float* c_out, const float* x, const float* gscale, const float* gshift,
                        const float* w, float* g_out, float* gstats_partial, float* dw, float* db, int B, int T, int C_in,
                        int C_out, int ktaps, void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- embeddings ------------------------------------------------------------------------------------------- */
/* emb = time_mlp(fourier(t)) (+ cond_mlp(cond)); writes emb (B, E) and silu(emb) (B, E).  E = 4*mc.
 * blocks.py:22-26, unet.py:210-227,383-388.  cond pointers NULL when the model is unconditioned. */
int tq_embed_fwd(const float* t, const float* cond, const float* fourier_w, const float* w0, const float* b0,
                 const float* w2, const float* b2, const float* cw0, const float* cb0, const float* cw2, const float* cb2,
                 float* emb, float* silu_emb, float* hidden /* (B, 2, E) scratch: pre-activations, kept for backward */,
                 int B, int mc, int ncond, hipStream_t stream);

/* All per-ResBlock projections Linear(SiLU(emb)) (unet.py:91-97) as one GEMM: out (B, N) = silu_emb (B, E) W^T + bias. */
int tq_linear_fwd(const float* x, const float* w, const float* bias, float* out, int B, int E, int N, hipStream_t stream);

/* ---- attention -------------------------------------------------------------------------------------------- */
/* QKVAttention (blocks.py:156-190), qkv (B, T, 3*H*D) channels-last with channel order [q heads | k heads | v heads],
 * q and k each scaled by D^-1/4, softmax over keys in fp32, out (B, T, H*D).  D in {32, 64, 128}.
 * The workspace holds the pre-split K / V planes of the second-generation kernels (D = 32 / 64); for D = 128 (first-generation kernel)
 * it holds the partial rows of the key split that kernel uses where its grid is far below the chip (round 6; without a workspace it
 * never splits). */
size_t tq_attention_workspace_bytes(int B, int T, int H, int D);
int tq_attention_fwd(const float* qkv, float* out, float* lse /* (B,H,T) log-sum-exp per query, NULL at inference */,
                     void* workspace /* tq_attention_workspace_bytes(); NULL selects the workspace-free kernel */, int B, int T,
                     int H, int D, hipStream_t stream);
/* attention core on q from qkv and K / V planes already written by tq_conv1d_fwd_qkv (no log-sum-exp output: inference) */
int tq_attention_fwd_presplit(const float* qkv, const void* kv_planes, float* out, int B, int T, int H, int D, int v_format,
                              hipStream_t stream);
/* Backward of tq_attention_fwd (recomputes P from qkv and lse): dqkv (B, T, 3*H*D) from dout (B, T, H*D); delta (B,H,T) is scratch.
 * Replaces the autograd backward of blocks.py:156-190.  workspace: 2 * tq_attention_workspace_bytes() of scratch, nullable.  With it,
 * D = 32 / 64 run the second-generation kernels (one prep pass writes bf16 hi / lo planes of Q, K, V, dO and delta; both passes then
 * stream 16-byte copies, P / dS stay in registers).  D = 128, or workspace == NULL, run the first-generation kernels: two passes,
 * queries-stationary for dq, keys-stationary for dk/dv (no atomics). */
int tq_attention_bwd_ws(const float* qkv, const float* out, const float* dout, const float* lse, float* delta, float* dqkv,
                        void* workspace, int B, int T, int H, int D, hipStream_t stream);
/* The same with the K / V planes the training forward already wrote: `kv_planes` is the `workspace` argument of the
 * tq_attention_fwd call whose backward this is (D = 32 / 64; it must still hold that call's planes: give every attention block of a
 * training plan a workspace of its own).  The prep pass then forms Q, dO and delta only.  `workspace`: as tq_attention_bwd_ws
 * (its first half stays unused).  Gradients bit-identical to tq_attention_bwd_ws. */
int tq_attention_bwd_ws_kv(const float* qkv, const float* out, const float* dout, const float* lse, float* delta, float* dqkv,
                           void* workspace, const void* kv_planes, int B, int T, int H, int D, hipStream_t stream);

/* ABI 8.  Every head size D with 8 | D and 8 <= D <= 256 (attention_hd.hip): the first-generation kernels (attention_g1.hpp, the text that tq_attention_fwd / tq_attention_bwd_ws instantiate for
 * an exact head size, here instantiated with the padding masks) on the smallest tile in
 * {32, 64, 128, 256} that holds the head; channels >= D are zero-filled on load and skipped on store, strides and the D^-1/4 scale are
 * those of the true D.  Same tensors and layouts as tq_attention_fwd / tq_attention_bwd_ws.  The entry points above keep their contract
 * (D in {32, 64, 128}, TQ_ERR_SHAPE otherwise).
 *   tq_attention_head_tile: the tile width for head size D, 0 where there is no kernel (needs no device).
 *   tq_attention_hd_lds_bytes: dynamic LDS of a launch, pass 0 forward, 1 dQ, 2 dK / dV; 0 without a kernel (needs no device).
 *   tq_attention_hd_workspace_bytes: the partial rows of the forward's key split; workspace == NULL never splits.
 *   tq_attention_bwd_hd: `workspace` is reserved (these kernels take no scratch) and may be NULL. */
int tq_attention_head_tile(int D);
size_t tq_attention_hd_lds_bytes(int D, int pass);
size_t tq_attention_hd_workspace_bytes(int B, int T, int H, int D);
int tq_attention_fwd_hd(const float* qkv, float* out, float* lse, void* workspace, int B, int T, int H, int D, hipStream_t stream);
int tq_attention_bwd_hd(const float* qkv, const float* out, const float* dout, const float* lse, float* delta, float* dqkv,
                        void* workspace, int B, int T, int H, int D, hipStream_t stream);

/* ---- EDM / sampler elementwise ------------------------------------------------------------------------------ */
/* Argument checks of the elementwise entry points of this section and the three below (DDPM, losses, VAE, concat), and of
 * tq_fourier_features / tq_gemm_f32_jobs / tq_zero_stuff / tq_pair_sum: a NULL pointer that is not marked nullable, a non-positive
 * B / size / count (n == 0 for the size_t ones) or channels that are not a multiple of 4 return TQ_ERR_ARG before the device is
 * touched (tests/test_side_kernels_host.py).  tq_embed_fwd, tq_linear_fwd and tq_gn_bwd_finalize answer a NULL pointer with
 * TQ_ERR_ARG and a shape they are not built for with TQ_ERR_SHAPE (tq_linear_fwd: E <= 511, the 160 KB of LDS). */
/* per-sample scalars from sigma: c_in, c_out, c_skip, c_noise, loss weight  (edm.py:24-37); sigma_stride 0 = shared */
int tq_edm_scalars(const float* sigma, int sigma_stride, float sigma_data, float* c_in, float* c_out, float* c_skip,
                   float* c_noise, float* lweight, int B, hipStream_t stream);
/* consistency preconditioning scalars (consistency_model.py:69-74) */
int tq_cm_scalars(const float* sigma, int sigma_stride, float sigma_data, float sigma_min, float* c_out, float* c_skip,
                  int B, hipStream_t stream);
/* training noise injection: sigma = exp(eps*P_std + P_mean); x = y + sigma * n   (edm.py:126-129) */
int tq_edm_noise_inject(const float* y, const float* unit_noise, const float* eps, float P_mean, float P_std,
                        float* sigma, float* x_noisy, int B, int n_per_sample, hipStream_t stream);
/* loss = mean(lweight[b] * (pred - y)^2); also d loss / d pred (edm.py:131-134).  loss_out: 1 float (zeroed inside). */
int tq_edm_loss(const float* pred, const float* y, const float* lweight, float* loss_out, float* dpred, int B,
                int n_per_sample, hipStream_t stream);
/* Heun sampler state updates, fp64 state / fp32 network output (edm.py:182-194).
 * euler:   d = (x - D)/s;  x_next = x + d * (float)(s_next - s);  x32 = (float)x_next
 * correct: d' = (x_next - D')/s_next;  x_new = x + (float)(s_next - s) * (0.5 d + 0.5 d');  x32 = (float)x_new */
int tq_heun_euler(const double* x, const float* denoised, const float* sigma, const float* sigma_next, double* d_cur,
                  double* x_next, float* x32, size_t n, hipStream_t stream);
int tq_heun_correct(const double* x, const double* x_next, const float* denoised_next, const double* d_cur,
                    const float* sigma, const float* sigma_next, double* x_out, float* x32, size_t n, hipStream_t stream);
/* x64 = unit_noise64 * sigma0; x32 = (float)x64   (edm.py:160) */
int tq_sampler_init(const double* unit_noise, const float* sigma0, double* x, float* x32, size_t n, hipStream_t stream);

/* Stochastic (churned) sampler, edm.py:198-230: the temporary noise increase x_hat = x + (n * S_noise) * c (lines 205-208), c =
 * sqrt(sigma_hat^2 - sigma^2) formed by the caller in fp32 as the reference does (device scalar).  The Euler / correction steps are
 * tq_heun_euler / tq_heun_correct with sigma_hat in place of sigma (lines 217-228). */
int tq_heun_churn(const double* x, const double* unit_noise, const float* coef, double s_noise, double* x_hat, float* x32,
                  size_t n, hipStream_t stream);

/* out[b] = x[b] + noise[b] * sigma[b]: the two noised copies of the iCT training step (consistency_model.py:150-160). */
int tq_axpy_sigma(const float* x, const float* noise, const float* sigma, float* out, int B, int n_per_sample,
                  hipStream_t stream);

/* ---- DDPM (tqdne/diffusion.py:55-109; ABI 3).  The reference delegates this arithmetic to diffusers' DDPMScheduler, which is not in
 * its lockfile: restated from the published algorithm (Ho et al. 2020), see tqdne_amd/diffusion.py. ------------------------------- */
/* out[b] = a[b] x[b] + c[b] y[b]: the forward process of the training step (noise_scheduler.add_noise, diffusion.py:98). */
int tq_scale_add2(const float* x, const float* y, const float* a, const float* c, float* out, int B, int n_per_sample,
                  hipStream_t stream);
/* One ancestral sampling step (noise_scheduler.step, diffusion.py:77): x0 = (x - sqrt(1 - abar_t) model_out) / sqrt(abar_t) for an
 * epsilon-predicting network, else model_out; clipped to +-clip when clip > 0; out = coef_x0 x0 + coef_xt x + sigma noise
 * (noise nullable: the last step adds none). */
int tq_ddpm_step(const float* x, const float* model_out, const float* noise, float* out, size_t n, int epsilon_prediction,
                 double sqrt_one_minus_abar, double inv_sqrt_abar, double clip, double coef_x0, double coef_xt, double sigma,
                 hipStream_t stream);

/* Weighted pseudo-Huber distance of improved consistency training (consistency_model.py:163-173):
 * loss = mean(w_b (sqrt((pred - target)^2 + c^2) - c)); dpred (nullable) = d loss / d pred.  loss_out is overwritten. */
int tq_pseudo_huber_loss(const float* pred, const float* target, const float* weight, float c, float* loss_out, float* dpred,
                         int B, int n_per_sample, hipStream_t stream);

/* Mean squared error (autoencoder.py:61-63): loss_out = mean((a - b)^2) (overwritten), d (nullable) = 2 (a - b) / n. */
int tq_mse_loss(const float* a, const float* b, float* loss_out, float* d, size_t n, hipStream_t stream);

/* VAE bottleneck (autoencoder.py:37-43,64-66).  enc (B, 2L, T) = [mean | log_std]; eps, z, dz (B, L, T).
 * fwd: z = mean + eps exp(log_std); kl_out (nullable, overwritten) = mean over (b, t) of 0.5 sum_c (mean^2 + std^2 - 2 log_std - 1).
 * bwd: denc (B, 2L, T) = [dz + kw mean | dz eps std + kw (std^2 - 1)], kw = kl_weight / (B T). */
int tq_vae_reparam_fwd(const float* enc, const float* eps, float* z, float* kl_out, int B, int L, int T, hipStream_t stream);
int tq_vae_reparam_bwd(const float* enc, const float* eps, const float* dz, float* denc, float kl_weight, int B, int L, int T,
                       hipStream_t stream);

/* Stem input of a signal-conditioned model (edm.py:108-109): out (B, C0 + C1, T) = [x * scale[b] | cond_signal]; scale nullable. */
int tq_concat_scale(const float* x, const float* scale, const float* cond_signal, float* out, int B, int C0, int C1, int T,
                    hipStream_t stream);

/* ---- NCW <-> channels-last boundary of models with 17 ... 64 signal channels (csrc/boundary.hip) ---------- */
/* The dedicated stem / head kernels above stop at 16 signal channels; a stem or head of 17 ... tq_boundary_max_channels() signal
 * channels is an ordinary 32- / 64-channel contraction and runs as tq_conv1d_fwd / tq_conv1d_bwd_* on channels-last tensors padded to
 * the 32-channel granule.  These two launches are the layout change on either side, with what the dedicated kernels fold into it
 * (edm.py:105-113, consistency_model.py:63-78).  Any B, T >= 1; both go through an LDS tile of 64 positions; additive to ABI 8.
 *   tq_boundary_max_channels(): 64 (needs no device).
 *   tq_nct_to_btc: out (B, T, Cp), 32 | Cp >= C0 + C1 <= 64:  out[b, t, c] = x[b, c, t] * scale[b] for c < C0 (scale nullable = 1),
 *     cond[b, c - C0, t] for C0 <= c < C0 + C1 (cond NULL iff C1 = 0), and exactly 0 for C0 + C1 <= c < Cp -- written on every call.
 *   tq_btc_to_nct: y (B, C, T) = v[b, t, c_off + c] * a[b] + s[b] * skip_src[b, c, t] from v (B, T, Cp), 32 | Cp >= c_off + C,
 *     C <= 64; a nullable (= 1); s and skip_src (B, C, T) both given or both NULL. */
int tq_boundary_max_channels(void);
int tq_nct_to_btc(const float* x_nct, const float* scale, const float* cond_nct, float* out_btc, int B, int C0, int C1, int T, int Cp,
                  hipStream_t stream);
int tq_btc_to_nct(const float* v_btc, const float* a, const float* s, const float* skip_src, float* y_nct, int B, int T, int Cp,
                  int c_off, int C, hipStream_t stream);

/* ---- parameter-free resampling (csrc/resample_plain.hip; added under ABI 8) -------------------------------- */
/* Downsample / Upsample with use_conv=False (blocks.py:29-108; a model built with conv_resample=False): channels-last fp32 tensors,
 * 4 | C <= 1024, T_in >= 2 (TQ_ERR_SHAPE otherwise; a null x / y / dy / dx: TQ_ERR_ARG -- both before the device is touched).
 *   tq_avg_pool2_fwd:   y (B, T_out = T_in / 2, C) = (x[b, 2t] + x[b, 2t+1]) * 0.5f in this association (the bits of avg_pool1d for
 *     finite inputs); the last row of an odd T_in is dropped.
 *   tq_nearest_up2_fwd: y (B, T_out = 2 T_in, C), y[b, 2t] = y[b, 2t+1] = x[b, t].
 *   stats (nullable): (B, ceil(T_out / 128), C, 2) = {sum y, sum y^2} per channel and 128-position slot of the OUTPUT -- what a
 *     TQ_CONV_STATS epilogue leaves and tq_gn_finalize reads with slot = 128.  A workgroup owns whole (b, slot) rows and adds in a fixed
 *     order (no atomics): the same input gives the same bits.
 *   tq_avg_pool2_bwd:   dx (B, T_in, C): dx[b, 2t], dx[b, 2t+1] (+)= 0.5f * dy[b, t] with dy (B, T_in / 2, C); with an odd T_in and
 *     accumulate == 0 the last row of dx is written as zero (left alone when accumulating).
 * The gradient of tq_nearest_up2_fwd is tq_pair_sum. */
int tq_avg_pool2_fwd(const float* x, float* y, float* stats, int B, int T_in, int C, hipStream_t stream);
int tq_nearest_up2_fwd(const float* x, float* y, float* stats, int B, int T_in, int C, hipStream_t stream);
int tq_avg_pool2_bwd(const float* dy, float* dx, int B, int T_in, int C, int accumulate, hipStream_t stream);

/* ---- optimizer (edm.py:240-251, ema.py:24-28) ------------------------------------------------------------- */
/* One launch for the whole model: torch.optim.Adam's update (no weight decay, no amsgrad) on every chunk of the table,
 *   g' = g * grad_scale;  m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= step_size * m / (sqrt(v) * inv_bias2_sqrt + eps)       step_size = lr / (1 - beta1^t), inv_bias2_sqrt = 1/sqrt(1 - beta2^t)
 * preceded by p *= decay_factor (torch.optim.AdamW's decoupled weight decay 1 - lr * wd, autoencoder.py:93-95; 1.0 = Adam) and
 * followed, where ema != NULL, by the EMA callback's lerp  ema += ema_weight * (p - ema)  (ema_weight = 1 - decay).
 * The scalars are doubles (host-side values as torch computes them: 1 - beta in double) and are rounded to fp32 once.
 * `chunks` is a DEVICE array; a chunk is <= TQ_ADAM_CHUNK consecutive elements of one tensor, its pointers 16-byte aligned. */
#define TQ_ADAM_CHUNK 4096
typedef struct TqAdamChunk {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema; /* NULL: no EMA for this chunk */
    int32_t n;
    int32_t reserved;
} TqAdamChunk;
/* skip_flag (nullable: NULL = unconditional): a DEVICE-side predicate -- when `*skip_flag != 0` at execution time the launch leaves
 * parameters, moments and EMA untouched.  The data-parallel trainer passes the range-guard flag of the fp16-range forward scheme
 * (TqConvDesc.range_flag, max-reduced over the ranks): a step whose forward came close to the fp16 range is dropped on the device,
 * without a host synchronisation, before the host has seen the flag and moved the plan to bf16x3.
 * NULL table or n_chunks < 0: TQ_ERR_ARG; n_chunks == 0: 0, nothing launched. */
int tq_adam_ema_step_guarded(const TqAdamChunk* chunks, int n_chunks, double step_size, double beta1, double beta2, double eps,
                             double inv_bias2_sqrt, double ema_weight, double grad_scale, double decay_factor,
                             const int32_t* skip_flag, hipStream_t stream);

/* torch.optim.RAdam with its defaults (no weight decay, the consistency model's optimizer) on the same chunk table, behind the same
 * device-side predicate, followed by the same EMA lerp:
 *   g' = g * grad_scale;  m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   rect != 0:  p -= step_size * m * (rect / (sqrt(v) + eps))       rect == 0:  p -= step_size * m
 * The host, which knows t, forms step_size = lr / (1 - beta1^t) and, where rho_t > 5, rect = r_t * sqrt(1 - beta2^t) in double
 * (r_t: the variance rectification); rect = 0 selects the un-rectified form of the first steps.  eps is added to sqrt(v) BEFORE
 * the sqrt(1 - beta2^t) factor, as torch does.  NULL table or n_chunks <= 0: TQ_ERR_ARG, nothing launched. */
int tq_radam_ema_step_guarded(const TqAdamChunk* chunks, int n_chunks, double step_size, double beta1, double beta2, double eps,
                              double rect, double ema_weight, double grad_scale, const int32_t* skip_flag, hipStream_t stream);

/* Gradient clipping and gradient-norm tracking inside the one-launch update (what pl.Trainer's gradient_clip_val /
 * gradient_clip_algorithm do for the reference): decided on the device, no host synchronisation, no extra pass over parameters or
 * moments.  Two small launches in front of the update form the norm over the optimizer's own chunk table:
 *   tq_grad_sumsq:     one workgroup per chunk, reads g only: partials[i] = sum of g^2 over chunk i (a DEVICE array of n_chunks
 *     doubles); squares and sums in fp64 from the fp32 values, in a fixed order (no atomics): the same gradients give the same bits.
 *   tq_grad_clip_coef: one workgroup adds the partials in a fixed order in fp64 (any n_chunks) and writes two DEVICE floats,
 *       out[0] = norm = (float)(grad_scale * sqrt(total))            the norm of the scaled gradient, before clipping
 *       out[1] = coef = min(1, max_norm / (norm + 1e-6f))            in fp32, as torch.nn.utils.clip_grad_norm_ forms it
 *     max_norm <= 0: coef = 1 (tracking only).  Non-finite norms are not special: a NaN norm gives a NaN coefficient, as in torch
 *     (error_if_nonfinite=False).
 * The _clipped entry points are the _guarded ones with two more arguments; per element, every step rounded to fp32 in torch's order,
 *   g' = g * grad_scale;   clip_coef != NULL: g' *= *clip_coef;   clip_value > 0: g' = clamp(g', -clip_value, clip_value)
 * and the update goes on with g' as above (a NaN stays a NaN through the clamp, as in clip_grad_value_).  `clip_coef` is a DEVICE
 * float (out + 1 of tq_grad_clip_coef), read once per workgroup like `skip_flag`; NULL with clip_value == 0 runs the kernel of the
 * _guarded entry point.  A raised `skip_flag` still drops the whole update.
 * NULL table / partials / out, n_chunks <= 0 or a negative clip_value: TQ_ERR_ARG, nothing launched. */
int tq_grad_sumsq(const TqAdamChunk* chunks, int n_chunks, double* partials, hipStream_t stream);
int tq_grad_clip_coef(const double* partials, int n_chunks, double grad_scale, double max_norm, float* out, hipStream_t stream);
int tq_adam_ema_step_clipped(const TqAdamChunk* chunks, int n_chunks, double step_size, double beta1, double beta2, double eps,
                             double inv_bias2_sqrt, double ema_weight, double grad_scale, double decay_factor,
                             const int32_t* skip_flag, const float* clip_coef, double clip_value, hipStream_t stream);
int tq_radam_ema_step_clipped(const TqAdamChunk* chunks, int n_chunks, double step_size, double beta1, double beta2, double eps,
                              double rect, double ema_weight, double grad_scale, const int32_t* skip_flag, const float* clip_coef,
                              double clip_value, hipStream_t stream);

/* The second half of the EMA callback (ema.py:30-48: EMA weights into the module before every validation / test / predict pass, the
 * training weights back afterwards) as an exchange in place: for every chunk with ema != NULL, p[i] <-> ema[i] for
 * i < n.  One launch for the whole model, the optimizer kernel's geometry (one workgroup of 256 threads per chunk, 16-byte body, one-word
 * tail), no second copy of the weights.  Only p, ema and n of a chunk are read (g, m, v may be NULL); chunks whose ema is NULL are left
 * alone.  Bit patterns are moved, nothing is rounded: NaN payloads, infinities, -0.0 and denormals arrive unchanged, and two calls restore
 * both sides bit for bit.  The caller invalidates whatever it derived from the parameters (DataParallelTrainer.ema_weights bumps their
 * autograd versions, so the packed weights follow).
 * NULL table with n_chunks > 0, or n_chunks < 0: TQ_ERR_ARG; n_chunks == 0: 0, nothing launched. */
int tq_ema_swap(const TqAdamChunk* chunks, int n_chunks, hipStream_t stream);

/* ---- signal representation either side of the path (representation.py:41-60, MovingAverageEnvelope) ------- */
/* x (N, C, T) fp32 NCW -> out (N, 2C, T) fp32: channels [0, C) = x / (env + eps), [C, 2C) = log(env + log_eps) - log(log_eps)/2,
 * env = mean of |x| over [t - W/2, t + (W-1)/2] with zeros outside the signal (np.convolve(..., mode="same")); float64 inside,
 * like numpy.  Requires window <= T (the reference's np.convolve changes length otherwise) and window <= 4096. */
int tq_envelope_fwd(const float* x, float* out, int N, int C, int T, int window, double log_eps, double eps, hipStream_t stream);
/* repr (N, 2C, T) -> waveform (N, C, T): scaled * (exp(log_env + log(log_eps)/2) + eps)   (representation.py:56-59) */
int tq_envelope_inv(const float* repr, float* out, int N, int C, int T, double log_eps, double eps, hipStream_t stream);

/* ---- classifier head and its loss (csrc/classifier.hip; added under ABI 8; classifier.py:39-64) ------------------ */
/* The head behind the encoder's output conv, read where that conv left it: h (B, T, C) channels-last, contiguous.
 *   pooled[b, c] = (sum_t h[b, t, c]) / T;   a1 = W1 silu(pooled) + b1;   emb = W2 silu(a1) + b2;   logits = W3 emb + b3
 * W1, W2 (C, C), W3 (K, C) row-major as nn.Linear keeps them; pooled, a1 (pre-activation), emb (B, C) and logits (B, K) are
 * overwritten.  Exact fp32 (FMA, expf, true division), fp32 accumulation; every sum runs in an order that depends on (T, C, K) alone
 * and there are no atomics, so two calls on the same inputs give the same bits -- in all three entry points.  One workgroup per
 * sample (any B).  Every pointer must be 16-byte aligned.
 * Limits, answered without a device: 32 | C <= tq_classifier_head_max_channels() = 1024, K <= tq_classifier_head_max_classes() = 1024
 * (the reference trains 36 classes).
 * Argument checks, before the device is touched: a NULL pointer that is not marked nullable or a non-positive B / T / C / K returns
 * TQ_ERR_ARG (checked first); a C that is not a multiple of 32 or above the limit, or a K above the limit, TQ_ERR_SHAPE.
 *   tq_classifier_head_fwd: logits nullable (embed() only: W3, b3 and K are then not read and may be NULL / anything).
 *   tq_cross_entropy: torch.nn.functional.cross_entropy(logits, labels, weight, ignore_index, reduction='mean'):
 *       loss = sum_i w[y_i] nll_i / sum_i w[y_i] over the labels that are not ignored, nll_i = log sum_k exp(x_ik - max_k x_ik) + max_k x_ik
 *       - x_i,y_i;  dlogits[i, k] = w[y_i] (softmax(x_i)[k] - [k == y_i]) / sum_i w[y_i], and zero in the rows of ignored labels.
 *     labels int64 (B); weight (K) nullable (= 1); loss_out (1 float) overwritten; dlogits (B, K) nullable.  The per-sample terms are in
 *     fp32, their sums over the samples in fp64, by a fixed tree of one workgroup.  A label outside [0, K) that is not ignore_index is
 *     treated as ignored (torch raises; the device cannot).  A batch in which EVERY label is ignored returns loss = NaN (0 / 0, as
 *     torch does) and dlogits = 0.
 *   tq_classifier_head_bwd: from dlogits (B, K) and the saved pooled / a1 / emb of the forward: dW3 (K, C), db3 (K), dW2, dW1 (C, C),
 *     db2, db1 (C) -- sums over the samples b = 0 .. B-1 in order, OVERWRITTEN, not accumulated -- and dh[b, t, c] = dpooled[b, c] / T,
 *     (B, T, C) channels-last: the gradient buffer of the encoder's output conv.  Three launches (per-sample chain, weight gradients,
 *     broadcast).  W3 == NULL: `dlogits` is d emb (B, C) itself (the backward of embed()); dW3 / db3 are not written and K is not read.
 *     workspace: tq_classifier_head_bwd_workspace(B, C) bytes (5 B C floats; 0 for a non-positive B / C), 16-byte
 *     aligned; fewer workspace_bytes than that: TQ_ERR_ARG. */
int tq_classifier_head_max_channels(void);
int tq_classifier_head_max_classes(void);
size_t tq_classifier_head_bwd_workspace(int B, int C);
int tq_classifier_head_fwd(const float* h, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                           const float* b3, float* pooled, float* a1, float* emb, float* logits, int B, int T, int C, int K,
                           hipStream_t stream);
int tq_cross_entropy(const float* logits, const int64_t* labels, const float* weight, int64_t ignore_index, float* loss_out,
                     float* dlogits, int B, int K, hipStream_t stream);
int tq_classifier_head_bwd(const float* dlogits, const float* pooled, const float* a1, const float* emb, const float* W1,
                           const float* W2, const float* W3, float* dW3, float* db3, float* dW2, float* db2, float* dW1, float* db1,
                           float* dh, void* workspace, size_t workspace_bytes, int B, int T, int C, int K, hipStream_t stream);

/* ---- LogSpectrogram (csrc/spectrogram.hip; added under ABI 8; representation.py:63-175) ------------------------- */
/* The STFT of librosa.stft(y, n_fft, hop_length) at its defaults (win_length = n_fft, periodic Hann, center=True with n_fft / 2
 * zeros on either side, F = 1 + T / hop frames) and librosa.griffinlim(S, n_iter, hop_length, n_fft, momentum, init="random",
 * random_state) in one launch.  Exact fp32 arithmetic (FMA, logf / expf / hypotf, true division; no fast-math functions, no
 * atomics): every sum has an order that depends on (n_fft, hop, F) alone, so results are bit-reproducible and a waveform's result
 * does not depend on the rest of the batch.  Built for n_fft = 256 with hop 32 or 64; the Nyquist row is never stored (the
 * reference drops it after the STFT and feeds zeros for it to the inversion).
 *   tables: a device copy of what tq_spectrogram_tables wrote -- Hann window, cos and sin of 2 pi m / n_fft (n_fft floats each) and,
 *     for F > 0, the window sum-square of F frames (hop (F - 1) + n_fft floats), all computed in double.  A table made for F frames
 *     serves tq_stft_fwd for any length and tq_griffinlim for exactly F frames.  tq_spectrogram_table_floats: its length (0 for
 *     arguments the kernels refuse).  Both are host functions and touch no device.
 *   tq_stft_fwd: x (N, T) -> either or both of spec (N, n_fft / 2, F) as interleaved (re, im) fp32 and repr (N, n_fft / 2, F) =
 *     2 (log max(|S|, clip) - log clip) / (log_max - log clip) - 1, in one launch.  Any T >= n_fft.
 *   tq_griffinlim: in (N, n_fft / 2, F) -> out (N, hop (F - 1)).  `in` holds magnitudes, or with log_input != 0 the normalised
 *     log-magnitudes above, mapped back by exp((r + 1) / 2 (log_max - log clip) + log clip) as they are loaded.  phase: (n_fft / 2, F)
 *     interleaved (cos, sin) of the initial phases, shared by all N waveforms (the reference draws
 *     RandomState(0).random((n_fft / 2 + 1, F)) for every waveform).  Each of the n_iter iterations: y = istft(A), R = stft(y),
 *     C = R - momentum / (1 + momentum) * Rprev (no such term in the first), A = S C / (|C| + FLT_MIN); the result is istft(A).
 *     One workgroup per waveform holds all state on chip; F <= tq_griffinlim_max_frames(n_fft, hop) = 128.
 * Argument checks, before the device is touched: NULL x / in / out / tables / phase, neither spec nor repr, n_iter < 0, a
 * non-positive n_fft or hop, a hop that does not divide n_fft, or (where the log map is used) clip <= 0 or log_max <= log clip:
 * TQ_ERR_ARG; an n_fft / hop without a kernel, N < 1, T < n_fft (hop (F - 1) < n_fft) or F above the limit: TQ_ERR_SHAPE.  The
 * limit query returns the same codes for the same n_fft / hop. */
int tq_griffinlim_max_frames(int n_fft, int hop);
size_t tq_spectrogram_table_floats(int n_fft, int hop, int F);
int tq_spectrogram_tables(int n_fft, int hop, int F, float* host_out);
int tq_stft_fwd(const float* x, float* spec, float* repr, const float* tables, int N, int T, int n_fft, int hop, double clip,
                double log_max, hipStream_t stream);
int tq_griffinlim(const float* in, float* out, const float* tables, const float* phase, int N, int F, int n_fft, int hop, int n_iter,
                  double momentum, int log_input, double clip, double log_max, hipStream_t stream);

/* ---- ground-motion intensity measures (csrc/intensity.hip; added under ABI 8; scripts/seismo_evaluations) ---------- */
/* Directional peaks of N two-component waveforms, the input of GMRotDpp / RotDpp (smtk's semantics restated):
 *     peaks[n, k, phi] = max_t | sx_k(t) cos phi + sy_k(t) sin phi |,   phi = 0 .. 179 degrees (0 and 90 exactly unrotated),
 * over the T - 1 samples of K = 3 + P series pairs: k = 0 the ground acceleration x[:-1], k = 1 its velocity
 * dt * cumulative_trapezoid(a, initial 0), k = 2 the displacement (the same of v), k = 3 + i the absolute acceleration
 * -(2 xi w u' + w^2 u) of the oscillator u'' + 2 xi w u' + w^2 u = -a(t), w = 2 pi / periods[i], from rest, a linear between
 * samples, solved exactly from sample to sample (Nigam-Jennings; output sample j is the state at (j + 1) dt).
 *   tables: a device copy of what tq_oscillator_tables wrote (tq_oscillator_table_floats(P) = 360 + 12 P floats): cos and sin of
 *     the 180 angles, then per period the step of the scaled state s = (w^2 u, w u'), s' = A s + B0 a_j + B1 a_(j+1), as
 *     A11 A12 A21 A22 B0[0] B0[1] B1[0] B1[1] 2xi 0 0 0, all computed in double.  Host functions; they touch no device.
 *   tq_rotd_peaks: x, y (N, T) -> peaks (N, 3 + P, 180), one launch, no atomics, no workspace; any T >= 2 (there is no limit on
 *     T).  Every sum has one order that depends on (T, P) alone: launches repeat bit for bit and a waveform's values do not depend
 *     on the rest of the batch.  A waveform with a non-finite sample in either component gets NaN in all of its values.
 * Argument checks, before the device is touched: NULL pointers, P < 0, dt not positive and finite, damping outside [0, 1), a period
 * not positive and finite: TQ_ERR_ARG; N < 1 or T < 2: TQ_ERR_SHAPE. */
size_t tq_oscillator_table_floats(int P);
int tq_oscillator_tables(const double* periods, int P, double dt, double damping, float* host_out);
int tq_rotd_peaks(const float* x, const float* y, const float* tables, float* peaks, int N, int T, int P, double dt,
                  hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TQDNE_HIP_H */
