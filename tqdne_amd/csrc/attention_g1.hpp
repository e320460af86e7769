// 1-D self-attention core of the tqdne UNet (QKVAttention, tqdne/blocks.py:156-190) for gfx950, first generation: forward, key-split
// combine, and the two backward passes, written once for every head size.
//
//   qkv (B, T, 3*H*d) channels-last, channel order [q heads | k heads | v heads]
//   out[b, t, h*d + c] = sum_s softmax_s( (q*d^-1/4) . (k*d^-1/4) )[t, s] * v[s, c]
//
// Flash-style: the (T x T) score matrix of the reference (4 MB per sample per block at T=512) never
// exists in HBM.  One workgroup = 64 queries of one (b, head), 4 waves x 16 queries; keys/values are
// streamed in tiles of 64 through LDS; QK^T and PV run on v_mfma_f32_16x16x32_bf16 with the same
// bf16 hi/lo 3-product split as the convolutions (scores feed an exponential, so single bf16 is not
// accurate enough for the 1e-3 parity target); the online softmax is fp32, as in the reference.
//
// Every kernel is a template <int D, bool PAD> on the tile width D in {32, 64, 128, 256}:
//   PAD = false  the head size IS the tile (attention.hip: 32 / 64 / 128, the paper model).  d is the constant D, the run-time
//                argument is ignored, and every in_head() test folds away.
//   PAD = true   any head size d with 8 | d on the smallest tile D >= d (attention_hd.hip).  d is the last kernel argument; the
//                channels >= d are zero-filled on load and skipped on store.
// The run-time head size is the LAST kernel argument on purpose: in the middle of the list it regroups the scalar argument loads
// of the PAD = false instantiations and renumbers their scalar registers.  The kernels are instantiated directly as __global__
// templates: a __global__ wrapper around a shared __device__ body changes the register allocation (DESIGN_LOG.md).
//
// The 256-wide tile: one workgroup per CU (its LDS footprint allows no more, and two would spill), and the dK / dV pass streams
// 32-query tiles instead of 64 (64 rows of the Q / dO images come to 172,544 B, over the 163,840 B a workgroup may declare).
//
// Included by attention.hip and attention_hd.hip, two translation units so that the build compiles them in parallel; everything is
// in the unnamed namespace, so each unit holds the instantiations it asks for and nothing else.
#pragma once
#include "common.hpp"
#include "../../include/tqdne_hip.h"

using namespace tq;

namespace {

constexpr int QT = 64;   // queries per workgroup
constexpr int KTILE = 64;  // keys per tile
constexpr int ATT_KSPLIT_MAX = 8;
constexpr int occupancy(int DT) { return DT == 256 ? 1 : 2; }      // workgroups per CU the kernels are compiled for
constexpr int dkv_queries(int DT) { return DT == 256 ? 32 : 64; }  // queries per streamed tile of the dK / dV pass

// channel c of the tile belongs to the head (PAD = false: the tile is the head, and the test folds away)
template <bool PAD>
__device__ __forceinline__ bool in_head(int c, int d) { return !PAD || c < d; }

// dynamic LDS of the three kernels on tile D (QB: queries per streamed tile of the dK / dV pass)
constexpr size_t fwd_lds_bytes(int D) { return (size_t)2 * KTILE * (D * 2 + 16) + 2 * D * (KTILE * 2 + 16) + 4 * 2 * 16 * (KTILE * 2 + 16); }
constexpr size_t dq_lds_bytes(int D) { return (size_t)4 * 64 * (D * 2 + 16) + 4 * 2 * 16 * (64 * 2 + 16); }
constexpr size_t dkv_lds_bytes(int D, int QB) { return (size_t)4 * QB * (D * 2 + 16) + 128 * sizeof(float) + 4 * 4 * 16 * (QB * 2 + 16); }

// key split of the forward (needs the workspace): where the grid would leave most of the chip idle -- under 128 workgroups for 256
// compute units -- deal the key tiles over as many workgroups as bring it to ~256
inline int key_split(int wgs, int nkt, const void* workspace) {
    int ksplit = 1;
    if (workspace && wgs < 128) {
        ksplit = 256 / wgs;
        if (ksplit > nkt) ksplit = nkt;
        if (ksplit > ATT_KSPLIT_MAX) ksplit = ATT_KSPLIT_MAX;
        if (ksplit < 1) ksplit = 1;
    }
    return ksplit;
}

// ``ksplit`` > 1 -- the key tiles of one (b, head, query tile) are dealt over ``ksplit`` workgroups, each leaving its
// un-normalised output rows, running maxima and row sums in ``part``; attn_combine_kernel merges them.  For grids far below the chip
// (the tiny config's middle block at B = 4: one head of 128 channels, 32 workgroups walking 8 key tiles each; one head of 256
// channels at B = 2, T = 512: 16 workgroups).
template <int D, bool PAD>
__global__ __launch_bounds__(256, occupancy(D)) void attention_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                      float* __restrict__ lse, int T, int H, float scale, int ksplit,
                                                                      float* __restrict__ part, int d_arg) {
    const int d = PAD ? d_arg : D;   // head size
    constexpr int KS = D / 32;       // k-steps over the head dimension
    constexpr int CB = D / 16;       // output column blocks
    constexpr int KROW = D * 2 + 16;   // bytes per key row of the K image (padded)
    constexpr int VROW = KTILE * 2 + 16;  // bytes per channel row of the V^T image
    constexpr int PROW = KTILE * 2 + 16;  // bytes per query row of the P image
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* k_hi = lds;
    unsigned char* k_lo = k_hi + KTILE * KROW;
    unsigned char* v_hi = k_lo + KTILE * KROW;
    unsigned char* v_lo = v_hi + D * VROW;
    unsigned char* p_base = v_lo + D * VROW;  // [4 waves][2 planes][16][PROW]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nqt = (T + QT - 1) / QT;
    const int grp = nqt * ksplit;
    int bid = xcd_group_id(blockIdx.x, grp, gridDim.x / grp);  // the tiles of one (b, h) share an XCD's L2
    const int ksid = bid % ksplit; bid /= ksplit;
    const int qt = bid % nqt; bid /= nqt;
    const int h = bid % H;
    const int b = bid / H;
    const int C3 = 3 * H * d;
    const float* base = qkv + (size_t)b * T * C3;
    const int q0 = qt * QT + wave * 16;
    unsigned char* p_hi = p_base + wave * 2 * 16 * PROW;
    unsigned char* p_lo = p_hi + 16 * PROW;

    // ---- Q fragments (A operand: row = query l&15, k = d) kept in registers for the whole kernel
    Frag qh[KS], ql[KS];
    {
        const int q = q0 + (lane & 15);
        const bool ok = q < T;
        const float* qp = base + (size_t)(ok ? q : 0) * C3 + h * d + 8 * (lane >> 4);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            float4 a = make_float4(0, 0, 0, 0), c = a;
            if (ok && in_head<PAD>(ks * 32 + 8 * (lane >> 4), d)) {
                a = *reinterpret_cast<const float4*>(qp + ks * 32);
                c = *reinterpret_cast<const float4*>(qp + ks * 32 + 4);
            }
            const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                __bf16 hh, ll;
                split_bf16(v[j] * scale, hh, ll);
                qh[ks].v[j] = hh; ql[ks].v[j] = ll;
            }
        }
    }

    f32x4 o[CB];
#pragma unroll
    for (int i = 0; i < CB; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run[4], l_run[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; }

    const int nkt = (T + KTILE - 1) / KTILE;
    const int kt_begin = ksid * nkt / ksplit, kt_end = (ksid + 1) * nkt / ksplit;   // (ksplit <= nkt: never empty)
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const int s0 = kt * KTILE;
        __syncthreads();  // previous tile fully consumed
        // ---- stage K tile: thread -> (key = i / (D/4), 4 channels)
        for (int i = tid; i < KTILE * (D / 4); i += 256) {
            const int key = i / (D / 4), c4 = i % (D / 4);
            float4 v = make_float4(0, 0, 0, 0);
            if (s0 + key < T && in_head<PAD>(4 * c4, d)) v = *reinterpret_cast<const float4*>(base + (size_t)(s0 + key) * C3 + (H + h) * d + 4 * c4);
            const float u[4] = {v.x * scale, v.y * scale, v.z * scale, v.w * scale};
            bf16x4 hv, lv;
#pragma unroll
            for (int j = 0; j < 4; ++j) { __bf16 hh, ll; split_bf16(u[j], hh, ll); hv[j] = hh; lv[j] = ll; }
            *reinterpret_cast<bf16x4*>(k_hi + key * KROW + c4 * 8) = hv;
            *reinterpret_cast<bf16x4*>(k_lo + key * KROW + c4 * 8) = lv;
        }
        // ---- stage V^T tile: thread -> (4 channels c4, 4 keys kg), transposed in registers
        for (int i = tid; i < (KTILE / 4) * (D / 4); i += 256) {
            const int c4 = i % (D / 4), kg = i / (D / 4);
            float4 v[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int key = s0 + 4 * kg + kk;
                v[kk] = make_float4(0, 0, 0, 0);
                if (key < T && in_head<PAD>(4 * c4, d)) v[kk] = *reinterpret_cast<const float4*>(base + (size_t)key * C3 + (2 * H + h) * d + 4 * c4);
            }
            const float cols[4][4] = {{v[0].x, v[1].x, v[2].x, v[3].x}, {v[0].y, v[1].y, v[2].y, v[3].y},
                                      {v[0].z, v[1].z, v[2].z, v[3].z}, {v[0].w, v[1].w, v[2].w, v[3].w}};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bf16x4 hv, lv;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) { __bf16 hh, ll; split_bf16(cols[j][kk], hh, ll); hv[kk] = hh; lv[kk] = ll; }
                *reinterpret_cast<bf16x4*>(v_hi + (4 * c4 + j) * VROW + kg * 8) = hv;
                *reinterpret_cast<bf16x4*>(v_lo + (4 * c4 + j) * VROW + kg * 8) = lv;
            }
        }
        __syncthreads();

        // ---- S = Q K^T  (16 queries x 64 keys per wave)
        f32x4 s[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            s[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int key = cb * 16 + (lane & 15);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                Frag bh, bl;
                const int off = key * KROW + (ks * 4 + (lane >> 4)) * 16;
                bh.u = *reinterpret_cast<const uint4*>(k_hi + off);
                bl.u = *reinterpret_cast<const uint4*>(k_lo + off);
                s[cb] = mfma_x3(qh[ks].v, ql[ks].v, bh.v, bl.v, s[cb]);
            }
        }
        // ---- online softmax; lane holds rows 4*(lane>>4)+r, column cb*16 + (lane&15)
        float alpha[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = -INFINITY;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const bool valid = (s0 + cb * 16 + (lane & 15)) < T;
                if (!valid) s[cb][r] = -INFINITY;
                mx = fmaxf(mx, s[cb][r]);
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            const float m_new = fmaxf(m_run[r], mx);
            alpha[r] = (m_run[r] == -INFINITY) ? 0.f : __expf(m_run[r] - m_new);
            float rs = 0.f;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const float pv = (s[cb][r] == -INFINITY) ? 0.f : __expf(s[cb][r] - m_new);
                s[cb][r] = pv;
                rs += pv;
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) rs += __shfl_xor(rs, off);
            l_run[r] = l_run[r] * alpha[r] + rs;
            m_run[r] = m_new;
        }
#pragma unroll
        for (int i = 0; i < CB; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[i][r] *= alpha[r];
        // ---- P -> LDS (per-wave image [query][key], bf16 hi/lo)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                __bf16 hh, ll;
                split_bf16(s[cb][r], hh, ll);
                const int off = (4 * (lane >> 4) + r) * PROW + (cb * 16 + (lane & 15)) * 2;
                *reinterpret_cast<__bf16*>(p_hi + off) = hh;
                *reinterpret_cast<__bf16*>(p_lo + off) = ll;
            }
        __syncthreads();
        // ---- O += P V   (A = P: row = query l&15, k = key; B = V^T rows = channel)
#pragma unroll
        for (int ks = 0; ks < KTILE / 32; ++ks) {
            Frag ph, pl;
            const int poff = (lane & 15) * PROW + (ks * 4 + (lane >> 4)) * 16;
            ph.u = *reinterpret_cast<const uint4*>(p_hi + poff);
            pl.u = *reinterpret_cast<const uint4*>(p_lo + poff);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                Frag vh, vl;
                const int voff = (cb * 16 + (lane & 15)) * VROW + (ks * 4 + (lane >> 4)) * 16;
                vh.u = *reinterpret_cast<const uint4*>(v_hi + voff);
                vl.u = *reinterpret_cast<const uint4*>(v_lo + voff);
                o[cb] = mfma_x3(ph.v, pl.v, vh.v, vl.v, o[cb]);
            }
        }
    }
    if (ksplit > 1) {   // ---- partial result: rows relative to this split's running maximum, with (m, l) behind them
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = q0 + 4 * (lane >> 4) + r;
            if (q < T) {
                // (rows of D + 4 floats: 16-byte aligned; the tile's columns >= d are stored as the zeros they are)
                float* pr = part + ((((size_t)b * H + h) * ksplit + ksid) * T + q) * (D + 4);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) pr[cb * 16 + (lane & 15)] = o[cb][r];
                if ((lane & 15) == 0) { pr[D] = m_run[r]; pr[D + 1] = l_run[r]; }
            }
        }
        return;
    }
    // ---- normalise and store
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * (lane >> 4) + r;
        if (q < T) {
            const float inv = 1.0f / l_run[r];
            if (lse && (lane & 15) == 0) lse[((size_t)b * H + h) * T + q] = m_run[r] + __logf(l_run[r]);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
                if (in_head<PAD>(cb * 16 + (lane & 15), d))
                    out[((size_t)b * T + q) * (H * d) + h * d + cb * 16 + (lane & 15)] = o[cb][r] * inv;
        }
    }
}

// out[b, q, h d + c] = sum_s o_s[c] e^(m_s - M) / sum_s l_s e^(m_s - M), M = max_s m_s; one thread per (row, 4 channels of the tile)
template <int D, bool PAD>
__global__ __launch_bounds__(256) void attn_combine_kernel(const float* __restrict__ part, float* __restrict__ out, float* __restrict__ lse,
                                                           int T, int H, int ksplit, size_t n, int d_arg) {
    const int d = PAD ? d_arg : D;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c4 = (int)(i % (D / 4));
    size_t row = i / (D / 4);
    const int q = (int)(row % T); row /= T;
    const int h = (int)(row % H);
    const int b = (int)(row / H);
    if (!in_head<PAD>(4 * c4, d)) return;
    const float* pr = part + ((((size_t)b * H + h) * ksplit) * T + q) * (D + 4);
    const size_t stride = (size_t)T * (D + 4);
    float M = -INFINITY;
    for (int s = 0; s < ksplit; ++s) M = fmaxf(M, pr[s * stride + D]);
    float L = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < ksplit; ++s) {
        const float w = __expf(pr[s * stride + D] - M);
        L += pr[s * stride + D + 1] * w;
        const float4 o = *reinterpret_cast<const float4*>(pr + s * stride + 4 * c4);
        acc.x += o.x * w; acc.y += o.y * w; acc.z += o.z * w; acc.w += o.w * w;
    }
    const float inv = 1.0f / L;
    *reinterpret_cast<float4*>(out + ((size_t)b * T + q) * (H * d) + h * d + 4 * c4) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    if (lse && c4 == 0) lse[((size_t)b * H + h) * T + q] = M + __logf(L);
}

// =================================================================================================
// Attention backward (flash-style recompute).  Per (b, head), with Qs = scale*Q, Ks = scale*K:
//   S = Qs Ks^T,  P = exp(S - lse),  O = P V,   delta_i = sum_d dO[i,d] O[i,d]
//   dV = P^T dO,  dP = dO V^T,  dS = P o (dP - delta),  dQ = scale * dS Ks,  dK = scale * dS^T Qs
// Pass A keeps 64 queries stationary and streams key tiles (dQ); pass B keeps 64 keys stationary and streams
// query tiles (dK, dV).  No atomics; P is recomputed in each pass.  Operands whose MFMA k index is the LDS row
// (key / query) are fetched with ds_read_b64_tr_b16 from the same row-major images the other products read.
// =================================================================================================

// 4 x 4 16-bit elements of an LDS image, transposed (ds_read_b64_tr_b16); the second-generation kernels of attention.hip use it too
typedef short s16x4b __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 tr_read(const unsigned char* p) {
    s16x4b v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4b*)(p));
    union { s16x4b s; uint2 u; } c;
    c.s = v;
    return c.u;
}

// delta[b, h, t] = sum_c dO[b, t, h D + c] O[b, t, h D + c].  The head size D is a run-time argument for every caller, so there is one
// kernel per translation unit; PAD only tells the two units' copies apart by name.
template <bool PAD>   // (a name tag only: the body does not use it)
__global__ void attn_delta_kernel(const float* __restrict__ o, const float* __restrict__ d_o, float* __restrict__ delta, int T,
                                  int H, int D, size_t n) {
    // one wave per (b, t, h) row would be wasteful for D <= 128: one thread per row, 16-byte loads
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int h = (int)(i % H);
    const size_t bt = i / H;
    const int t = (int)(bt % T);
    const size_t b = bt / T;
    const float4* po = reinterpret_cast<const float4*>(o + bt * (size_t)(H * D) + h * D);
    const float4* pd = reinterpret_cast<const float4*>(d_o + bt * (size_t)(H * D) + h * D);
    float a = 0.f;
    for (int j = 0; j < D / 4; ++j) {
        const float4 x = po[j], y = pd[j];
        a += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    delta[(b * H + h) * T + t] = a;
}

// stage a [ROWS rows][D] fp32 tile (rows of `src` with row stride `rs`, optional scale) as bf16 hi/lo row-major images
template <int D, bool PAD, int ROWS = 64>
__device__ __forceinline__ void stage_rows(const float* src, size_t rs, int row0, int T, int d, float scale, unsigned char* hi,
                                           unsigned char* lo, int ROWB) {
    for (int i = threadIdx.x; i < ROWS * (D / 4); i += 256) {
        const int r = i / (D / 4), c4 = i % (D / 4);
        float4 v = make_float4(0, 0, 0, 0);
        if (row0 + r < T && in_head<PAD>(4 * c4, d)) v = *reinterpret_cast<const float4*>(src + (size_t)(row0 + r) * rs + 4 * c4);
        const float u[4] = {v.x * scale, v.y * scale, v.z * scale, v.w * scale};
        bf16x4 hv, lv;
#pragma unroll
        for (int j = 0; j < 4; ++j) { __bf16 hh, ll; split_bf16(u[j], hh, ll); hv[j] = hh; lv[j] = ll; }
        *reinterpret_cast<bf16x4*>(hi + r * ROWB + c4 * 8) = hv;
        *reinterpret_cast<bf16x4*>(lo + r * ROWB + c4 * 8) = lv;
    }
}

// A-operand fragments (row = l&15 of a 16-row block starting at row0, k = channel) straight from global memory
template <int D, bool PAD>
__device__ __forceinline__ void load_row_frags(const float* src, size_t rs, int row, bool ok, int d, float scale, Frag (&fh)[D / 32],
                                               Frag (&fl)[D / 32]) {
    const int lane = threadIdx.x & 63;
    const float* p = src + (size_t)(ok ? row : 0) * rs + 8 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
        float4 a = make_float4(0, 0, 0, 0), c = a;
        if (ok && in_head<PAD>(ks * 32 + 8 * (lane >> 4), d)) {
            a = *reinterpret_cast<const float4*>(p + ks * 32);
            c = *reinterpret_cast<const float4*>(p + ks * 32 + 4);
        }
        const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) { __bf16 hh, ll; split_bf16(v[j] * scale, hh, ll); fh[ks].v[j] = hh; fl[ks].v[j] = ll; }
    }
}

// write a 16 x (16 N) accumulator tile set (N column blocks) as bf16 hi/lo [row][col] image for use as an A operand
template <int N>
__device__ __forceinline__ void acc_to_image(const f32x4 (&s)[N], unsigned char* hi, unsigned char* lo, int ROWB) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int cb = 0; cb < N; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            __bf16 hh, ll;
            split_bf16(s[cb][r], hh, ll);
            const int off = (4 * (lane >> 4) + r) * ROWB + (cb * 16 + (lane & 15)) * 2;
            *reinterpret_cast<__bf16*>(hi + off) = hh;
            *reinterpret_cast<__bf16*>(lo + off) = ll;
        }
}

// ---- pass A: dQ ------------------------------------------------------------------------------------------
template <int D, bool PAD>
__global__ __launch_bounds__(256, occupancy(D)) void attention_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                                             const float* __restrict__ lse, const float* __restrict__ delta,
                                                                             float* __restrict__ dqkv, int T, int H, float scale, int d_arg) {
    const int d = PAD ? d_arg : D;
    constexpr int KS = D / 32, CB = D / 16;
    constexpr int ROWB = D * 2 + 16;
    constexpr int PROW = 64 * 2 + 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* k_hi = lds;
    unsigned char* k_lo = k_hi + 64 * ROWB;
    unsigned char* v_hi = k_lo + 64 * ROWB;
    unsigned char* v_lo = v_hi + 64 * ROWB;
    unsigned char* p_base = v_lo + 64 * ROWB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nqt = (T + 63) / 64;
    int bid = xcd_group_id(blockIdx.x, nqt, gridDim.x / nqt);  // the tiles of one (b, h) share an XCD's L2
    const int qt = bid % nqt; bid /= nqt;
    const int h = bid % H;
    const int b = bid / H;
    const int C3 = 3 * H * d, C1 = H * d;
    const float* base = qkv + (size_t)b * T * C3;
    const int q0 = qt * 64 + wave * 16;
    unsigned char* p_hi = p_base + wave * 2 * 16 * PROW;
    unsigned char* p_lo = p_hi + 16 * PROW;

    Frag qh[KS], ql[KS], gh[KS], gl[KS];
    {
        const int q = q0 + (lane & 15);
        load_row_frags<D, PAD>(base + h * d, C3, q, q < T, d, scale, qh, ql);
        load_row_frags<D, PAD>(d_o + (size_t)b * T * C1 + h * d, C1, q, q < T, d, 1.0f, gh, gl);
    }
    float lrow[4], drow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * (lane >> 4) + r;
        lrow[r] = (q < T) ? lse[((size_t)b * H + h) * T + q] : 0.f;
        drow[r] = (q < T) ? delta[((size_t)b * H + h) * T + q] : 0.f;
    }
    f32x4 dq[CB];
#pragma unroll
    for (int i = 0; i < CB; ++i) dq[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nkt = (T + 63) / 64;
    for (int kt = 0; kt < nkt; ++kt) {
        const int s0 = kt * 64;
        __syncthreads();
        stage_rows<D, PAD>(base + (H + h) * d, C3, s0, T, d, scale, k_hi, k_lo, ROWB);
        stage_rows<D, PAD>(base + (2 * H + h) * d, C3, s0, T, d, 1.0f, v_hi, v_lo, ROWB);
        __syncthreads();
        f32x4 s[4], dp[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            s[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int key = cb * 16 + (lane & 15);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                Frag bh, bl;
                const int off = key * ROWB + (ks * 4 + (lane >> 4)) * 16;
                bh.u = *reinterpret_cast<const uint4*>(k_hi + off);
                bl.u = *reinterpret_cast<const uint4*>(k_lo + off);
                s[cb] = mfma_x3(qh[ks].v, ql[ks].v, bh.v, bl.v, s[cb]);
                bh.u = *reinterpret_cast<const uint4*>(v_hi + off);
                bl.u = *reinterpret_cast<const uint4*>(v_lo + off);
                dp[cb] = mfma_x3(gh[ks].v, gl[ks].v, bh.v, bl.v, dp[cb]);
            }
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const bool valid = (s0 + cb * 16 + (lane & 15)) < T;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = valid ? __expf(s[cb][r] - lrow[r]) : 0.f;
                s[cb][r] = pv * (dp[cb][r] - drow[r]);  // dS
            }
        }
        acc_to_image(s, p_hi, p_lo, PROW);
        __syncthreads();
        // dQ += dS Ks : A = dS image (row = query), B[k = key][col = d] via transposed reads of the K image
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            Frag ah, al;
            const int poff = (lane & 15) * PROW + (ks * 4 + (lane >> 4)) * 16;
            ah.u = *reinterpret_cast<const uint4*>(p_hi + poff);
            al.u = *reinterpret_cast<const uint4*>(p_lo + poff);
            const int krow = ks * 32 + 8 * (lane >> 4) + ((lane >> 2) & 3);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                Frag bh, bl;
                const int off = krow * ROWB + (cb * 16 + 4 * (lane & 3)) * 2;
                bh.h[0] = tr_read(k_hi + off); bh.h[1] = tr_read(k_hi + off + 4 * ROWB);
                bl.h[0] = tr_read(k_lo + off); bl.h[1] = tr_read(k_lo + off + 4 * ROWB);
                dq[cb] = mfma_x3(ah.v, al.v, bh.v, bl.v, dq[cb]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * (lane >> 4) + r;
        if (q < T) {
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
                if (in_head<PAD>(cb * 16 + (lane & 15), d))
                    dqkv[((size_t)b * T + q) * C3 + h * d + cb * 16 + (lane & 15)] = dq[cb][r] * scale;
        }
    }
}

// ---- pass B: dK, dV --------------------------------------------------------------------------------------
// QB: queries per streamed tile, 64 or 32 (dkv_queries).  The 256-wide tile streams 32 (its Q / dO images of 64 rows would pass the LDS a
// workgroup may declare); the products accumulate over the queries in the same order either way.
template <int D, bool PAD>
__global__ __launch_bounds__(256, occupancy(D)) void attention_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                                              const float* __restrict__ lse, const float* __restrict__ delta,
                                                                              float* __restrict__ dqkv, int T, int H, float scale, int d_arg) {
    const int d = PAD ? d_arg : D;
    constexpr int QB = dkv_queries(D);
    constexpr int KS = D / 32, CB = D / 16, NQ = QB / 16;
    constexpr int ROWB = D * 2 + 16;
    constexpr int PROW = QB * 2 + 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* q_hi = lds;
    unsigned char* q_lo = q_hi + QB * ROWB;
    unsigned char* g_hi = q_lo + QB * ROWB;
    unsigned char* g_lo = g_hi + QB * ROWB;
    float* lq = reinterpret_cast<float*>(g_lo + QB * ROWB);  // [64] lse of the query tile
    float* dq_ = lq + 64;                                     // [64] delta of the query tile
    unsigned char* p_base = reinterpret_cast<unsigned char*>(dq_ + 64);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nkt = (T + 63) / 64;
    int bid = xcd_group_id(blockIdx.x, nkt, gridDim.x / nkt);  // the tiles of one (b, h) share an XCD's L2
    const int kt = bid % nkt; bid /= nkt;
    const int h = bid % H;
    const int b = bid / H;
    const int C3 = 3 * H * d, C1 = H * d;
    const float* base = qkv + (size_t)b * T * C3;
    const int k0 = kt * 64 + wave * 16;
    unsigned char* p_hi = p_base + wave * 4 * 16 * PROW;   // P^T image
    unsigned char* p_lo = p_hi + 16 * PROW;
    unsigned char* s_hi = p_lo + 16 * PROW;                // dS^T image
    unsigned char* s_lo = s_hi + 16 * PROW;

    Frag kh[KS], kl[KS], vh[KS], vl[KS];
    {
        const int key = k0 + (lane & 15);
        load_row_frags<D, PAD>(base + (H + h) * d, C3, key, key < T, d, scale, kh, kl);
        load_row_frags<D, PAD>(base + (2 * H + h) * d, C3, key, key < T, d, 1.0f, vh, vl);
    }
    f32x4 dk[CB], dv[CB];
#pragma unroll
    for (int i = 0; i < CB; ++i) { dk[i] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    const int nqt = (T + QB - 1) / QB;
    for (int qt = 0; qt < nqt; ++qt) {
        const int q0 = qt * QB;
        __syncthreads();
        stage_rows<D, PAD, QB>(base + h * d, C3, q0, T, d, scale, q_hi, q_lo, ROWB);
        stage_rows<D, PAD, QB>(d_o + (size_t)b * T * C1 + h * d, C1, q0, T, d, 1.0f, g_hi, g_lo, ROWB);
        if (tid < QB) {
            const bool ok = (q0 + tid) < T;
            lq[tid] = ok ? lse[((size_t)b * H + h) * T + q0 + tid] : 0.f;
            dq_[tid] = ok ? delta[((size_t)b * H + h) * T + q0 + tid] : 0.f;
        }
        __syncthreads();
        // S^T = Ks Qs^T,  dP^T = V dO^T   (16 keys x QB queries)
        f32x4 s[NQ], dp[NQ];
#pragma unroll
        for (int cb = 0; cb < NQ; ++cb) {
            s[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int qq = cb * 16 + (lane & 15);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                Frag bh, bl;
                const int off = qq * ROWB + (ks * 4 + (lane >> 4)) * 16;
                bh.u = *reinterpret_cast<const uint4*>(q_hi + off);
                bl.u = *reinterpret_cast<const uint4*>(q_lo + off);
                s[cb] = mfma_x3(kh[ks].v, kl[ks].v, bh.v, bl.v, s[cb]);
                bh.u = *reinterpret_cast<const uint4*>(g_hi + off);
                bl.u = *reinterpret_cast<const uint4*>(g_lo + off);
                dp[cb] = mfma_x3(vh[ks].v, vl[ks].v, bh.v, bl.v, dp[cb]);
            }
        }
        f32x4 ds[NQ];
#pragma unroll
        for (int cb = 0; cb < NQ; ++cb) {
            const int qq = cb * 16 + (lane & 15);
            const bool valid = (q0 + qq) < T;
            const float lv = lq[qq], dl = dq_[qq];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = valid ? __expf(s[cb][r] - lv) : 0.f;
                s[cb][r] = pv;
                ds[cb][r] = pv * (dp[cb][r] - dl);
            }
        }
        acc_to_image(s, p_hi, p_lo, PROW);
        acc_to_image(ds, s_hi, s_lo, PROW);
        __syncthreads();
        // dV += P^T dO,  dK += dS^T Qs : B[k = query][col = d] via transposed reads of the dO / Q images
#pragma unroll
        for (int ks = 0; ks < QB / 32; ++ks) {
            Frag ph, pl, sh_, sl_;
            const int poff = (lane & 15) * PROW + (ks * 4 + (lane >> 4)) * 16;
            ph.u = *reinterpret_cast<const uint4*>(p_hi + poff);
            pl.u = *reinterpret_cast<const uint4*>(p_lo + poff);
            sh_.u = *reinterpret_cast<const uint4*>(s_hi + poff);
            sl_.u = *reinterpret_cast<const uint4*>(s_lo + poff);
            const int qrow = ks * 32 + 8 * (lane >> 4) + ((lane >> 2) & 3);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                Frag bh, bl;
                const int off = qrow * ROWB + (cb * 16 + 4 * (lane & 3)) * 2;
                bh.h[0] = tr_read(g_hi + off); bh.h[1] = tr_read(g_hi + off + 4 * ROWB);
                bl.h[0] = tr_read(g_lo + off); bl.h[1] = tr_read(g_lo + off + 4 * ROWB);
                dv[cb] = mfma_x3(ph.v, pl.v, bh.v, bl.v, dv[cb]);
                bh.h[0] = tr_read(q_hi + off); bh.h[1] = tr_read(q_hi + off + 4 * ROWB);
                bl.h[0] = tr_read(q_lo + off); bl.h[1] = tr_read(q_lo + off + 4 * ROWB);
                dk[cb] = mfma_x3(sh_.v, sl_.v, bh.v, bl.v, dk[cb]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int key = k0 + 4 * (lane >> 4) + r;
        if (key < T) {
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                if (!in_head<PAD>(cb * 16 + (lane & 15), d)) continue;
                const size_t o = ((size_t)b * T + key) * C3 + cb * 16 + (lane & 15);
                dqkv[o + (H + h) * d] = dk[cb][r] * scale;
                dqkv[o + (2 * H + h) * d] = dv[cb][r];
            }
        }
    }
}

// ---- launchers: tile DT, head size d (= DT unless PAD) -----------------------------------------------------------------------
inline float head_scale(int d) { return (float)(1.0 / sqrt(sqrt((double)d))); }  // blocks.py:173 (python double, then fp32)

template <int DT, bool PAD>
int launch_fwd(const float* qkv, float* out, float* lse, void* workspace, int B, int T, int H, int d, hipStream_t stream) {
    const size_t sh = fwd_lds_bytes(DT);
    if (sh > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_kernel<DT, PAD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    const int nqt = (T + QT - 1) / QT, nkt = (T + KTILE - 1) / KTILE;
    const int wgs = B * H * nqt;
    const int ksplit = key_split(wgs, nkt, workspace);
    float* part = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL((attention_kernel<DT, PAD>), dim3(wgs * ksplit), dim3(256), sh, stream, qkv, out, lse, T, H, head_scale(d), ksplit, part, d);
    TQ_CHECK_LAUNCH();
    if (ksplit > 1) {
        const size_t n = (size_t)B * H * T * (DT / 4);
        hipLaunchKernelGGL((attn_combine_kernel<DT, PAD>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part, out, lse, T, H, ksplit, n, d);
        TQ_CHECK_LAUNCH();
    }
    return 0;
}

template <int DT, bool PAD>
int launch_bwd(const float* qkv, const float* out, const float* d_o, const float* lse, float* delta, float* dqkv, int B, int T,
               int H, int d, hipStream_t stream) {
    const size_t n = (size_t)B * T * H;
    hipLaunchKernelGGL(attn_delta_kernel<PAD>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out, d_o, delta, T, H, d, n);
    TQ_CHECK_LAUNCH();
    const int nt = (T + 63) / 64;
    const size_t shA = dq_lds_bytes(DT), shB = dkv_lds_bytes(DT, dkv_queries(DT));
    if (shA > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_bwd_dq_kernel<DT, PAD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shA);
    if (shB > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_bwd_dkv_kernel<DT, PAD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shB);
    hipLaunchKernelGGL((attention_bwd_dq_kernel<DT, PAD>), dim3(B * H * nt), dim3(256), shA, stream, qkv, d_o, lse, delta, dqkv, T, H, head_scale(d), d);
    TQ_CHECK_LAUNCH();
    hipLaunchKernelGGL((attention_bwd_dkv_kernel<DT, PAD>), dim3(B * H * nt), dim3(256), shB, stream, qkv, d_o, lse, delta, dqkv, T, H, head_scale(d), d);
    TQ_CHECK_LAUNCH();
    return 0;
}
}  // namespace
