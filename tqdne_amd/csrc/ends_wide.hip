// Stem and head convolutions at every first-level width 32 | C <= 1024.
//
// The kernels of small_ops.hip (stem_conv_kernel, head_conv_kernel, head_conv_row_kernel) and backward.hip (head_bwd_kernel,
// head_bwd_stream_kernel) hold the whole channel extent in one workgroup's LDS and need it to divide 256 threads: they take widths of
// 32, 64, 128 (and, for some, 256 ... 1024 at small signal-channel counts).  The kernels here TILE the channel axis instead and are
// reached only for the shapes those launchers used to refuse -- a shape that worked before runs the kernel, grid and bits it always did.
//   stem forward   independent per output channel: grid (b x 128-position slot, 128-channel tile); a tile of 32 / 64 / 96 channels
//                  leaves the threads beyond nrow * tile / 4 idle.  The statistics layout (B, ceil(T / 128), C_out, 2) is unchanged.
//   head forward   a reduction over C_in: the row-per-lane / quarter-per-wave scheme of head_conv_row_kernel walking C_in in chunks of
//                  <= 128 channels inside the workgroup (stage, barrier, accumulate KT x C_out sums in registers, barrier, next chunk).
//                  The input is read once plus the halo; fp32 FMA; no atomics; <= 44 KB of LDS.
//   head backward  independent per input channel apart from db: head_bwd_stream_kernel's thread-per-channel scheme with a grid
//                  dimension over 128-channel chunks; every chunk stages its own copy of the small dF tile, chunk 0 owns db.  dw / db
//                  leave as one partial row per workgroup (plain stores) summed by a second launch when a workspace is given -- the
//                  number of workgroups per chunk is bounded so that the rows fit -- and as atomics otherwise.
// All arithmetic is exact fp32 FMA, as in the kernels these stand next to.
#include "common.hpp"
#include "ends_wide.hpp"
#include "../../include/tqdne_hip.h"

using namespace tq;

namespace {
constexpr int CH = 128;   // channels per tile / chunk

__host__ __device__ inline bool wide_width(int C) { return C >= 32 && C <= 1024 && C % 32 == 0; }
__host__ __device__ inline bool wide_taps(int k) { return k == 1 || k == 3 || k == 5; }

// =================================================================================================
// Stem: (B, C_in <= 16, T) NCW -> conv k "same" -> (B, T, C_out) channels-last, + bias, + partial statistics.
// Workgroup = (b, 128-position slot, tile of ct <= 128 output channels); thread = (4 output channels, rows tr, tr + nrow, ...).
// =================================================================================================
template <int KT>
__global__ __launch_bounds__(256) void stem_wide_kernel(const float* __restrict__ x, const float* __restrict__ in_scale,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, float* __restrict__ stats, int C_in, int T,
                                                        int C_out, int nslots, int xs_floats) {
    extern __shared__ __attribute__((aligned(16))) float shm[];
    constexpr int PAD = KT / 2;
    constexpr int TW = STAT_SLOT + KT - 1;
    const int c0 = blockIdx.y * CH;
    const int ct = min(CH, C_out - c0);     // this tile's channels: 32, 64, 96 or 128
    float* xs = shm;                        // [C_in][TW]  (xs_floats: rounded up to 16 bytes)
    float* ws = xs + xs_floats;             // [KT][C_in][ct]
    float* red = ws + KT * C_in * ct;       // [nrow][ct][2]   (nrow * ct <= 1024)
    const int slot = blockIdx.x % nslots;
    const int b = blockIdx.x / nslots;
    const int t0 = slot * STAT_SLOT;
    const float sc = in_scale ? in_scale[b] : 1.0f;
    for (int i = threadIdx.x; i < C_in * TW; i += 256) {
        const int c = i / TW, j = i % TW;
        const int t = t0 - PAD + j;
        xs[i] = (t >= 0 && t < T) ? x[((size_t)b * C_in + c) * T + t] * sc : 0.f;
    }
    for (int i = threadIdx.x; i < KT * C_in * ct; i += 256) {
        const int co = i % ct, r = i / ct;
        const int ci = r % C_in, k = r / C_in;
        ws[i] = w[((size_t)(c0 + co) * C_in + ci) * KT + k];
    }
    __syncthreads();
    const int ngrp = ct >> 2;               // groups of 4 output channels: 8, 16, 24 or 32
    const int nrow = 256 / ngrp;            // positions per pass; threads tr >= nrow idle (ngrp = 24: 240 of 256 work)
    const int cg = threadIdx.x % ngrp;
    const int tr = threadIdx.x / ngrp;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias) bv = *reinterpret_cast<const float4*>(bias + c0 + 4 * cg);
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const int nkc = KT * C_in;
    float* yb = y + (size_t)b * T * C_out + c0 + 4 * cg;
    if (tr < nrow && nkc <= 16) {
        // the usual 3-channel stem: the thread's weights in registers, see stem_conv_kernel
        float4 wr[16];
        int xoff[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ii = i < nkc ? i : 0;
            wr[i] = *reinterpret_cast<const float4*>(ws + ii * ct + 4 * cg);
            if (i >= nkc) wr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int k = ii / C_in, ci = ii % C_in;   // ws is [k][ci][co]
            xoff[i] = ci * TW + k;
        }
        for (int tl = tr; tl < STAT_SLOT; tl += nrow) {
            const int t = t0 + tl;
            if (t >= T) break;
            float4 a = bv;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i < nkc) {   // (uniform)
                    const float xv = xs[xoff[i] + tl];
                    a.x = fmaf(wr[i].x, xv, a.x); a.y = fmaf(wr[i].y, xv, a.y);
                    a.z = fmaf(wr[i].z, xv, a.z); a.w = fmaf(wr[i].w, xv, a.w);
                }
            }
            *reinterpret_cast<float4*>(yb + (size_t)t * C_out) = a;
            s1[0] += a.x; s1[1] += a.y; s1[2] += a.z; s1[3] += a.w;
            s2[0] += a.x * a.x; s2[1] += a.y * a.y; s2[2] += a.z * a.z; s2[3] += a.w * a.w;
        }
    } else if (tr < nrow) {
        for (int tl = tr; tl < STAT_SLOT; tl += nrow) {
            const int t = t0 + tl;
            if (t >= T) break;
            float4 a = bv;
            for (int k = 0; k < KT; ++k)
                for (int ci = 0; ci < C_in; ++ci) {
                    const float xv = xs[ci * TW + tl + k];
                    const float4 wv = *reinterpret_cast<const float4*>(ws + (k * C_in + ci) * ct + 4 * cg);
                    a.x = fmaf(wv.x, xv, a.x); a.y = fmaf(wv.y, xv, a.y);
                    a.z = fmaf(wv.z, xv, a.z); a.w = fmaf(wv.w, xv, a.w);
                }
            *reinterpret_cast<float4*>(yb + (size_t)t * C_out) = a;
            s1[0] += a.x; s1[1] += a.y; s1[2] += a.z; s1[3] += a.w;
            s2[0] += a.x * a.x; s2[1] += a.y * a.y; s2[2] += a.z * a.z; s2[3] += a.w * a.w;
        }
    }
    if (stats) {
        if (tr < nrow) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                red[(tr * ct + 4 * cg + j) * 2] = s1[j];
                red[(tr * ct + 4 * cg + j) * 2 + 1] = s2[j];
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < ct; c += 256) {
            float a1 = 0.f, a2 = 0.f;
            for (int r = 0; r < nrow; ++r) { a1 += red[(r * ct + c) * 2]; a2 += red[(r * ct + c) * 2 + 1]; }
            float* st = stats + (((size_t)b * nslots + slot) * C_out + c0 + c) * 2;
            st[0] = a1; st[1] = a2;
        }
    }
}

// =================================================================================================
// Head forward: GroupNorm + SiLU (folded) -> conv k "same" to <= 8 of the head's C_tot output channels -> NCW, with the skip epilogue.
// head_conv_row_kernel with a chunk loop: a workgroup owns 64 consecutive input rows of one sample and, per chunk of ch <= 128 channels,
//   1. stages the rows' chunk, activated, in LDS ([row][CH + 4]); a thread owns one 4-channel column (for ch = 96 the 24 columns take
//      10 rows per pass and threads 240 ... 255 idle);
//   2. wave w takes the chunk's channels [w ch / 4, (w + 1) ch / 4), lane = row: the KT x NCO weights of a channel are wave-uniform
//      scalar loads feeding the FMAs; the partial sums stay in registers across the chunks;
// then the four waves' sums meet in LDS (in the tile's place), where the tap shift is an address offset.
// =================================================================================================
template <int KT, int NCO>
__global__ __launch_bounds__(256) void head_wide_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gscale,
                                                            const float* __restrict__ gshift, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ c_out,
                                                            const float* __restrict__ c_skip, const float* __restrict__ skip_src,
                                                            float* __restrict__ y, int T, int C_in, int ntiles, int co0, int nco,
                                                            int C_tot) {
    constexpr int PAD = KT / 2, NOUT = 64 - (KT - 1), NP = KT * NCO, RS = CH + 4;
    static_assert(NCO >= 1 && NCO <= 8, "a wave emits at most two output channels");
    extern __shared__ __attribute__((aligned(16))) float shm[];
    float* tile = shm;                          // [64][RS]
    float* part = shm;                          // [4][NP][68]: takes the tile's place once every wave is done reading it
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x / ntiles, t0 = (blockIdx.x % ntiles) * NOUT;
    // the epilogue's skip-connection operand: requested now, used after the last barrier
    const int to = t0 + lane;
    const bool emit_t = lane < NOUT && to < T;
    size_t oo[2];
    float skipv[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int co = wave + 4 * h;
        oo[h] = ((size_t)b * C_tot + co0 + (co < nco ? co : 0)) * T + (to < T ? to : 0);
        if (c_out && emit_t && co < nco) skipv[h] = skip_src[oo[h]];
    }
    float acc[KT][NCO];
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int co = 0; co < NCO; ++co) acc[k][co] = 0.f;
    for (int c0 = 0; c0 < C_in; c0 += CH) {
        const int ch = min(CH, C_in - c0);      // 32, 64, 96 or 128
        if (c0) __syncthreads();                // (the previous chunk's readers are done with the tile)
        // ---- 1. stage
        {
            const int ncol = ch >> 2, rpp = 256 / ncol;   // 4-channel columns, rows per pass
            const int c4 = threadIdx.x % ncol, r0 = threadIdx.x / ncol;
            if (r0 < rpp) {
                float4 a4 = make_float4(1.f, 1.f, 1.f, 1.f), s4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gscale) {
                    a4 = *reinterpret_cast<const float4*>(gscale + (size_t)b * C_in + c0 + 4 * c4);
                    s4 = *reinterpret_cast<const float4*>(gshift + (size_t)b * C_in + c0 + 4 * c4);
                }
                const float* xb = x + (size_t)b * T * C_in + c0 + 4 * c4;
                for (int r = r0; r < 64; r += rpp) {
                    const int t = t0 - PAD + r;
                    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);   // zero padding of the ACTIVATED input
                    if (t >= 0 && t < T) {
                        u = *reinterpret_cast<const float4*>(xb + (size_t)t * C_in);
                        if (gscale) {
                            u.x = silu_f(fmaf(a4.x, u.x, s4.x)); u.y = silu_f(fmaf(a4.y, u.y, s4.y));
                            u.z = silu_f(fmaf(a4.z, u.z, s4.z)); u.w = silu_f(fmaf(a4.w, u.w, s4.w));
                        }
                    }
                    *reinterpret_cast<float4*>(tile + r * RS + 4 * c4) = u;
                }
            }
        }
        __syncthreads();
        // ---- 2. lane = row, wave = quarter of the chunk
        const int cq = ch >> 2;                 // 8, 16, 24 or 32 channels
        const float* ur = tile + lane * RS + wave * cq;
        const float* wc[NCO];   // per output channel: this wave's (cq, KT) weight block (channels past nco repeat the last one; never emitted)
#pragma unroll
        for (int co = 0; co < NCO; ++co) wc[co] = w + ((size_t)(co0 + (co < nco ? co : nco - 1)) * C_in + c0 + wave * cq) * KT;
        // (one 4-channel step per trip, not unrolled: see head_conv_row_kernel)
#pragma unroll 1
        for (int c4 = 0; c4 < (cq >> 2); ++c4) {
            const float4 v4 = *reinterpret_cast<const float4*>(ur + 4 * c4);
            const float u[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int co = 0; co < NCO; ++co) {
                const float* wr = wc[co] + 4 * c4 * KT;   // wave-uniform: scalar loads
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int k = 0; k < KT; ++k) acc[k][co] = fmaf(wr[e * KT + k], u[e], acc[k][co]);
            }
        }
    }
    // ---- 3. partial sums -> LDS, tap shift = address offset
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int co = 0; co < NCO; ++co) {
            float* pr = part + ((wave * NP) + k * NCO + co) * 68;
            pr[lane] = acc[k][co];
            if (lane < 4) pr[64 + lane] = 0.f;   // (read by the outputs the workgroup does not emit)
        }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < (NCO > 4 ? 2 : 1); ++h) {
        const int co = wave + 4 * h;
        if (emit_t && co < NCO && co < nco) {
            float v = bias ? bias[co0 + co] : 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k)
#pragma unroll
                for (int wv = 0; wv < 4; ++wv) v += part[((wv * NP) + k * NCO + co) * 68 + lane + k];
            if (c_out) v = v * c_out[b] + c_skip[b] * skipv[h];
            y[oo[h]] = v;
        }
    }
}

// =================================================================================================
// Head backward.  dF = c_out[b] * dpred (B, C_out, T).  Workgroup = (run of (b, slot) units, chunk of ch <= 128 input channels);
// thread = (input channel of the chunk, position segment), as in head_bwd_stream_kernel:
//   dW[co][ci][k] += sum_t dF[co][t] z[ci][t+k-pad];   db[co] += sum_t dF[co][t]   (chunk 0 only)
//   G[t][ci] = (sum_{co,k} W[co][ci][k] dF[co][t+pad-k]) * silu'(a h + s),  GN partial sums {sum G, sum G h} per 128-position slot
// nseg = 8 / 4 / 2 / 2 position segments for ch = 32 / 64 / 96 / 128 (ch = 96: threads 192 ... 255 idle).
// =================================================================================================
template <int KT, int MAXCO>
__global__ __launch_bounds__(256) void head_wide_bwd_kernel(const float* __restrict__ dpred, const float* __restrict__ c_out,
                                                            const float* __restrict__ h, const float* __restrict__ gscale,
                                                            const float* __restrict__ gshift, const float* __restrict__ w,
                                                            float* __restrict__ G, float* __restrict__ gstats,
                                                            float* __restrict__ dw, float* __restrict__ db, float* __restrict__ part,
                                                            int T, int C_in, int C_out, int nslots, int nunits, int upw) {
    extern __shared__ float shm[];
    constexpr int PAD = KT / 2, TW = STAT_SLOT + 2 * PAD, BLK = 8;
    constexpr int GRP = MAXCO < 8 ? MAXCO : 8;   // output channels per pass of the final reduction (bounds its LDS)
    float* dfs = shm;                          // [MAXCO][TW]  dF of positions t0 - pad .. t0 + 127 + pad
    float* red = dfs + MAXCO * TW;             // [nseg][max(2, GRP * KT)][ch]
    const int c0 = blockIdx.y * CH;
    const int ch = min(CH, C_in - c0);
    const int nseg = ch <= 32 ? 8 : ch <= 64 ? 4 : 2;
    const int L = STAT_SLOT / nseg;
    const bool active = (int)threadIdx.x < nseg * ch;
    const int ci = threadIdx.x % ch, seg = active ? (int)threadIdx.x / ch : 0;
    const int cg = c0 + ci;                    // the thread's channel of the whole input
    const size_t nout = (size_t)C_out * C_in * KT;   // a partial row: dw, then db padded to MAXCO
    float wr[MAXCO][KT], aw[MAXCO][KT];
#pragma unroll
    for (int co = 0; co < MAXCO; ++co)
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            wr[co][k] = co < C_out ? w[((size_t)co * C_in + cg) * KT + k] : 0.f;
            aw[co][k] = 0.f;
        }
    float dbs = 0.f;   // thread co < C_out of chunk 0 sums dF[co] over the slots' own positions
    const int u0 = blockIdx.x * upw, u1 = min(nunits, u0 + upw);
    for (int u = u0; u < u1; ++u) {
        const int slot = u % nslots, b = u / nslots;
        const int t0 = slot * STAT_SLOT;
        const float cs = c_out ? c_out[b] : 1.0f;
        __syncthreads();
        for (int i = threadIdx.x; i < C_out * TW; i += 256) {
            const int c = i / TW, j = i % TW;
            const int t = t0 - PAD + j;
            dfs[c * TW + j] = (t >= 0 && t < T) ? dpred[((size_t)b * C_out + c) * T + t] * cs : 0.f;
        }
        for (int i = C_out * TW + threadIdx.x; i < MAXCO * TW; i += 256) dfs[i] = 0.f;   // (unused output channels)
        __syncthreads();
        if (blockIdx.y == 0 && (int)threadIdx.x < C_out) {
            const int nv = min(STAT_SLOT, T - t0);
            for (int j = 0; j < nv; ++j) dbs += dfs[threadIdx.x * TW + PAD + j];
        }
        float s1 = 0.f, s2 = 0.f;
        if (active) {
            float ga = 1.f, gs = 0.f;
            if (gscale) { ga = gscale[(size_t)b * C_in + cg]; gs = gshift[(size_t)b * C_in + cg]; }
            const int tb = t0 + seg * L;
            const size_t rowb = ((size_t)b * T + tb) * C_in + cg;
            for (int tl = 0; tl < L; tl += BLK) {
                float hv[BLK];
#pragma unroll
                for (int j = 0; j < BLK; ++j) {   // (branch-free clamped loads, see stem_wgrad_stream_kernel)
                    const int tj = tb + tl + j;
                    const int tc = tj < T ? tj : T - 1;
                    hv[j] = h[((size_t)b * T + tc) * C_in + cg];
                }
                float g[BLK], z[BLK], ds[BLK];
#pragma unroll
                for (int j = 0; j < BLK; ++j) {
                    g[j] = 0.f;
                    if (gscale) { const float uu = ga * hv[j] + gs; z[j] = silu_f(uu); ds[j] = dsilu_f(uu); }
                    else { z[j] = hv[j]; ds[j] = 1.f; }
                    if (tb + tl + j >= T) z[j] = 0.f;   // (positions past the signal contribute nothing)
                }
#pragma unroll
                for (int co = 0; co < MAXCO; ++co) {
                    // window: dF[co] at slot-relative positions (seg L + tl) - pad .. + BLK - 1 + pad  ->  dfs index + PAD
                    float q[BLK + 2 * PAD];
#pragma unroll
                    for (int j = 0; j < BLK + 2 * PAD; ++j) q[j] = dfs[co * TW + seg * L + tl + j];   // (wave-uniform unless ch = 96)
#pragma unroll
                    for (int j = 0; j < BLK; ++j)
#pragma unroll
                        for (int k = 0; k < KT; ++k) {
                            const float f = q[j + 2 * PAD - k];   // dF[co][t + pad - k]
                            aw[co][k] = fmaf(z[j], f, aw[co][k]);
                            g[j] = fmaf(wr[co][k], f, g[j]);
                        }
                }
#pragma unroll
                for (int j = 0; j < BLK; ++j) {
                    if (tb + tl + j < T) {
                        const float gv = g[j] * ds[j];
                        G[rowb + (size_t)(tl + j) * C_in] = gv;
                        s1 += gv; s2 += gv * hv[j];
                    }
                }
            }
        }
        if (gstats) {   // the slot's partial sums: combine the position segments through LDS
            __syncthreads();
            if (active) {
                red[(seg * 2 + 0) * ch + ci] = s1;
                red[(seg * 2 + 1) * ch + ci] = s2;
            }
            __syncthreads();
            if (active && seg == 0) {
                float a1 = 0.f, a2 = 0.f;
                for (int sg = 0; sg < nseg; ++sg) { a1 += red[(sg * 2 + 0) * ch + ci]; a2 += red[(sg * 2 + 1) * ch + ci]; }
                float* st = gstats + (((size_t)b * nslots + slot) * C_in + cg) * 2;
                st[0] = a1; st[1] = a2;
            }
        }
    }
#pragma unroll
    for (int g0 = 0; g0 < MAXCO; g0 += GRP) {
        __syncthreads();
        if (active) {
#pragma unroll
            for (int co = 0; co < GRP; ++co)
#pragma unroll
                for (int k = 0; k < KT; ++k) red[(seg * GRP * KT + co * KT + k) * ch + ci] = aw[g0 + co][k];
        }
        __syncthreads();
        const int ngc = min(GRP, C_out - g0);   // valid output channels of this pass (<= 0: none)
        for (int o = threadIdx.x; o < ngc * KT * ch; o += 256) {
            const int c = o % ch, ck = o / ch;   // ck = (co - g0) * KT + k
            float v = 0.f;
            for (int sg = 0; sg < nseg; ++sg) v += red[(sg * GRP * KT + ck) * ch + c];
            const int co = g0 + ck / KT, k = ck % KT;
            const size_t oi = ((size_t)co * C_in + c0 + c) * KT + k;
            // `part` given: this workgroup's sums go to its own row of the scratch (plain stores), rows_sum_kernel adds the rows
            // (same-line atomics from every workgroup serialise: see stem_wgrad_stream_kernel)
            if (part) part[(size_t)blockIdx.x * (nout + MAXCO) + oi] = v;
            else atomicAdd(dw + oi, v);
        }
    }
    if (blockIdx.y == 0 && (int)threadIdx.x < C_out) {
        if (part) part[(size_t)blockIdx.x * (nout + MAXCO) + nout + threadIdx.x] = dbs;
        else atomicAdd(db + threadIdx.x, dbs);
    }
}

// out[i] += sum_r part[r][i]   (i < n; rows `stride` floats apart)
__global__ __launch_bounds__(256) void rows_sum_kernel(const float* __restrict__ part, int nrows, size_t stride, int n,
                                                       float* __restrict__ out) {
    __shared__ float red2[4][64];
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    float a = 0.f;
    if (i < n)
        for (int r = q; r < nrows; r += 4) a += part[(size_t)r * stride + i];
    red2[q][threadIdx.x & 63] = a;
    __syncthreads();
    if (q == 0 && i < n) out[i] += (red2[0][threadIdx.x] + red2[1][threadIdx.x]) + (red2[2][threadIdx.x] + red2[3][threadIdx.x]);   // (threadIdx.x < 64 here)
}

inline int round4(int n) { return (n + 3) & ~3; }
}  // namespace

// ------------------------------------------------------------------------------------------------- limits
size_t tq::ends_wide_stem_lds(int C_in, int C_out, int ktaps) {
    if (C_in < 1 || C_in > 16 || !wide_width(C_out) || !wide_taps(ktaps)) return 0;
    const int ct = C_out < CH ? C_out : CH;
    return ((size_t)round4(C_in * (STAT_SLOT + ktaps - 1)) + (size_t)ktaps * C_in * ct + 2048) * sizeof(float);   // <= 57 KB
}

size_t tq::ends_wide_head_fwd_lds(int C_in, int C_out, int ktaps) {
    if (!wide_width(C_in) || C_out < 1 || C_out > 16 || !wide_taps(ktaps)) return 0;
    const int per = C_out <= 8 ? C_out : 8;
    const int nco = per == 5 ? 6 : per == 7 ? 8 : per;   // the kernel's NCO
    const size_t st_ = (size_t)64 * (CH + 4), sp_ = (size_t)4 * ktaps * nco * 68;
    return (st_ > sp_ ? st_ : sp_) * sizeof(float);      // <= 44 KB (the partial sums reuse the staged tile's space)
}

size_t tq::ends_wide_head_bwd_lds(int C_in, int C_out, int ktaps) {
    if (!wide_width(C_in) || C_out < 1 || C_out > 16 || !wide_taps(ktaps)) return 0;
    const int mco = C_out <= 4 ? 4 : C_out <= 8 ? 8 : 16, grp = mco < 8 ? mco : 8;
    const int per = grp * ktaps > 2 ? grp * ktaps : 2;
    return ((size_t)mco * (STAT_SLOT + ktaps - 1) + (size_t)256 * per) * sizeof(float);   // <= 49 KB
}

// ------------------------------------------------------------------------------------------------- launchers
int tq::ends_wide_stem_fwd(const float* x, const float* in_scale, const float* w, const float* bias, float* y, float* stats, int B,
                           int C_in, int T, int C_out, int ktaps, hipStream_t stream) {
    if (!x || !w || !y) return TQ_ERR_ARG;
    const size_t sh = ends_wide_stem_lds(C_in, C_out, ktaps);
    if (B <= 0 || T <= 0 || sh == 0) return TQ_ERR_SHAPE;
    const int nslots = (T + STAT_SLOT - 1) / STAT_SLOT;
    const dim3 grid((unsigned)(B * nslots), (unsigned)((C_out + CH - 1) / CH));
    const int xsf = round4(C_in * (STAT_SLOT + ktaps - 1));
#define TQ_STEMW(K) hipLaunchKernelGGL(stem_wide_kernel<K>, grid, dim3(256), sh, stream, x, in_scale, w, bias, y, stats, C_in, T, C_out, nslots, xsf)
    if (ktaps == 5) TQ_STEMW(5);
    else if (ktaps == 3) TQ_STEMW(3);
    else TQ_STEMW(1);
#undef TQ_STEMW
    TQ_CHECK_LAUNCH();
    return 0;
}

int tq::ends_wide_head_fwd(const float* x, const float* gscale, const float* gshift, const float* w, const float* bias,
                           const float* c_out, const float* c_skip, const float* skip_src, float* y, int B, int T, int C_in, int C_out,
                           int ktaps, hipStream_t stream) {
    if (!x || !w || !y) return TQ_ERR_ARG;
    if ((gscale == nullptr) != (gshift == nullptr)) return TQ_ERR_ARG;
    if (c_out && (!c_skip || !skip_src)) return TQ_ERR_ARG;
    const size_t sh = ends_wide_head_fwd_lds(C_in, C_out, ktaps);
    if (B <= 0 || T <= 0 || sh == 0) return TQ_ERR_SHAPE;
    const int nt = (T + (64 - (ktaps - 1)) - 1) / (64 - (ktaps - 1));
    // output channels per launch: <= 8 (9 ... 16 = two launches: the input is staged twice)
#define TQ_HEADW(K, N, CO0, NC) hipLaunchKernelGGL((head_wide_fwd_kernel<K, N>), dim3((unsigned)(B * nt)), dim3(256), sh, stream, x, gscale, gshift, \
                                                   w, bias, c_out, c_skip, skip_src, y, T, C_in, nt, CO0, NC, C_out)
#define TQ_HEADWK(K) { for (int c0 = 0; c0 < C_out; c0 += 8) { const int nc = C_out - c0 < 8 ? C_out - c0 : 8; \
                         if (nc == 1) TQ_HEADW(K, 1, c0, nc); else if (nc == 2) TQ_HEADW(K, 2, c0, nc); else if (nc == 3) TQ_HEADW(K, 3, c0, nc); \
                         else if (nc == 4) TQ_HEADW(K, 4, c0, nc); else if (nc <= 6) TQ_HEADW(K, 6, c0, nc); else TQ_HEADW(K, 8, c0, nc); } }
    if (ktaps == 5) TQ_HEADWK(5)
    else if (ktaps == 3) TQ_HEADWK(3)
    else TQ_HEADWK(1)
#undef TQ_HEADWK
#undef TQ_HEADW
    TQ_CHECK_LAUNCH();
    return 0;
}

int tq::ends_wide_head_bwd(const float* dpred_nct, const float* c_out, const float* x, const float* gscale, const float* gshift,
                           const float* w, float* g_out, float* gstats, float* dw, float* db, int B, int T, int C_in, int C_out,
                           int ktaps, void* workspace, size_t ws_bytes, hipStream_t stream) {
    if (!dpred_nct || !x || !w || !g_out || !dw || !db) return TQ_ERR_ARG;
    if ((gscale == nullptr) != (gshift == nullptr)) return TQ_ERR_ARG;
    const size_t sh = ends_wide_head_bwd_lds(C_in, C_out, ktaps);
    if (B <= 0 || T <= 0 || sh == 0) return TQ_ERR_SHAPE;
    const int mco = C_out <= 4 ? 4 : C_out <= 8 ? 8 : 16;
    const int nslots = (T + STAT_SLOT - 1) / STAT_SLOT;
    const int nchunks = (C_in + CH - 1) / CH;
    const int nunits = B * nslots;
    // about 512 workgroups in all (the count head_bwd_stream_kernel was tuned to); with a workspace no more per chunk than partial rows fit
    int nwg = 512 / nchunks;
    if (nwg > nunits) nwg = nunits;
    const size_t row = (size_t)C_out * C_in * ktaps + mco;
    float* part = nullptr;
    if (workspace && ws_bytes >= row * sizeof(float)) {
        const size_t fit = ws_bytes / (row * sizeof(float));
        if ((size_t)nwg > fit) nwg = (int)fit;
        part = reinterpret_cast<float*>(workspace);
    }
    const int upw = (nunits + nwg - 1) / nwg;
    const unsigned gx = (unsigned)((nunits + upw - 1) / upw);
    const dim3 grid(gx, (unsigned)nchunks);
#define TQ_HBW(K, M) hipLaunchKernelGGL((head_wide_bwd_kernel<K, M>), grid, dim3(256), sh, stream, dpred_nct, c_out, x, gscale, gshift, w, g_out, \
                                        gstats, dw, db, part, T, C_in, C_out, nslots, nunits, upw)
#define TQ_HBWK(K) { if (mco == 4) TQ_HBW(K, 4); else if (mco == 8) TQ_HBW(K, 8); else TQ_HBW(K, 16); }
    if (ktaps == 5) TQ_HBWK(5)
    else if (ktaps == 3) TQ_HBWK(3)
    else TQ_HBWK(1)
#undef TQ_HBWK
#undef TQ_HBW
    TQ_CHECK_LAUNCH();
    if (part) {
        const int n = (int)(row - mco);
        hipLaunchKernelGGL(rows_sum_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, stream, part, (int)gx, row, n, dw);
        TQ_CHECK_LAUNCH();
        hipLaunchKernelGGL(rows_sum_kernel, dim3(1), dim3(256), 0, stream, part + n, (int)gx, row, C_out, db);
        TQ_CHECK_LAUNCH();
    }
    return 0;
}
