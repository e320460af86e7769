// Parameter-free resampling of the reference's conv_resample=False models (blocks.py:29-108 with use_conv=False) on gfx950:
//   Downsample = avg_pool1d(kernel 2, stride 2), Upsample = nearest x2 with no conv behind it.
// Every activation a GroupNorm reads must arrive with its per-slot partial statistics {sum, sum of squares}; the conv epilogues and the
// stem emit them for their outputs, and these streaming kernels do the same for theirs.  A workgroup owns whole (sample, 128-position
// output slot) rows of the statistics: per-thread register sums, one fixed-order pass over LDS, plain stores -- no atomics, so two
// launches on the same input leave the same bits.  16 bytes per lane, lanes contiguous along C; grids capped, grid-stride loops.
#include "common.hpp"
#include "../../include/tqdne_hip.h"

using namespace tq;

namespace {
constexpr int RP_NT = 256;
constexpr unsigned RP_MAX_WGS = 2048;
constexpr int RP_MAX_C = 1024;   // c4n = C / 4 <= RP_NT: one thread per 4-channel column of a row

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 avg2(const float4 a, const float4 c) {
    // (x[2t] + x[2t+1]) * 0.5f in this association: the bits of avg_pool1d for finite inputs
    return make_float4((a.x + c.x) * 0.5f, (a.y + c.y) * 0.5f, (a.z + c.z) * 0.5f, (a.w + c.w) * 0.5f);
}
__device__ __forceinline__ void acc_stats(float4& s, float4& q, const float4 o) {
    s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
    q.x = fmaf(o.x, o.x, q.x); q.y = fmaf(o.y, o.y, q.y); q.z = fmaf(o.z, o.z, q.z); q.w = fmaf(o.w, o.w, q.w);
}

// One workgroup per (b, output slot) unit, grid-stride over the units.  Thread = (row r of nrow = 256 / c4n, column c4): it walks the
// slot's rows r, r + nrow, ...; the nrow partial sums of a column meet in LDS and thread (0, c4) adds them in row order.
// UP = false: y (B, T_out = T_in / 2, C) = pair averages of x.   UP = true: y (B, T_out = 2 T_in, C) = every row of x twice -- a slot of
// 128 output rows is 64 input rows, each counted twice (the doubling of both sums is exact).
template <bool UP>
__global__ __launch_bounds__(RP_NT) void resample_stats_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                float* __restrict__ stats, int T_in, int T_out, int C, int nslots,
                                                                int nunits) {
    __shared__ float4 red[2][RP_NT];
    const int c4n = C >> 2;
    const int nrow = RP_NT / c4n;
    const int tid = threadIdx.x;
    const int row = tid / c4n, c4 = tid - row * c4n;
    const bool active = row < nrow;
    for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
        const int b = u / nslots, sl = u - b * nslots;
        const int t0 = sl * STAT_SLOT;
        const int t1 = min(t0 + STAT_SLOT, T_out);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (active) {
            if (!UP) {
#pragma unroll 4
                for (int t = t0 + row; t < t1; t += nrow) {
                    const float* px = x + ((size_t)b * T_in + 2 * (size_t)t) * C + 4 * c4;
                    const float4 o = avg2(ld4(px), ld4(px + C));
                    st4(y + ((size_t)b * T_out + t) * C + 4 * c4, o);
                    acc_stats(s, q, o);
                }
            } else {
#pragma unroll 4
                for (int ti = (t0 >> 1) + row; ti < (t1 >> 1); ti += nrow) {
                    const float4 o = ld4(x + ((size_t)b * T_in + ti) * C + 4 * c4);
                    float* py = y + ((size_t)b * T_out + 2 * (size_t)ti) * C + 4 * c4;
                    st4(py, o);
                    st4(py + C, o);
                    acc_stats(s, q, o);
                }
            }
        }
        red[0][tid] = s;
        red[1][tid] = q;
        __syncthreads();
        if (tid < c4n) {
            for (int r = 1; r < nrow; ++r) {
                const float4 sr = red[0][r * c4n + tid], qr = red[1][r * c4n + tid];
                s.x += sr.x; s.y += sr.y; s.z += sr.z; s.w += sr.w;
                q.x += qr.x; q.y += qr.y; q.z += qr.z; q.w += qr.w;
            }
            if (UP) {
                s.x *= 2.0f; s.y *= 2.0f; s.z *= 2.0f; s.w *= 2.0f;
                q.x *= 2.0f; q.y *= 2.0f; q.z *= 2.0f; q.w *= 2.0f;
            }
            float* ps = stats + ((size_t)u * C + 4 * tid) * 2;   // (B, nslots, C, 2): {sum, sum of squares} per channel
            st4(ps, make_float4(s.x, q.x, s.y, q.y));
            st4(ps + 4, make_float4(s.z, q.z, s.w, q.w));
        }
        __syncthreads();   // (the next unit overwrites red)
    }
}

// The statistics-free forms: flat element-wise kernels (the access pattern of tq_pair_sum / tq_zero_stuff).
__global__ __launch_bounds__(RP_NT) void avg_pool2_kernel(const float* __restrict__ x, float* __restrict__ y, int T_in, int T_out, int C,
                                                           size_t n4) {
    const int c4n = C >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const size_t bt = i / c4n;
        const int t = (int)(bt % T_out);
        const size_t b = bt / T_out;
        const float* px = x + (b * T_in + 2 * (size_t)t) * C + 4 * c4;
        st4(y + 4 * i, avg2(ld4(px), ld4(px + C)));
    }
}

__global__ __launch_bounds__(RP_NT) void nearest_up2_kernel(const float* __restrict__ x, float* __restrict__ y, int T_in, int C, size_t n4) {
    const int c4n = C >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const size_t bt = i / c4n;   // b * T_in + t: output rows 2 bt and 2 bt + 1
        const float4 o = ld4(x + 4 * i);
        float* py = y + (2 * bt) * C + 4 * c4;
        st4(py, o);
        st4(py + C, o);
    }
}

// dx[b, 2t, :], dx[b, 2t + 1, :] (+)= 0.5f * dy[b, t, :]; the dropped last row of an odd T_in gets zero (nothing when accumulating)
__global__ __launch_bounds__(RP_NT) void avg_pool2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int T_in, int T_out,
                                                               int C, int accum, size_t n4) {
    const int c4n = C >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const size_t bu = i / c4n;
        const int t = (int)(bu % T_in) >> 1;
        const size_t b = bu / T_in;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < T_out) {
            const float4 g = ld4(dy + (b * T_out + t) * C + 4 * c4);
            o = make_float4(0.5f * g.x, 0.5f * g.y, 0.5f * g.z, 0.5f * g.w);
        } else if (accum) {
            continue;
        }
        if (accum) { const float4 ov = ld4(dx + 4 * i); o.x += ov.x; o.y += ov.y; o.z += ov.z; o.w += ov.w; }
        st4(dx + 4 * i, o);
    }
}

inline unsigned rp_grid(size_t n) {
    const size_t g = (n + RP_NT - 1) / RP_NT;
    return (unsigned)(g > RP_MAX_WGS ? RP_MAX_WGS : (g ? g : 1));
}

inline int rp_check(const void* a, const void* b, int B, int T_in, int C) {
    if (!a || !b) return TQ_ERR_ARG;
    if (B <= 0 || T_in < 2 || C <= 0 || C % 4 || C > RP_MAX_C) return TQ_ERR_SHAPE;
    return 0;
}
}  // namespace

extern "C" int tq_avg_pool2_fwd(const float* x, float* y, float* stats, int B, int T_in, int C, hipStream_t stream) {
    if (const int rc = rp_check(x, y, B, T_in, C)) return rc;
    const int T_out = T_in / 2;
    if (stats) {
        const int nslots = (T_out + STAT_SLOT - 1) / STAT_SLOT;
        const int nunits = B * nslots;
        hipLaunchKernelGGL(resample_stats_kernel<false>, dim3(nunits > (int)RP_MAX_WGS ? RP_MAX_WGS : nunits), dim3(RP_NT), 0, stream, x, y,
                           stats, T_in, T_out, C, nslots, nunits);
    } else {
        const size_t n4 = (size_t)B * T_out * (C / 4);
        hipLaunchKernelGGL(avg_pool2_kernel, dim3(rp_grid(n4)), dim3(RP_NT), 0, stream, x, y, T_in, T_out, C, n4);
    }
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tq_nearest_up2_fwd(const float* x, float* y, float* stats, int B, int T_in, int C, hipStream_t stream) {
    if (const int rc = rp_check(x, y, B, T_in, C)) return rc;
    const int T_out = 2 * T_in;
    if (stats) {
        const int nslots = (T_out + STAT_SLOT - 1) / STAT_SLOT;
        const int nunits = B * nslots;
        hipLaunchKernelGGL(resample_stats_kernel<true>, dim3(nunits > (int)RP_MAX_WGS ? RP_MAX_WGS : nunits), dim3(RP_NT), 0, stream, x, y,
                           stats, T_in, T_out, C, nslots, nunits);
    } else {
        const size_t n4 = (size_t)B * T_in * (C / 4);
        hipLaunchKernelGGL(nearest_up2_kernel, dim3(rp_grid(n4)), dim3(RP_NT), 0, stream, x, y, T_in, C, n4);
    }
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tq_avg_pool2_bwd(const float* dy, float* dx, int B, int T_in, int C, int accumulate, hipStream_t stream) {
    if (const int rc = rp_check(dy, dx, B, T_in, C)) return rc;
    const size_t n4 = (size_t)B * T_in * (C / 4);
    hipLaunchKernelGGL(avg_pool2_bwd_kernel, dim3(rp_grid(n4)), dim3(RP_NT), 0, stream, dy, dx, T_in, T_in / 2, C, accumulate, n4);
    TQ_CHECK_LAUNCH();
    return 0;
}
