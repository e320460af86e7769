// Time-domain conditioning of waveform batches (include/tqdne_series.h): a causal second-order-section IIR cascade after an optional
// detrend, and the reference's hold-and-recompute envelope.
//
// Both recurrences are sequential in time and independent between rows, so ONE LANE owns ONE ROW from its first sample to its last
// (the form of tq_rotd_peaks): the state lives in registers, there is no LDS and no atomic, and nothing a lane reads or writes belongs
// to another row.  A lane walks its row twice: the first walk looks for a non-finite sample and forms the detrend's fp64 sums in
// sample order, the second one runs the recurrence.  Samples move in chunks of CHUNK per lane: a chunk's loads are issued together, one
// chunk ahead of its use; they come before the stores of their own chunk and are disjoint from the stores of the previous one, which
// is what makes y == x safe.  A chunk inside the row is loaded and stored without a branch, which lets the compiler move 16 bytes per
// instruction.
//
// Lanes of a wave read different rows, so every load and store touches one cache line per lane, and a wave's time is set by the
// latency of that traffic and by its fp64 chain (five FMAs per section and sample, two of them -- y, then z1 -- on the sample-to-
// sample dependence), not by how many lanes it carries.  A workgroup is therefore a quarter wave of 16 rows: the 576 rows of a
// validation batch become 36 waves on 36 compute units instead of 9 on 9.  (A batch of tens of thousands of rows would be served
// better by full waves; the reference's batches are hundreds of rows.)
//
// No fast-math functions; every product-sum of the recurrences is an explicit fma, so the result does not depend on the compiler's
// contraction setting.
#include <cfloat>
#include <cmath>

#include "../csrc/common.hpp"
#include "../../include/tqdne_series.h"

namespace {

constexpr int THREADS = 16;   // rows per workgroup: a quarter wave (see above)
constexpr int CHUNK = 16;
constexpr int MAX_SECTIONS = TQS_SOSFILT_MAX_SECTIONS;
constexpr int MAX_T = 1 << 30;   // the sample index, one chunk past the end included, stays an int

__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= FLT_MAX); }

// v[k] = p[t - back] for the times t = t0 + k of a chunk with back <= t < T, zero at the others.  A chunk that lies inside [back, T) --
// all but the first and last of a row -- takes the branch-free loads.
__device__ __forceinline__ void load_chunk(float (&v)[CHUNK], const float* p, int t0, int back, int T) {
    if (t0 >= back && t0 + CHUNK <= T) {
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) v[k] = p[t0 + k - back];
    } else {
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) v[k] = (t0 + k >= back && t0 + k < T) ? p[t0 + k - back] : 0.f;
    }
}

__device__ __forceinline__ void store_chunk(float* p, const float (&v)[CHUNK], int t0, int T) {
    if (t0 + CHUNK <= T) {
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) p[t0 + k] = v[k];
    } else {
#pragma unroll
        for (int k = 0; k < CHUNK; ++k)
            if (t0 + k < T) p[t0 + k] = v[k];
    }
}

template <int NS>
__global__ __launch_bounds__(THREADS) void sosfilt_kernel(const float* x, float* y, const double* __restrict__ sos, int R, int T,
                                                          long long ldx, long long ldy, int detrend) {
    const long long row = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (row >= R) return;
    const float* xr = x + row * ldx;
    float* yr = y + row * ldy;

    // first walk: the non-finite flag and the sums of the least-squares line over the centred time axis
    const double tbar = 0.5 * (double)(T - 1);
    double s0 = 0.0, s1 = 0.0;
    bool bad = false;
    for (int t0 = 0; t0 < T; t0 += CHUNK) {
        float v[CHUNK];
        load_chunk(v, xr, t0, 0, T);
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) {   // (a padded sample adds an exact zero to both sums)
            bad |= not_finite(v[k]);
            s0 += (double)v[k];
            s1 = fma((double)(t0 + k) - tbar, (double)v[k], s1);
        }
    }
    double mean = 0.0, slope = 0.0;
    if (detrend != TQS_DETREND_NONE) mean = s0 / (double)T;
    if (detrend == TQS_DETREND_LINEAR && T > 1) {
        const double n = (double)T;
        slope = s1 / (n * (n * n - 1.0) / 12.0);   // sum (t - tbar)^2 = T (T^2 - 1) / 12, exact in double for T < 2^17
    }

    double b0[NS], b1[NS], b2[NS], a1[NS], a2[NS], z1[NS], z2[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        b0[j] = sos[6 * j];
        b1[j] = sos[6 * j + 1];
        b2[j] = sos[6 * j + 2];
        a1[j] = sos[6 * j + 4];
        a2[j] = sos[6 * j + 5];
        z1[j] = 0.0;
        z2[j] = 0.0;
    }
    const float nan = __builtin_nanf("");
    float v[CHUNK], next[CHUNK];
    load_chunk(v, xr, 0, 0, T);
    for (int t0 = 0; t0 < T; t0 += CHUNK) {
        load_chunk(next, xr, t0 + CHUNK, 0, T);   // in flight under this chunk's chain; ahead of, and disjoint from, this chunk's stores
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) {
            double u = (double)v[k];
            if (detrend != TQS_DETREND_NONE) u = fma(-slope, (double)(t0 + k) - tbar, u - mean);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const double w = fma(b0[j], u, z1[j]);
                z1[j] = fma(-a1[j], w, fma(b1[j], u, z2[j]));
                z2[j] = fma(-a2[j], w, b2[j] * u);
                u = w;
            }
            v[k] = bad ? nan : (float)u;
        }
        store_chunk(yr, v, t0, T);
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) v[k] = next[k];
    }
}

__global__ __launch_bounds__(THREADS) void hold_envelope_kernel(const float* __restrict__ x, float* __restrict__ env, int R, int T,
                                                                long long ldx, long long ldy, int window, float jump,
                                                                float add_eps) {
    const long long row = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (row >= R) return;
    const float* xr = x + row * ldx;
    float* er = env + row * ldy;

    bool bad = false;
    for (int t0 = 0; t0 < T; t0 += CHUNK) {
        float v[CHUNK];
        load_chunk(v, xr, t0, 0, T);
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) bad |= not_finite(v[k]);
    }

    const float nan = __builtin_nanf("");
    const double eps = (double)add_eps;
    double sum = 0.0, out = 0.0;
    float prev = 0.f;
    // old: the samples that leave the window, x[t - window] at the times t >= window
    float v[CHUNK], old[CHUNK], next[CHUNK], next_old[CHUNK];
    load_chunk(v, xr, 0, 0, T);
    load_chunk(old, xr, 0, window, T);
    for (int t0 = 0; t0 < T; t0 += CHUNK) {
        load_chunk(next, xr, t0 + CHUNK, 0, T);
        load_chunk(next_old, xr, t0 + CHUNK, window, T);
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) {
            const int t = t0 + k;
            const float a = fabsf(v[k]);
            sum = (sum + (double)a) - (double)fabsf(old[k]);
            if (t == 0) {
                out = (double)a;
            } else if (a > __fmul_rn(jump, prev)) {   // the decision in fp32: product, rounded, then the compare
                out = sum / (double)(t + 1 < window ? t + 1 : window);
            }
            prev = a;
            v[k] = bad ? nan : (float)(out + eps);
        }
        store_chunk(er, v, t0, T);
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) {
            v[k] = next[k];
            old[k] = next_old[k];
        }
    }
}

template <int NS>
void launch_sosfilt(const float* x, float* y, const double* sos, int R, int T, long long ldx, long long ldy, int detrend,
                    hipStream_t s) {
    const unsigned blocks = (unsigned)(((long long)R + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(sosfilt_kernel<NS>, dim3(blocks), dim3(THREADS), 0, s, x, y, sos, R, T, ldx, ldy, detrend);
}

}  // namespace

extern "C" int tqs_abi_version(void) { return TQS_ABI_VERSION; }

extern "C" int tqs_sosfilt_max_sections(void) { return MAX_SECTIONS; }

extern "C" int tqs_sosfilt(const float* x, float* y, const double* sos, int R, int T, int64_t ldx, int64_t ldy, int n_sections,
                           int detrend, hipStream_t s) {
    if (!x || !y || !sos) return TQ_ERR_ARG;
    if (detrend != TQS_DETREND_NONE && detrend != TQS_DETREND_DEMEAN && detrend != TQS_DETREND_LINEAR) return TQ_ERR_ARG;
    if (R < 1 || T < 1 || T > MAX_T || ldx < T || ldy < T || n_sections < 1 || n_sections > MAX_SECTIONS) return TQ_ERR_SHAPE;
    switch (n_sections) {
        case 1: launch_sosfilt<1>(x, y, sos, R, T, ldx, ldy, detrend, s); break;
        case 2: launch_sosfilt<2>(x, y, sos, R, T, ldx, ldy, detrend, s); break;
        case 3: launch_sosfilt<3>(x, y, sos, R, T, ldx, ldy, detrend, s); break;
        case 4: launch_sosfilt<4>(x, y, sos, R, T, ldx, ldy, detrend, s); break;
        case 5: launch_sosfilt<5>(x, y, sos, R, T, ldx, ldy, detrend, s); break;
        case 6: launch_sosfilt<6>(x, y, sos, R, T, ldx, ldy, detrend, s); break;
        case 7: launch_sosfilt<7>(x, y, sos, R, T, ldx, ldy, detrend, s); break;
        default: launch_sosfilt<8>(x, y, sos, R, T, ldx, ldy, detrend, s); break;
    }
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tqs_hold_envelope(const float* x, float* env, int R, int T, int64_t ldx, int64_t ldy, int window, float jump,
                                 float add_eps, hipStream_t s) {
    if (!x || !env || env == x) return TQ_ERR_ARG;
    if (!(fabsf(jump) <= FLT_MAX) || !(fabsf(add_eps) <= FLT_MAX)) return TQ_ERR_ARG;
    if (R < 1 || T < 1 || T > MAX_T || ldx < T || ldy < T || window < 1) return TQ_ERR_SHAPE;
    const unsigned blocks = (unsigned)(((long long)R + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(hold_envelope_kernel, dim3(blocks), dim3(THREADS), 0, s, x, env, R, T, (long long)ldx, (long long)ldy, window,
                       jump, add_eps);
    TQ_CHECK_LAUNCH();
    return 0;
}
