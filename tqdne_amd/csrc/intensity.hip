// Ground-motion intensity measures (the reference's scripts/seismo_evaluations: gmrotdpp_withPG, parallel_processing_sa,
// process_kanno; smtk's semantics restated, not run): for N two-component waveforms the directional peaks
//     m[n, k, phi] = max_t | sx_k(t) cos phi + sy_k(t) sin phi |,   phi = 0 .. 179 degrees,
// of K = 3 + P series pairs -- ground acceleration a = x[:-1], velocity v and displacement d (cumulative trapezoids of a and of
// v) and the absolute-acceleration response of P damped oscillators (Nigam-Jennings: the oscillator equation solved exactly from
// sample to sample for an input that is linear in between) -- in ONE launch.  GMRotDpp / RotDpp are a sort over 90 / 180 of
// these values and stay in torch.
//
// Form: one LANE per (waveform, series), one workgroup (one wave) per 64 such pairs and per CHUNK of the angle axis.  A lane
// walks the time axis once, advancing its own series by the 2 x 2 recurrence and folding every new sample pair into the running
// maxima of its chunk's angles, which live in registers.  The series itself never exists in memory (no scratch in HBM, no LDS),
// there is no reduction across lanes (no atomics, no shuffles) and every sum has one order that depends on (T, P) alone: two
// launches agree bit for bit and a waveform's result does not depend on the rest of the batch.  The recurrence is recomputed by
// every angle chunk of a pair: 20 fused multiply-adds per sample next to 4 instructions per angle.  Chunks of 6 angles (30 workgroups per 64
// pairs) while K <= 32 -- the reference's own 4 periods at 192 waveforms are 1344 pairs, 21 waves, and fill 630 -- and chunks of
// 30 angles (6 per 64 pairs) beyond, where the pairs alone fill the chip and the recomputation would be the larger part.  The
// choice looks at K only, never at N.  The direction cosines of a chunk are wave-uniform: they are read from the table with a
// uniform index into scalar registers before the time loop and enter the vector instructions as scalar operands.
//
// Oscillator state: (w^2 u, w u'), so that the step matrix and the input weights are O(1) in fp32 for every period (the classic
// arrangement with 2 xi / (w^3 dt) cancels).  tq_oscillator_tables computes them on the host in double.  The ground series keep
// float64 accumulators (as the envelope kernel does): v and d are sums of thousands of terms with a mean.
//
// Non-finite input: v_max drops a NaN operand, so the maxima cannot carry one.  Every lane sees every sample of its waveform's
// two components and folds x * 0 into a carrier that is added to each result: +0 for finite input, NaN otherwise.
#include <cmath>

#include "common.hpp"
#include "../../include/tqdne_hip.h"

namespace {

constexpr int N_ANGLES = 180;
constexpr int TAB_COS = 0, TAB_SIN = N_ANGLES, TAB_OSC = 2 * N_ANGLES, OSC_FLOATS = 12;
constexpr int LANES = 64;
constexpr int PREFETCH = 8;          // samples loaded ahead of the recurrence, per component
constexpr int CHUNK_FEW = 6, CHUNK_MANY = 30, FEW_SERIES = 32;
static_assert(N_ANGLES % CHUNK_FEW == 0 && N_ANGLES % CHUNK_MANY == 0, "chunks tile the angle axis");

// sx c + sy s with BOTH products rounded (no fused multiply-add): the two terms are then treated alike, so that a pair of equal
// components gives exactly 0 at 135 degrees, where c = -s, and not the rounding residue of one product -- GMRotD takes the square
// root of that value times the peak at 45 degrees, which would lift 2^-25 of the peak to 1.7e-4 of it.
__device__ __forceinline__ float rotated(float sx, float c, float sy, float s) {
#pragma clang fp contract(off)
    return sx * c + sy * s;
}

// m = max(m, |t|) in ONE instruction.  fmaxf(m, fabsf(t)) costs two: m arrives through the loop, the compiler cannot see that it is
// no signalling NaN and quiets it first (v_max m, m, m).  Both operands are results of arithmetic here, and a NaN among them is
// carried by the separate carrier, not by m.
__device__ __forceinline__ void fold_abs_max(float& m, float t) {
    asm("v_max_f32_e64 %0, %0, |%1|" : "+v"(m) : "v"(t));
}

template <int CHUNK>
__global__ __launch_bounds__(LANES) void rotd_peaks_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ tables, float* __restrict__ peaks, int N, int T,
                                                           int P, double dt) {
    const long long n_ground = 3ll * N, n_pairs = n_ground + (long long)N * P;
    const long long j = (long long)blockIdx.x * LANES + threadIdx.x;
    if (j >= n_pairs) return;
    const int a0 = blockIdx.y * CHUNK;
    // pairs 0 .. 3N-1 are the ground series, the oscillators follow: a wave is of one kind except at the boundary
    const bool ground = j < n_ground;
    const int n = ground ? (int)(j / 3) : (int)((j - n_ground) / P);
    const int k = ground ? (int)(j % 3) : 3 + (int)((j - n_ground) % P);
    const float* xs = x + (size_t)n * T;
    const float* ys = y + (size_t)n * T;

    float cs[CHUNK], sn[CHUNK], m[CHUNK];
#pragma unroll
    for (int i = 0; i < CHUNK; ++i) {
        cs[i] = tables[TAB_COS + a0 + i];   // uniform address: a scalar load
        sn[i] = tables[TAB_SIN + a0 + i];
        m[i] = 0.f;
    }
    const float* co = tables + TAB_OSC + (size_t)(ground ? 0 : k - 3) * OSC_FLOATS;
    float a11 = 0.f, a12 = 0.f, a21 = 0.f, a22 = 0.f, b0p = 0.f, b0q = 0.f, b1p = 0.f, b1q = 0.f, two_xi = 0.f;
    if (!ground) {
        a11 = co[0]; a12 = co[1]; a21 = co[2]; a22 = co[3];
        b0p = co[4]; b0q = co[5]; b1p = co[6]; b1q = co[7];
        two_xi = co[8];
    }

    const int L = T - 1;                       // samples of every series
    float px = 0.f, qx = 0.f, py = 0.f, qy = 0.f;   // oscillator state of the two components
    double vx = 0.0, dx = 0.0, vy = 0.0, dy = 0.0;  // ground velocity and displacement
    const double hdt = 0.5 * dt;
    float poison = 0.f;

    float nx[PREFETCH], ny[PREFETCH];
#pragma unroll
    for (int u = 0; u < PREFETCH; ++u) {       // samples 1 .. PREFETCH (index clamped to the last sample: never past the row)
        const int t = min(1 + u, L);
        nx[u] = xs[t];
        ny[u] = ys[t];
    }
    float x0 = xs[0], y0 = ys[0];
    poison = fmaf(x0, 0.f, poison);
    poison = fmaf(y0, 0.f, poison);

    for (int t0 = 0; t0 < L; t0 += PREFETCH) {
        float cx[PREFETCH], cy[PREFETCH];
#pragma unroll
        for (int u = 0; u < PREFETCH; ++u) {
            cx[u] = nx[u];
            cy[u] = ny[u];
            const int t = min(t0 + PREFETCH + 1 + u, L);
            nx[u] = xs[t];
            ny[u] = ys[t];
        }
#pragma unroll
        for (int u = 0; u < PREFETCH; ++u) {
            if (t0 + u < L) {                  // uniform: L is the launch's
                const float x1 = cx[u], y1 = cy[u];   // samples t0 + u + 1; x0, y0 are samples t0 + u
                poison = fmaf(x1, 0.f, poison);
                poison = fmaf(y1, 0.f, poison);
                float sx, sy;
                if (ground) {
                    // series sample t0 + u: a, v, d at that time (v and d are 0 at sample 0)
                    sx = k == 0 ? x0 : k == 1 ? (float)vx : (float)dx;
                    sy = k == 0 ? y0 : k == 1 ? (float)vy : (float)dy;
                    const double wx = vx + hdt * ((double)x0 + (double)x1), wy = vy + hdt * ((double)y0 + (double)y1);
                    dx += hdt * (vx + wx);
                    dy += hdt * (vy + wy);
                    vx = wx;
                    vy = wy;
                } else {
                    const float p1 = fmaf(b1p, x1, fmaf(b0p, x0, fmaf(a12, qx, a11 * px)));
                    const float q1 = fmaf(b1q, x1, fmaf(b0q, x0, fmaf(a22, qx, a21 * px)));
                    const float p2 = fmaf(b1p, y1, fmaf(b0p, y0, fmaf(a12, qy, a11 * py)));
                    const float q2 = fmaf(b1q, y1, fmaf(b0q, y0, fmaf(a22, qy, a21 * py)));
                    px = p1; qx = q1; py = p2; qy = q2;
                    sx = -fmaf(two_xi, qx, px);
                    sy = -fmaf(two_xi, qy, py);
                }
#pragma unroll
                for (int i = 0; i < CHUNK; ++i) fold_abs_max(m[i], rotated(sx, cs[i], sy, sn[i]));
                x0 = x1;
                y0 = y1;
            }
        }
    }
    float* o = peaks + ((size_t)n * (3 + P) + k) * N_ANGLES + a0;
#pragma unroll
    for (int i = 0; i < CHUNK; ++i) o[i] = m[i] + poison;
}

bool periods_ok(const double* periods, int P) {
    for (int i = 0; i < P; ++i)
        if (!(periods[i] > 0.0) || !std::isfinite(periods[i])) return false;
    return true;
}

}  // namespace

extern "C" size_t tq_oscillator_table_floats(int P) {
    return P < 0 ? 0 : (size_t)TAB_OSC + (size_t)P * OSC_FLOATS;
}

extern "C" int tq_oscillator_tables(const double* periods, int P, double dt, double damping, float* host_out) {
    if (!host_out || P < 0 || (P > 0 && !periods)) return TQ_ERR_ARG;
    if (!(dt > 0.0) || !std::isfinite(dt) || !(damping >= 0.0 && damping < 1.0) || !periods_ok(periods, P)) return TQ_ERR_ARG;
    const double pi = 3.14159265358979323846264338327950288;
    for (int i = 0; i < N_ANGLES; ++i) {   // 0 and 90 degrees leave the components exactly as they are
        host_out[TAB_COS + i] = i == 90 ? 0.f : (float)cos(pi * i / 180.0);
        host_out[TAB_SIN + i] = (float)sin(pi * i / 180.0);
    }
    for (int i = 0; i < P; ++i) {
        // state s = (w^2 u, w u'):  s' = w J s + (0, -w) a,  J = [[0, 1], [-1, -2 xi]];  one step of length h with a linear between
        // its ends:  s(h) = A s(0) + B0 a(0) + B1 a(h),  A = exp(w J h),  g = (w J)^-1 (A - I) (0, -w),
        // B1 = (w J)^-1 (g - h (0, -w)) / h,  B0 = g - B1;  J^-1 = [[-2 xi, -1], [1, 0]]
        const double w = 2.0 * pi / periods[i], xi = damping, r = sqrt(1.0 - xi * xi), wh = w * dt;
        const double e = exp(-xi * wh), c = cos(r * wh), s = sin(r * wh);
        const double A11 = e * (c + xi / r * s), A12 = e * s / r, A21 = -A12, A22 = e * (c - xi / r * s);
        const double g0 = 2.0 * xi * A12 + (A22 - 1.0), g1 = -A12;
        const double B1p = (-2.0 * xi * g0 - (g1 + wh)) / wh, B1q = g0 / wh;
        float* o = host_out + TAB_OSC + (size_t)i * OSC_FLOATS;
        o[0] = (float)A11; o[1] = (float)A12; o[2] = (float)A21; o[3] = (float)A22;
        o[4] = (float)(g0 - B1p); o[5] = (float)(g1 - B1q); o[6] = (float)B1p; o[7] = (float)B1q;
        o[8] = (float)(2.0 * xi);
        o[9] = o[10] = o[11] = 0.f;
    }
    return 0;
}

extern "C" int tq_rotd_peaks(const float* x, const float* y, const float* tables, float* peaks, int N, int T, int P, double dt,
                             hipStream_t stream) {
    if (!x || !y || !tables || !peaks || P < 0) return TQ_ERR_ARG;
    if (!(dt > 0.0) || !std::isfinite(dt)) return TQ_ERR_ARG;
    if (N <= 0 || T < 2) return TQ_ERR_SHAPE;
    const long long n_pairs = (long long)N * (3 + (long long)P);
    const long long blocks = (n_pairs + LANES - 1) / LANES;
    if (blocks > 0x7fffffffll) return TQ_ERR_SHAPE;
    if (3 + (long long)P <= FEW_SERIES)
        hipLaunchKernelGGL(rotd_peaks_kernel<CHUNK_FEW>, dim3((unsigned)blocks, N_ANGLES / CHUNK_FEW), dim3(LANES), 0, stream, x, y,
                           tables, peaks, N, T, P, dt);
    else
        hipLaunchKernelGGL(rotd_peaks_kernel<CHUNK_MANY>, dim3((unsigned)blocks, N_ANGLES / CHUNK_MANY), dim3(LANES), 0, stream, x, y,
                           tables, peaks, N, T, P, dt);
    TQ_CHECK_LAUNCH();
    return 0;
}
