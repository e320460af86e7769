// Arias energy, Husid curve and threshold crossings of waveform rows, and numpy's gradient (include/tqdne_duration.h).
//
// tqd_arias: a row needs one running sum and a few comparisons, but the thresholds are fractions of the total, so the row is walked
// twice.  ONE WAVE owns ONE ROW.  With C = ceil(T / 64), lane l owns the samples l C ... (l + 1) C - 1 and the trapezoid terms that end
// at them (the term of sample i joins s[i-1] and s[i]; sample 0 has none).  First walk: the lane adds its terms in sample order from
// zero (its chunk sum), keeps the largest s and looks for a non-finite sample.  The 64 chunk sums become bases by a serial exclusive sum
// in lane order, base[l+1] = base[l] + chunk[l]: 64 dependent adds once per row, the same on every lane.  Second walk, same order:
// cum[i] = base[l] + (partial sum from the chunk's start), so the value at a chunk's last sample is bit for bit the next lane's base,
// the sequence is non-decreasing, and energy = base[64] is cum[T-1] itself.  Each lane keeps the first index of its chunk that reaches
// each threshold; one wave-wide minimum per threshold gives the crossing.  Lanes whose chunk is empty (T < 64, or the tail) add exact
// zeros.  No LDS, no atomics; the order of every sum depends on T only.
//
// A lane reads its chunk as 16-byte groups where the chunk's address allows it (the usual case: T and the row stride multiples of 4),
// else sample by sample.  Lanes of a wave read addresses C samples apart, so a load instruction touches one cache line per lane: the
// wave's time is set by the texture path, not by arithmetic.  A workgroup is therefore one wave, which spreads the few hundred rows of
// an evaluation batch over as many compute units instead of stacking four rows on each.
//
// Every add and multiply of the sums is __dadd_rn / __dmul_rn / fma, so the compiler's contraction setting cannot change a result.
#include <cfloat>
#include <climits>
#include <cmath>

#include "../csrc/common.hpp"
#include "../../include/tqdne_duration.h"

namespace {

constexpr int WAVE = 64;
constexpr int GROUP = 4;          // samples per 16-byte load
constexpr int MAX_F = TQD_MAX_FRACTIONS;
constexpr int MAX_T = 1 << 30;    // 64 chunks of at most 2^24 samples: every sample index stays an int
constexpr int GRAD_THREADS = 256;

struct Fractions {
    double f[MAX_F];
};

__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= FLT_MAX); }

// v[k] = p[i + k] for i + k < end, zero past it; one 16-byte load where the chunk is aligned and the group lies inside it
__device__ __forceinline__ void load_group(float (&v)[GROUP], const float* p, int i, int end, bool vec) {
    if (vec && i + GROUP <= end) {
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < GROUP; ++k) v[k] = (i + k < end) ? p[i + k] : 0.f;
    }
}

__device__ __forceinline__ void store_group(float* p, const float (&v)[GROUP], int i, int end, bool vec) {
    if (vec && i + GROUP <= end) {
        *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < GROUP; ++k)
            if (i + k < end) p[i + k] = v[k];
    }
}

template <bool TWO>
__device__ __forceinline__ double square_sum(float a, float b) {
    const double xx = (double)a * (double)a;   // exact: 48 bits
    return TWO ? fma((double)b, (double)b, xx) : xx;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

template <bool TWO, bool HUSID>
__global__ __launch_bounds__(WAVE) void arias_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                     double* __restrict__ energy, double* __restrict__ peak2,
                                                     int* __restrict__ index, float* __restrict__ husid, int T, long long ldx,
                                                     long long ldy, double half_step, Fractions fr, int F) {
    const long long row = blockIdx.x;
    const int lane = threadIdx.x;
    const float* xr = x + row * ldx;
    const float* yr = TWO ? y + row * ldy : xr;
    const int C = (T + WAVE - 1) / WAVE;
    const int i0 = lane * C < T ? lane * C : T;         // (63 * 2^24 fits)
    const int end = i0 + C < T ? i0 + C : T;            // empty chunk: i0 == end
    const bool vx = aligned16(xr + i0), vy = aligned16(yr + i0);

    // the sample before the chunk: the left end of the chunk's first term
    double before = 0.0;
    if (i0 > 0 && i0 < end) before = square_sum<TWO>(xr[i0 - 1], TWO ? yr[i0 - 1] : 0.f);

    // first walk: chunk sum in sample order, largest s, non-finite flag
    double chunk = 0.0, top = 0.0, prev = before;
    bool bad = false;
    for (int i = i0; i < end; i += GROUP) {
        float a[GROUP], b[GROUP];
        load_group(a, xr, i, end, vx);
        if (TWO) load_group(b, yr, i, end, vy);
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            if (i + k < end) {
                bad |= not_finite(a[k]) || (TWO && not_finite(b[k]));
                const double s = square_sum<TWO>(a[k], TWO ? b[k] : 0.f);
                if (i + k > 0) chunk = __dadd_rn(chunk, __dmul_rn(__dadd_rn(prev, s), half_step));
                top = s > top ? s : top;
                prev = s;
            }
        }
    }
    bad = __any(bad);
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const double o = __shfl_xor(top, d);
        top = o > top ? o : top;
    }

    // bases: the serial exclusive sum of the chunk sums in lane order (every lane runs the same 64 adds)
    double base = 0.0, run = 0.0;
    for (int l = 0; l < WAVE; ++l) {
        const double c = __shfl(chunk, l);
        if (lane == l) base = run;
        run = __dadd_rn(run, c);
    }
    const double total = run;               // cum[T-1]
    const bool dead = bad || !(total > 0.0);   // no crossing is defined, the Husid row is NaN
    const double nan = __builtin_nan("");
    if (lane == 0) {
        energy[row] = bad ? nan : total;
        peak2[row] = bad ? nan : top;
    }
    int* irow = index + row * (long long)F;
    if (dead) {
        if (lane < F) irow[lane] = -1;
        if (!HUSID) return;
    }

    // second walk, the same order: cum[i] = base + partial
    double thr[MAX_F];
    int first[MAX_F];
#pragma unroll
    for (int j = 0; j < MAX_F; ++j) {
        thr[j] = __dmul_rn(fr.f[j], total);
        first[j] = INT_MAX;
    }
    float* hr = HUSID ? husid + row * (long long)T : nullptr;
    const bool vh = HUSID && aligned16(hr + i0);
    const float nanf = __builtin_nanf("");
    double partial = 0.0;
    prev = before;
    for (int i = i0; i < end; i += GROUP) {
        float a[GROUP], b[GROUP], h[GROUP];
        load_group(a, xr, i, end, vx);
        if (TWO) load_group(b, yr, i, end, vy);
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            h[k] = nanf;
            if (i + k < end) {
                const double s = square_sum<TWO>(a[k], TWO ? b[k] : 0.f);
                if (i + k > 0) partial = __dadd_rn(partial, __dmul_rn(__dadd_rn(prev, s), half_step));
                prev = s;
                const double cum = __dadd_rn(base, partial);
#pragma unroll
                for (int j = 0; j < MAX_F; ++j)
                    if (j < F && cum >= thr[j] && first[j] == INT_MAX) first[j] = i + k;
                if (HUSID && !dead) h[k] = (float)__ddiv_rn(cum, total);
            }
        }
        if (HUSID) store_group(hr, h, i, end, vh);
    }
    if (dead) return;
#pragma unroll
    for (int j = 0; j < MAX_F; ++j) {
        if (j < F) {
            int m = first[j];
#pragma unroll
            for (int d = WAVE / 2; d > 0; d >>= 1) {
                const int o = __shfl_xor(m, d);
                m = o < m ? o : m;
            }
            if (lane == 0) irow[j] = m == INT_MAX ? -1 : m;
        }
    }
}

__global__ __launch_bounds__(GRAD_THREADS) void gradient_kernel(const float* __restrict__ x, float* __restrict__ g, int R, int T,
                                                                long long ldx, long long ldg, float dt, float two_dt) {
    const long long i = (long long)blockIdx.x * GRAD_THREADS + threadIdx.x;
    if (i >= T) return;
    const int lo = i == 0 ? 0 : (int)i - 1, hi = i == T - 1 ? (int)i : (int)i + 1;
    const float den = (i == 0 || i == T - 1) ? dt : two_dt;
    for (long long row = blockIdx.y; row < R; row += gridDim.y) {
        const float* xr = x + row * ldx;
        g[row * ldg + i] = __fdiv_rn(__fsub_rn(xr[hi], xr[lo]), den);
    }
}

template <bool TWO, bool HUSID>
void launch_arias(const float* x, const float* y, double* energy, double* peak2, int* index, float* husid, int R, int T, long long ldx,
                  long long ldy, double half_step, const Fractions& fr, int F, hipStream_t s) {
    hipLaunchKernelGGL((arias_kernel<TWO, HUSID>), dim3((unsigned)R), dim3(WAVE), 0, s, x, y, energy, peak2, index, husid, T, ldx, ldy,
                       half_step, fr, F);
}

// [p, p + ((R - 1) ld + T) floats) of two row sets intersect
bool overlap(const float* a, long long lda, const float* b, long long ldb, int R, int T) {
    const unsigned long long a0 = (unsigned long long)a, b0 = (unsigned long long)b;
    const unsigned long long a1 = a0 + 4ull * ((unsigned long long)(R - 1) * (unsigned long long)lda + (unsigned long long)T);
    const unsigned long long b1 = b0 + 4ull * ((unsigned long long)(R - 1) * (unsigned long long)ldb + (unsigned long long)T);
    return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int tqd_abi_version(void) { return TQD_ABI_VERSION; }

extern "C" int tqd_max_fractions(void) { return MAX_F; }

extern "C" int tqd_arias(const float* x, const float* y, double* energy, double* peak2, int32_t* index, float* husid, int R, int T,
                         int64_t ldx, int64_t ldy, double step, const double* fractions, int n_fractions, hipStream_t s) {
    if (!x || !energy || !peak2 || !index || !fractions) return TQ_ERR_ARG;
    if (!(step > 0.0) || !(step <= DBL_MAX)) return TQ_ERR_ARG;
    if (R < 1 || T < 2 || T > MAX_T || ldx < T || (y && ldy < T)) return TQ_ERR_SHAPE;
    if (n_fractions < 1 || n_fractions > MAX_F) return TQ_ERR_SHAPE;
    Fractions fr;
    for (int j = 0; j < MAX_F; ++j) {
        fr.f[j] = j < n_fractions ? fractions[j] : 0.0;
        if (!(fr.f[j] >= 0.0 && fr.f[j] <= 1.0)) return TQ_ERR_ARG;
    }
    if (husid && (overlap(husid, T, x, ldx, R, T) || (y && overlap(husid, T, y, ldy, R, T)))) return TQ_ERR_ARG;
    const double half_step = 0.5 * step;   // exact; 0.5 (a + b) step == (a + b) (0.5 step) bit for bit
    if (y) {
        if (husid) launch_arias<true, true>(x, y, energy, peak2, index, husid, R, T, ldx, ldy, half_step, fr, n_fractions, s);
        else launch_arias<true, false>(x, y, energy, peak2, index, husid, R, T, ldx, ldy, half_step, fr, n_fractions, s);
    } else {
        if (husid) launch_arias<false, true>(x, y, energy, peak2, index, husid, R, T, ldx, ldy, half_step, fr, n_fractions, s);
        else launch_arias<false, false>(x, y, energy, peak2, index, husid, R, T, ldx, ldy, half_step, fr, n_fractions, s);
    }
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tqd_gradient(const float* x, float* g, int R, int T, int64_t ldx, int64_t ldg, float dt, hipStream_t s) {
    if (!x || !g) return TQ_ERR_ARG;
    if (!(dt > 0.f) || !(dt <= FLT_MAX)) return TQ_ERR_ARG;
    if (R < 1 || T < 2 || T > MAX_T || ldx < T || ldg < T) return TQ_ERR_SHAPE;
    if (overlap(g, ldg, x, ldx, R, T)) return TQ_ERR_ARG;
    const dim3 grid((unsigned)((T + GRAD_THREADS - 1) / GRAD_THREADS), (unsigned)(R < 65535 ? R : 65535));
    hipLaunchKernelGGL(gradient_kernel, grid, dim3(GRAD_THREADS), 0, s, x, g, R, T, (long long)ldx, (long long)ldg, dt, 2.f * dt);
    TQ_CHECK_LAUNCH();
    return 0;
}
