// Amplitude spectra of the evaluation stage (include/tqdne_eval.h): a batched real DFT at the signal's own length, 2 <= N <= 4096,
// the frequency-domain filter built on it, and float64 column moments.
//
// One workgroup of 256 threads owns one row from load to store.  The complex work array of M points (M = N for a power of two,
// else the smallest power of two >= 2N - 1 of Bluestein's convolution: at most 8192 points = 64 KiB) lives in LDS; twiddles, chirp and
// the transformed chirp filter are read from the table in global memory, which every workgroup shares (at most 112 KiB: it stays in
// L2).  The radix-2 levels (two per pass, on four points in registers) are decimation in frequency (natural order in, bit-reversed
// out) for the forward transform and decimation in time (bit-reversed in, natural out) for the inverse, so that the pointwise product
// between them needs no permutation: the filter table is stored bit-reversed.  No fast-math functions, no sincos, no atomics; every
// sum has a fixed order, and nothing a workgroup reads or writes belongs to another row: results are bit-reproducible and independent
// of the rest of the batch.
#include <cfloat>
#include <cmath>
#include <vector>

#include "../csrc/common.hpp"
#include "../../include/tqdne_eval.h"

namespace {

constexpr int MAX_N = TQE_RDFT_MAX_LENGTH, THREADS = 256;
constexpr int CM_COLS = 32, CM_WAYS = 8;   // tqe_column_moments: 32 columns x 8 row classes per workgroup

struct Plan {
    int N, M, logM, pow2;
};

bool make_plan(int N, Plan& p) {
    if (N < 2 || N > MAX_N) return false;
    p.N = N;
    p.pow2 = (N & (N - 1)) == 0;
    const int need = p.pow2 ? N : 2 * N - 1;
    p.M = 1;
    p.logM = 0;
    while (p.M < need) {
        p.M <<= 1;
        ++p.logM;
    }
    return true;
}

size_t lds_bytes(const Plan& p) { return sizeof(float2) * (size_t)p.M + 16; }   // work array, then the non-finite flag

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmul_conj(float2 a, float2 b) {   // a * conj(b)
    return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ int bitrev(int j, int logM) { return (int)(__brev((unsigned)j) >> (32 - logM)); }

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// forward FFT, decimation in frequency: natural order in, bit-reversed order out.  Ends with a barrier.  Radix-2 butterflies of span
// h with the twiddle exp(-2 pi i j / 2h) = tw[j << sh] (h << sh = M / 2); two consecutive levels (spans h and h / 2) are done on four
// points in registers between one pair of LDS accesses and one barrier, a last single level when log2 M is odd.
__device__ __forceinline__ void fft_dif(float2* w, const float2* __restrict__ tw, int M) {
    const int tid = threadIdx.x;
    int h = M >> 1, sh = 0;
    for (; h >= 2; h >>= 2, sh += 2) {
        const int q = h >> 1;
        for (int t = tid; t < (M >> 2); t += THREADS) {
            const int j = t & (q - 1), p = ((t - j) << 2) + j;
            const float2 u0 = w[p], u1 = w[p + q], u2 = w[p + h], u3 = w[p + h + q];
            const float2 s0 = cadd(u0, u2), d0 = cmul(csub(u0, u2), tw[j << sh]);            // span h
            const float2 s1 = cadd(u1, u3), d1 = cmul(csub(u1, u3), tw[(j + q) << sh]);
            const float2 c = tw[j << (sh + 1)];                                              // span h / 2
            w[p] = cadd(s0, s1);
            w[p + q] = cmul(csub(s0, s1), c);
            w[p + h] = cadd(d0, d1);
            w[p + h + q] = cmul(csub(d0, d1), c);
        }
        __syncthreads();
    }
    if (h == 1) {   // (sh = log2 M - 1: the twiddle is tw[0] = 1)
        for (int t = tid; t < (M >> 1); t += THREADS) {
            const float2 u = w[2 * t], v = w[2 * t + 1];
            w[2 * t] = cadd(u, v);
            w[2 * t + 1] = cmul(csub(u, v), tw[0]);
        }
        __syncthreads();
    }
}

// inverse FFT without its 1 / M (the filter table carries it), decimation in time: bit-reversed in, natural out.  Ends with a barrier.
// The mirror image of fft_dif: conjugate twiddles, spans h and 2 h per pass, a last single level of span M / 2 when log2 M is odd.
__device__ __forceinline__ void ifft_dit(float2* w, const float2* __restrict__ tw, int M, int logM) {
    const int tid = threadIdx.x;
    int h = 1, sh = logM - 1;
    for (; 4 * h <= M; h <<= 2, sh -= 2) {
        for (int t = tid; t < (M >> 2); t += THREADS) {
            const int j = t & (h - 1), p = ((t - j) << 2) + j;
            const float2 c = tw[j << sh];                                                    // span h
            const float2 u0 = w[p], v1 = cmul_conj(w[p + h], c), u2 = w[p + 2 * h], v3 = cmul_conj(w[p + 3 * h], c);
            const float2 a0 = cadd(u0, v1), a1 = csub(u0, v1), a2 = cadd(u2, v3), a3 = csub(u2, v3);
            const float2 b2 = cmul_conj(a2, tw[j << (sh - 1)]), b3 = cmul_conj(a3, tw[(j + h) << (sh - 1)]);   // span 2 h
            w[p] = cadd(a0, b2);
            w[p + h] = cadd(a1, b3);
            w[p + 2 * h] = csub(a0, b2);
            w[p + 3 * h] = csub(a1, b3);
        }
        __syncthreads();
    }
    if (2 * h == M) {   // (sh = 0)
        for (int t = tid; t < h; t += THREADS) {
            const float2 u = w[t], v = cmul_conj(w[t + h], tw[t]);
            w[t] = cadd(u, v);
            w[t + h] = csub(u, v);
        }
        __syncthreads();
    }
}

// row -> LDS (times the chirp for Bluestein, zero-padded to M).  Returns the workgroup-wide "a sample is not finite" flag.
__device__ __forceinline__ bool load_row(const float* __restrict__ xr, float2* w, int* flag, const float2* __restrict__ chirp, int N,
                                         int M, int pow2) {
    const int tid = threadIdx.x;
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int n = tid; n < M; n += THREADS) {
        float2 z = make_float2(0.f, 0.f);
        if (n < N) {
            const float v = xr[n];
            if (!(fabsf(v) <= FLT_MAX)) *flag = 1;   // (every writer stores the same value)
            if (pow2) {
                z.x = v;
            } else {
                const float2 c = chirp[n];
                z = make_float2(v * c.x, v * c.y);
            }
        }
        w[n] = z;
    }
    __syncthreads();
    return *flag != 0;
}

// the M-point convolution of Bluestein on a loaded work array: afterwards w[k] * chirp[k] is the DFT, k < N
__device__ __forceinline__ void bluestein_core(float2* w, const float2* __restrict__ tw, const float2* __restrict__ bhat, int M, int logM) {
    fft_dif(w, tw, M);
    for (int j = threadIdx.x; j < M; j += THREADS) w[j] = cmul(w[j], bhat[j]);
    __syncthreads();
    ifft_dit(w, tw, M, logM);
}

__global__ __launch_bounds__(THREADS) void rdft_kernel(const float* __restrict__ x, float* __restrict__ out, const float* __restrict__ tab,
                                                       int N, int M, int logM, int pow2, long long ld, int mode, float log_eps) {
    extern __shared__ __attribute__((aligned(16))) float2 rdft_lds[];
    float2* w = rdft_lds;
    int* flag = reinterpret_cast<int*>(rdft_lds + M);
    const float2* tw = reinterpret_cast<const float2*>(tab);
    const float2* chirp = reinterpret_cast<const float2*>(tab + M);
    const float2* bhat = reinterpret_cast<const float2*>(tab + M + 2 * (size_t)N);
    const int tid = threadIdx.x, K = N / 2 + 1;
    const size_t r = blockIdx.x;
    float* o = out + r * (size_t)K * (mode == TQE_RDFT_COMPLEX ? 2 : 1);
    if (load_row(x + r * ld, w, flag, chirp, N, M, pow2)) {
        const float nan = __builtin_nanf("");
        for (int i = tid; i < K * (mode == TQE_RDFT_COMPLEX ? 2 : 1); i += THREADS) o[i] = nan;
        return;
    }
    if (pow2)
        fft_dif(w, tw, M);
    else
        bluestein_core(w, tw, bhat, M, logM);
    for (int k = tid; k < K; k += THREADS) {
        const float2 X = pow2 ? w[bitrev(k, logM)] : cmul(w[k], chirp[k]);
        if (mode == TQE_RDFT_COMPLEX) {
            o[2 * k] = X.x;
            o[2 * k + 1] = X.y;
        } else {
            const float m = hypotf(X.x, X.y);
            o[k] = mode == TQE_RDFT_ABS ? m : logf(fmaxf(m, log_eps));
        }
    }
}

__device__ __forceinline__ float2 h_full(const float2* __restrict__ h, int k, int N) {
    if (2 * k <= N) return h[k];
    const float2 c = h[N - k];
    return make_float2(c.x, -c.y);
}

__global__ __launch_bounds__(THREADS) void spectral_filter_kernel(const float* __restrict__ x, const float* __restrict__ hh,
                                                                  float* __restrict__ y, const float* __restrict__ tab, int N, int M,
                                                                  int logM, int pow2, long long ld) {
    extern __shared__ __attribute__((aligned(16))) float2 filt_lds[];
    float2* w = filt_lds;
    int* flag = reinterpret_cast<int*>(filt_lds + M);
    const float2* tw = reinterpret_cast<const float2*>(tab);
    const float2* chirp = reinterpret_cast<const float2*>(tab + M);
    const float2* bhat = reinterpret_cast<const float2*>(tab + M + 2 * (size_t)N);
    const float2* h = reinterpret_cast<const float2*>(hh);
    const int tid = threadIdx.x;
    const size_t r = blockIdx.x;
    float* o = y + r * (size_t)N;
    if (load_row(x + r * ld, w, flag, chirp, N, M, pow2)) {
        const float nan = __builtin_nanf("");
        for (int i = tid; i < N; i += THREADS) o[i] = nan;
        return;
    }
    const float fN = (float)N;
    if (pow2) {
        fft_dif(w, tw, M);
        for (int j = tid; j < M; j += THREADS) w[j] = cmul(w[j], h_full(h, bitrev(j, logM), N));
        __syncthreads();
        ifft_dit(w, tw, M, logM);
        for (int n = tid; n < N; n += THREADS) o[n] = w[n].x / fN;
        return;
    }
    bluestein_core(w, tw, bhat, M, logM);
    for (int k = tid; k < M; k += THREADS) {   // Z = Hfull X; the inverse transform is the forward one of conj(Z), conjugated
        float2 z = make_float2(0.f, 0.f);
        if (k < N) {
            const float2 c = chirp[k];
            const float2 Z = cmul(cmul(w[k], c), h_full(h, k, N));
            z = cmul(make_float2(Z.x, -Z.y), c);
        }
        w[k] = z;
    }
    __syncthreads();
    bluestein_core(w, tw, bhat, M, logM);
    for (int n = tid; n < N; n += THREADS) {
        const float2 c = chirp[n], v = w[n];
        o[n] = (v.x * c.x - v.y * c.y) / fN;
    }
}

// 32 columns x 8 row classes: thread (c, q) sums rows q, q + 8, ... of its column, the eight partial sums are added in the order
// q = 0 .. 7; the same again for the squared deviations.
__global__ __launch_bounds__(CM_COLS* CM_WAYS) void column_moments_kernel(const float* __restrict__ a, double* __restrict__ mean,
                                                                         double* __restrict__ sd, int R, int F) {
    __shared__ double part[CM_WAYS][CM_COLS];
    __shared__ double mu[CM_COLS];
    const int c = threadIdx.x % CM_COLS, q = threadIdx.x / CM_COLS;
    const long long col = (long long)blockIdx.x * CM_COLS + c;
    const bool live = col < F;
    double s = 0.0;
    if (live)
        for (int r = q; r < R; r += CM_WAYS) s += (double)a[(size_t)r * F + col];
    part[q][c] = s;
    __syncthreads();
    if (q == 0) {
        double t = 0.0;
        for (int i = 0; i < CM_WAYS; ++i) t += part[i][c];
        mu[c] = t / (double)R;
    }
    __syncthreads();
    const double m = mu[c];
    s = 0.0;
    if (live)
        for (int r = q; r < R; r += CM_WAYS) {
            const double d = (double)a[(size_t)r * F + col] - m;
            s += d * d;
        }
    part[q][c] = s;   // (the first reduction has read ``part`` before the barrier that published ``mu``)
    __syncthreads();
    if (q == 0 && live) {
        double t = 0.0;
        for (int i = 0; i < CM_WAYS; ++i) t += part[i][c];
        mean[col] = m;
        sd[col] = sqrt(t / (double)R);
    }
}

// in-place double-precision radix-2 FFT (natural order in and out) for the chirp filter
void host_fft(std::vector<double>& re, std::vector<double>& im, int M, int logM) {
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < M; ++i) {
        int j = 0;
        for (int b = 0; b < logM; ++b) j |= ((i >> b) & 1) << (logM - 1 - b);
        if (j > i) {
            std::swap(re[i], re[j]);
            std::swap(im[i], im[j]);
        }
    }
    std::vector<double> c(M / 2 > 0 ? M / 2 : 1), s(M / 2 > 0 ? M / 2 : 1);
    for (int j = 0; j < M / 2; ++j) {
        c[j] = cos(two_pi * j / M);
        s[j] = -sin(two_pi * j / M);
    }
    for (int h = 1; h < M; h <<= 1) {
        const int step = M / (2 * h);
        for (int base = 0; base < M; base += 2 * h)
            for (int j = 0; j < h; ++j) {
                const int a = base + j, b = a + h;
                const double wr = c[j * step], wi = s[j * step];
                const double vr = re[b] * wr - im[b] * wi, vi = re[b] * wi + im[b] * wr;
                re[b] = re[a] - vr;
                im[b] = im[a] - vi;
                re[a] += vr;
                im[a] += vi;
            }
    }
}

template <typename K>
int opt_in_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024)
        return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return 0;
}

}  // namespace

extern "C" int tqe_abi_version(void) { return TQE_ABI_VERSION; }

extern "C" int tqe_rdft_max_length(void) { return MAX_N; }

extern "C" size_t tqe_rdft_table_floats(int N) {
    Plan p;
    if (!make_plan(N, p)) return 0;
    return p.pow2 ? (size_t)p.M : (size_t)3 * p.M + 2 * (size_t)N;
}

extern "C" int tqe_rdft_tables(int N, float* host_out) {
    if (!host_out) return TQ_ERR_ARG;
    Plan p;
    if (!make_plan(N, p)) return TQ_ERR_SHAPE;
    const double two_pi = 6.283185307179586476925286766559, pi = 0.5 * two_pi;
    const int M = p.M;
    for (int j = 0; j < M / 2; ++j) {
        host_out[2 * j] = (float)cos(two_pi * j / M);
        host_out[2 * j + 1] = (float)(-sin(two_pi * j / M));
    }
    if (p.pow2) return 0;
    float* chirp = host_out + M;
    float* bhat = host_out + M + 2 * (size_t)N;
    std::vector<double> br(M, 0.0), bi(M, 0.0);
    for (int n = 0; n < N; ++n) {
        const long long q = ((long long)n * n) % (2LL * N);   // exp(-i pi n^2 / N) has period 2N in n^2
        const double cr = cos(pi * (double)q / N), ci = -sin(pi * (double)q / N);
        chirp[2 * n] = (float)cr;
        chirp[2 * n + 1] = (float)ci;
        br[n] = cr;
        bi[n] = -ci;
        if (n) {
            br[M - n] = cr;
            bi[M - n] = -ci;
        }
    }
    host_fft(br, bi, M, p.logM);
    for (int j = 0; j < M; ++j) {
        int k = 0;
        for (int b = 0; b < p.logM; ++b) k |= ((j >> b) & 1) << (p.logM - 1 - b);
        bhat[2 * j] = (float)(br[k] / M);
        bhat[2 * j + 1] = (float)(bi[k] / M);
    }
    return 0;
}

extern "C" int tqe_rdft(const float* x, float* out, const float* tables, int R, int N, int64_t ld, int mode, float log_eps,
                        hipStream_t s) {
    if (!x || !out || !tables) return TQ_ERR_ARG;
    if (mode != TQE_RDFT_COMPLEX && mode != TQE_RDFT_ABS && mode != TQE_RDFT_LOG) return TQ_ERR_ARG;
    if (mode == TQE_RDFT_LOG && !(log_eps > 0.f)) return TQ_ERR_ARG;
    Plan p;
    if (R < 1 || !make_plan(N, p) || ld < N) return TQ_ERR_SHAPE;
    const size_t sh = lds_bytes(p);
    if (int e = opt_in_lds(rdft_kernel, sh)) return e;
    hipLaunchKernelGGL(rdft_kernel, dim3((unsigned)R), dim3(THREADS), sh, s, x, out, tables, N, p.M, p.logM, p.pow2, (long long)ld, mode,
                       log_eps);
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tqe_spectral_filter(const float* x, const float* h, float* y, const float* tables, int R, int N, int64_t ld,
                                   hipStream_t s) {
    if (!x || !h || !y || !tables) return TQ_ERR_ARG;
    Plan p;
    if (R < 1 || !make_plan(N, p) || ld < N) return TQ_ERR_SHAPE;
    const size_t sh = lds_bytes(p);
    if (int e = opt_in_lds(spectral_filter_kernel, sh)) return e;
    hipLaunchKernelGGL(spectral_filter_kernel, dim3((unsigned)R), dim3(THREADS), sh, s, x, h, y, tables, N, p.M, p.logM, p.pow2,
                       (long long)ld);
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tqe_column_moments(const float* a, double* mean, double* std, int R, int F, hipStream_t s) {
    if (!a || !mean || !std) return TQ_ERR_ARG;
    if (R < 1 || F < 1) return TQ_ERR_SHAPE;
    hipLaunchKernelGGL(column_moments_kernel, dim3((unsigned)((F + CM_COLS - 1) / CM_COLS)), dim3(CM_COLS * CM_WAYS), 0, s, a, mean, std,
                       R, F);
    TQ_CHECK_LAUNCH();
    return 0;
}
