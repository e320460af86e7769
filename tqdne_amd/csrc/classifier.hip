// Classifier head (reference tqdne/classifier.py:39-59) behind the encoder's channels-last output conv, and its loss:
//   pooled = mean_t h;  a1 = W1 silu(pooled) + b1;  emb = W2 silu(a1) + b2;  logits = W3 emb + b3;  weighted cross-entropy.
// 33 MFLOP at B = 128, C = 256: plain fp32 FMAs, no MFMA, no split-precision scheme.  Every sum runs in an order fixed by the shape
// alone (no atomics): two calls on the same inputs give the same bits.
//
// Two building blocks, both over a row-major matrix M (rows x C) with 16-byte loads along C (4 | C):
//   vecmat:  out[c] = sum_r v[r] M[r, c]   (v == nullptr: v = 1, the pooling sum).  Thread (g, q) of the workgroup owns the float4 column q and
//            the rows g, g + G, g + 2G, ... (G = threads / (C / 4): at C = 256 one wave per row), adds them in that order, and the G partial
//            rows are combined through LDS by one thread per channel, g = 0 .. G-1 in order.
//   matvec:  out[j] = bias[j] + sum_c M[j, c] s[c]: one wave per output row, lane l takes the float4 columns l, l + 64, ..., then the
//            xor butterfly of wave_sum (the same tree on every call).
#include "common.hpp"
#include "../../include/tqdne_hip.h"

namespace {
using namespace tq;

constexpr int CLS_NT = 1024;          // threads of the per-sample workgroups (16 waves)
constexpr int CLS_MAX_C = 1024;       // channels: 32 | C <= 1024 (the two LDS vectors, the partial rows of vecmat)
constexpr int CLS_MAX_K = 1024;       // classes (the LDS copy of one sample's d logits)
constexpr int CE_NT = 256;

__device__ __forceinline__ float sigmoid_exact(float u) { return 1.0f / (1.0f + expf(-u)); }
__device__ __forceinline__ float silu_exact(float u) { return u * sigmoid_exact(u); }
__device__ __forceinline__ float dsilu_exact(float u) {
    const float s = sigmoid_exact(u);
    return s * (1.0f + u * (1.0f - s));
}

// out[c] = sum_r v[r] M[r, c], c < C.  part: CLS_NT float4 of LDS; v and out: LDS (v may be nullptr); ends with a barrier.
__device__ __forceinline__ void vecmat(const float* __restrict__ M, const float* v, int rows, int C, float4* part, float* out) {
    const int nq = C >> 2, G = CLS_NT / nq;
    const int q = threadIdx.x % nq, g = threadIdx.x / nq;
    if (g < G) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4* col = reinterpret_cast<const float4*>(M) + q;
#pragma unroll 4
        for (int r = g; r < rows; r += G) {
            const float4 m = col[(size_t)r * nq];
            const float s = v ? v[r] : 1.0f;
            acc.x = fmaf(s, m.x, acc.x);
            acc.y = fmaf(s, m.y, acc.y);
            acc.z = fmaf(s, m.z, acc.z);
            acc.w = fmaf(s, m.w, acc.w);
        }
        part[g * nq + q] = acc;
    }
    __syncthreads();
    const float* pf = reinterpret_cast<const float*>(part);
    for (int c = threadIdx.x; c < C; c += CLS_NT) {
        float a = 0.f;
        for (int k = 0; k < G; ++k) a += pf[k * C + c];
        out[c] = a;
    }
    __syncthreads();
}

// one wave: bias[j] + sum_c M[j, c] s[c]   (s: LDS, C floats); the value is valid in every lane
__device__ __forceinline__ float row_dot(const float* __restrict__ M, const float* bias, const float* s, int j, int C) {
    const int lane = threadIdx.x & 63, nq = C >> 2;
    const float4* row = reinterpret_cast<const float4*>(M + (size_t)j * C);
    const float4* s4 = reinterpret_cast<const float4*>(s);
    float acc = 0.f;
    for (int q = lane; q < nq; q += 64) {
        const float4 m = row[q], x = s4[q];
        acc = fmaf(m.x, x.x, acc);
        acc = fmaf(m.y, x.y, acc);
        acc = fmaf(m.z, x.z, acc);
        acc = fmaf(m.w, x.w, acc);
    }
    return wave_sum(acc) + bias[j];
}

__global__ __launch_bounds__(CLS_NT) void head_fwd_kernel(const float* __restrict__ h, const float* __restrict__ W1,
                                                          const float* __restrict__ b1, const float* __restrict__ W2,
                                                          const float* __restrict__ b2, const float* __restrict__ W3,
                                                          const float* __restrict__ b3, float* __restrict__ pooled,
                                                          float* __restrict__ a1, float* __restrict__ emb, float* __restrict__ logits,
                                                          int T, int C, int K) {
    __shared__ float4 part[CLS_NT];
    __shared__ __attribute__((aligned(16))) float va[CLS_MAX_C];
    __shared__ __attribute__((aligned(16))) float vb[CLS_MAX_C];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, NW = CLS_NT / 64;
    const size_t row = (size_t)b * C;
    vecmat(h + (size_t)b * T * C, nullptr, T, C, part, va);
    const float fT = (float)T;
    for (int c = threadIdx.x; c < C; c += CLS_NT) {
        const float p = va[c] / fT;
        pooled[row + c] = p;
        vb[c] = silu_exact(p);
    }
    __syncthreads();
    for (int j = wave; j < C; j += NW) {   // a1 = W1 silu(pooled) + b1; va <- silu(a1)
        const float v = row_dot(W1, b1, vb, j, C);
        if (lane == 0) {
            a1[row + j] = v;
            va[j] = silu_exact(v);
        }
    }
    __syncthreads();
    for (int j = wave; j < C; j += NW) {   // emb = W2 silu(a1) + b2
        const float v = row_dot(W2, b2, va, j, C);
        if (lane == 0) {
            emb[row + j] = v;
            vb[j] = v;
        }
    }
    if (!logits) return;
    __syncthreads();
    for (int k = wave; k < K; k += NW) {
        const float v = row_dot(W3, b3, vb, k, C);
        if (lane == 0) logits[(size_t)b * K + k] = v;
    }
}

// Per-sample chain of the backward.  ws: five (B, C) planes [d emb | d a1 | d pooled / T | silu(pooled) | silu(a1)].
__global__ __launch_bounds__(CLS_NT) void head_bwd_chain_kernel(const float* __restrict__ dlogits, const float* __restrict__ pooled,
                                                                const float* __restrict__ a1, const float* __restrict__ W1,
                                                                const float* __restrict__ W2, const float* __restrict__ W3,
                                                                float* __restrict__ ws, int B, int T, int C, int K) {
    __shared__ float4 part[CLS_NT];
    __shared__ float va[CLS_MAX_C];
    __shared__ float vb[CLS_MAX_C];
    __shared__ float vk[CLS_MAX_K];
    const int b = blockIdx.x;
    const size_t row = (size_t)b * C, plane = (size_t)B * C;
    if (W3) {
        for (int k = threadIdx.x; k < K; k += CLS_NT) vk[k] = dlogits[(size_t)b * K + k];
        __syncthreads();
        vecmat(W3, vk, K, C, part, va);             // d emb = W3^T d logits
    } else {                                        // (embed() under autograd: the incoming gradient is d emb itself)
        for (int c = threadIdx.x; c < C; c += CLS_NT) va[c] = dlogits[row + c];
        __syncthreads();
    }
    for (int c = threadIdx.x; c < C; c += CLS_NT) {
        ws[row + c] = va[c];
        ws[3 * plane + row + c] = silu_exact(pooled[row + c]);
        ws[4 * plane + row + c] = silu_exact(a1[row + c]);
    }
    vecmat(W2, va, C, C, part, vb);                 // d silu(a1) = W2^T d emb
    for (int c = threadIdx.x; c < C; c += CLS_NT) {
        const float d = vb[c] * dsilu_exact(a1[row + c]);
        vb[c] = d;                                  // (each thread rewrites the entries it alone reads here)
        ws[plane + row + c] = d;
    }
    __syncthreads();
    vecmat(W1, vb, C, C, part, va);                 // d silu(pooled) = W1^T d a1
    const float fT = (float)T;
    for (int c = threadIdx.x; c < C; c += CLS_NT) ws[2 * plane + row + c] = va[c] * dsilu_exact(pooled[row + c]) / fT;
}

// dW (J, C) = sum_b g[b, j] x[b, c] and db (J) = sum_b g[b, j], b = 0 .. B-1 in order: one thread per output, layer = blockIdx.y.
struct WgradLayer {
    const float* g;
    const float* x;
    float* dW;
    float* db;
    int J;
};
struct WgradArgs {
    WgradLayer l[3];
};

__global__ __launch_bounds__(256) void head_bwd_wgrad_kernel(WgradArgs a, int first, int B, int C) {
    const WgradLayer L = a.l[first + blockIdx.y];
    const int J = L.J;
    const long long nW = (long long)J * C;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id < nW) {
        const int j = (int)(id / C), c = (int)(id % C);
        const float* g = L.g + j;
        const float* x = L.x + c;
        float acc = 0.f;
#pragma unroll 4
        for (int b = 0; b < B; ++b) acc = fmaf(g[(size_t)b * J], x[(size_t)b * C], acc);
        L.dW[id] = acc;
    } else if (id < nW + J) {
        const int j = (int)(id - nW);
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += L.g[(size_t)b * J + j];
        L.db[j] = acc;
    }
}

// dh[b, t, :] = dp[b, :] for every t (dp already holds d pooled / T): 16-byte stores
__global__ __launch_bounds__(256) void head_bwd_broadcast_kernel(const float* __restrict__ dp, float* __restrict__ dh, int T, int C) {
    const int b = blockIdx.x, nq = C >> 2;
    const float4* src = reinterpret_cast<const float4*>(dp + (size_t)b * C);
    float4* dst = reinterpret_cast<float4*>(dh + (size_t)b * T * C);
    const size_t total = (size_t)T * nq, step = (size_t)gridDim.y * 256;
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < total; i += step) dst[i] = src[i % nq];
}

// One workgroup.  Thread i takes the samples i, i + 256, ...; the per-thread sums are combined by a fixed tree in fp64.
__global__ __launch_bounds__(CE_NT) void cross_entropy_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ weight, long long ignore_index,
                                                              float* __restrict__ loss_out, float* __restrict__ dlogits, int B, int K) {
    __shared__ double s_num[CE_NT], s_den[CE_NT];
    const int tid = threadIdx.x;
    double num = 0.0, den = 0.0;
    for (int i = tid; i < B; i += CE_NT) {
        const long long y = labels[i];
        if (y == ignore_index || y < 0 || y >= K) continue;
        const float* r = logits + (size_t)i * K;
        float m = r[0];
        for (int k = 1; k < K; ++k) m = fmaxf(m, r[k]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(r[k] - m);
        const float nll = (m - r[y]) + logf(s);
        const float w = weight ? weight[y] : 1.0f;
        num += (double)w * (double)nll;
        den += (double)w;
    }
    s_num[tid] = num;
    s_den[tid] = den;
    __syncthreads();
    for (int o = CE_NT / 2; o > 0; o >>= 1) {
        if (tid < o) {
            s_num[tid] += s_num[tid + o];
            s_den[tid] += s_den[tid + o];
        }
        __syncthreads();
    }
    const double total = s_den[0];
    if (tid == 0) loss_out[0] = (float)(s_num[0] / total);   // (0 / 0 = NaN when every label is ignored, as in torch)
    if (!dlogits) return;
    const float inv = (float)(1.0 / total);
    for (int i = tid; i < B; i += CE_NT) {
        const long long y = labels[i];
        float* d = dlogits + (size_t)i * K;
        if (y == ignore_index || y < 0 || y >= K) {
            for (int k = 0; k < K; ++k) d[k] = 0.f;
            continue;
        }
        const float* r = logits + (size_t)i * K;
        float m = r[0];
        for (int k = 1; k < K; ++k) m = fmaxf(m, r[k]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(r[k] - m);
        const float ws = (weight ? weight[y] : 1.0f) * inv;
        for (int k = 0; k < K; ++k) d[k] = ws * (expf(r[k] - m) / s - (k == y ? 1.0f : 0.0f));
    }
}

int head_shape(int B, int T, int C, int K) {
    if (B <= 0 || T <= 0 || C <= 0 || K <= 0) return TQ_ERR_ARG;
    if (C % 32 != 0 || C > CLS_MAX_C || K > CLS_MAX_K) return TQ_ERR_SHAPE;
    return 0;
}
}  // namespace

extern "C" int tq_classifier_head_max_channels(void) { return CLS_MAX_C; }
extern "C" int tq_classifier_head_max_classes(void) { return CLS_MAX_K; }
extern "C" size_t tq_classifier_head_bwd_workspace(int B, int C) {
    if (B <= 0 || C <= 0) return 0;
    return (size_t)5 * (size_t)B * (size_t)C * sizeof(float);
}

extern "C" int tq_classifier_head_fwd(const float* h, const float* W1, const float* b1, const float* W2, const float* b2,
                                      const float* W3, const float* b3, float* pooled, float* a1, float* emb, float* logits, int B,
                                      int T, int C, int K, hipStream_t stream) {
    if (!h || !W1 || !b1 || !W2 || !b2 || !pooled || !a1 || !emb) return TQ_ERR_ARG;
    if (logits && (!W3 || !b3)) return TQ_ERR_ARG;
    const int rc = head_shape(B, T, C, logits ? K : 1);
    if (rc) return rc;
    hipLaunchKernelGGL(head_fwd_kernel, dim3(B), dim3(CLS_NT), 0, stream, h, W1, b1, W2, b2, W3, b3, pooled, a1, emb, logits, T, C, K);
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tq_cross_entropy(const float* logits, const int64_t* labels, const float* weight, int64_t ignore_index, float* loss_out,
                                float* dlogits, int B, int K, hipStream_t stream) {
    if (!logits || !labels || !loss_out || B <= 0 || K <= 0) return TQ_ERR_ARG;
    if (K > CLS_MAX_K) return TQ_ERR_SHAPE;
    hipLaunchKernelGGL(cross_entropy_kernel, dim3(1), dim3(CE_NT), 0, stream, logits, labels, weight, (long long)ignore_index, loss_out,
                       dlogits, B, K);
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tq_classifier_head_bwd(const float* dlogits, const float* pooled, const float* a1, const float* emb, const float* W1,
                                      const float* W2, const float* W3, float* dW3, float* db3, float* dW2, float* db2, float* dW1,
                                      float* db1, float* dh, void* workspace, size_t workspace_bytes, int B, int T, int C, int K,
                                      hipStream_t stream) {
    if (!dlogits || !pooled || !a1 || !emb || !W1 || !W2 || !dW2 || !db2 || !dW1 || !db1 || !dh || !workspace) return TQ_ERR_ARG;
    if (W3 && (!dW3 || !db3)) return TQ_ERR_ARG;
    if (!W3) K = 1;
    const int rc = head_shape(B, T, C, K);
    if (rc) return rc;
    if (workspace_bytes < tq_classifier_head_bwd_workspace(B, C)) return TQ_ERR_ARG;
    float* ws = static_cast<float*>(workspace);
    const size_t plane = (size_t)B * C;
    hipLaunchKernelGGL(head_bwd_chain_kernel, dim3(B), dim3(CLS_NT), 0, stream, dlogits, pooled, a1, W1, W2, W3, ws, B, T, C, K);
    TQ_CHECK_LAUNCH();
    WgradArgs wa;
    wa.l[0] = WgradLayer{dlogits, emb, dW3, db3, K};
    wa.l[1] = WgradLayer{ws, ws + 4 * plane, dW2, db2, C};
    wa.l[2] = WgradLayer{ws + plane, ws + 3 * plane, dW1, db1, C};
    const int first = W3 ? 0 : 1, Jmax = (W3 && K > C) ? K : C;
    const unsigned gx = (unsigned)(((long long)Jmax * (C + 1) + 255) / 256);
    hipLaunchKernelGGL(head_bwd_wgrad_kernel, dim3(gx, 3 - first), dim3(256), 0, stream, wa, first, B, C);
    TQ_CHECK_LAUNCH();
    const size_t total4 = (size_t)T * (C >> 2);
    size_t gy = (total4 + 256 * 8 - 1) / (256 * 8);
    if (gy > 1024) gy = 1024;
    hipLaunchKernelGGL(head_bwd_broadcast_kernel, dim3(B, (unsigned)gy), dim3(256), 0, stream, ws + 2 * plane, dh, T, C);
    TQ_CHECK_LAUNCH();
    return 0;
}
