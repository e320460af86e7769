// The NCW <-> channels-last boundary of models with 17 ... 64 signal channels at either end.
//
// The dedicated stem / head kernels (small_ops.hip, ends_wide.hip, backward.hip) are exact-fp32 FMA kernels that keep K x C_out sums or
// weights per thread and stop at 16 signal channels.  Beyond that the end convs are ordinary 32- / 64-channel contractions and run on
// the MFMA conv kernels, which read and write (B, T, C) channels-last tensors whose channel count is a multiple of 32.  The two kernels
// here are the layout change in front of and behind them, with what the dedicated kernels fold into it:
//   tq_nct_to_btc   (B, C0, T) [* scale[b]] ++ (B, C1, T) -> (B, T, Cp), channels >= C0 + C1 written as 0 on every call
//                   (forward: the stem's input, scale = c_in, cond = the conditioning signal; backward: dF = c_out[b] * dpred)
//   tq_btc_to_nct   channels [c_off, c_off + C) of (B, T, Cp) -> (B, C, T), y = v * a[b] + s[b] * skip_src
//                   (forward: the head's preconditioning epilogue; backward: d loss / d x = in_scale[b] * dgrad)
// Workgroup = (sample, 64 positions).  The tile goes through LDS as [channel][65] floats: the NCW side moves 64 consecutive positions of
// one channel per wave (256-byte rows, conflict-free LDS columns), the channels-last side 16-byte pieces of consecutive channels (LDS
// bank 4q + j + r for piece q of row r: conflict-free at Cp = 64, two-way at Cp = 32 -- tolerable, the kernels are memory-bound).
// Memory-bound: B T (C0 + C1 + Cp) floats once each.
#include "common.hpp"
#include "../../include/tqdne_hip.h"

using namespace tq;

namespace {
constexpr int BT = 64;            // positions per workgroup
constexpr int BLD = BT + 1;       // LDS row stride (floats)
constexpr int BMAXC = 64;         // most signal channels (tq_boundary_max_channels)
constexpr int BROWS = BMAXC + 4;  // tq_btc_to_nct stages whole 16-byte pieces around [c_off, c_off + C)

__global__ __launch_bounds__(256) void nct_to_btc_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                         const float* __restrict__ cond, float* __restrict__ out, int C0, int C1,
                                                         int T, int Cp, int ntile) {
    __shared__ float tile[BMAXC * BLD];
    const int b = blockIdx.x / ntile, t0 = (blockIdx.x % ntile) * BT;
    const int tid = threadIdx.x, tx = tid & 63, cy = tid >> 6;
    const int Ct = C0 + C1;
    const float sc = scale ? scale[b] : 1.0f;
    const int t = t0 + tx;
    for (int c = cy; c < Ct; c += 4) {
        float v = 0.f;
        if (t < T) {
            if (c < C0) {
                v = x[((size_t)b * C0 + c) * T + t];
                if (scale) v *= sc;
            } else {
                v = cond[((size_t)b * C1 + (c - C0)) * T + t];
            }
        }
        tile[c * BLD + tx] = v;
    }
    __syncthreads();
    const int nq = Cp >> 2;
    const int rows = min(BT, T - t0);
    for (int i = tid; i < rows * nq; i += 256) {
        const int r = i / nq, c4 = (i - r * nq) * 4;
        float4 o;
        o.x = (c4 + 0 < Ct) ? tile[(c4 + 0) * BLD + r] : 0.f;
        o.y = (c4 + 1 < Ct) ? tile[(c4 + 1) * BLD + r] : 0.f;
        o.z = (c4 + 2 < Ct) ? tile[(c4 + 2) * BLD + r] : 0.f;
        o.w = (c4 + 3 < Ct) ? tile[(c4 + 3) * BLD + r] : 0.f;
        *reinterpret_cast<float4*>(out + ((size_t)b * T + t0 + r) * Cp + c4) = o;
    }
}

__global__ __launch_bounds__(256) void btc_to_nct_kernel(const float* __restrict__ v, const float* __restrict__ a,
                                                         const float* __restrict__ s, const float* __restrict__ skip,
                                                         float* __restrict__ y, int T, int Cp, int c_off, int C, int ntile) {
    __shared__ float tile[BROWS * BLD];
    const int b = blockIdx.x / ntile, t0 = (blockIdx.x % ntile) * BT;
    const int tid = threadIdx.x, tx = tid & 63, cy = tid >> 6;
    const int cb = c_off & ~3;                       // first staged channel (16-byte aligned in every row: 4 | Cp)
    const int nq = (c_off + C - cb + 3) >> 2;        // 16-byte pieces per row, <= BROWS / 4 (cb + 4 nq <= Cp: 4 | Cp)
    const int rows = min(BT, T - t0);
    for (int i = tid; i < rows * nq; i += 256) {
        const int r = i / nq, q = i - r * nq;
        const float4 u = *reinterpret_cast<const float4*>(v + ((size_t)b * T + t0 + r) * Cp + cb + 4 * q);
        tile[(4 * q + 0) * BLD + r] = u.x;
        tile[(4 * q + 1) * BLD + r] = u.y;
        tile[(4 * q + 2) * BLD + r] = u.z;
        tile[(4 * q + 3) * BLD + r] = u.w;
    }
    __syncthreads();
    const int t = t0 + tx;
    if (t >= T) return;
    const float av = a ? a[b] : 1.0f;
    const float sv = s ? s[b] : 0.0f;
    for (int c = cy; c < C; c += 4) {
        float o = tile[(c_off - cb + c) * BLD + tx];
        const size_t at = ((size_t)b * C + c) * T + t;
        if (a) o *= av;
        if (s) o += sv * skip[at];
        y[at] = o;
    }
}
}  // namespace

extern "C" int tq_boundary_max_channels(void) { return BMAXC; }

extern "C" int tq_nct_to_btc(const float* x_nct, const float* scale, const float* cond_nct, float* out_btc, int B, int C0, int C1,
                             int T, int Cp, hipStream_t stream) {
    if (!x_nct || !out_btc || B <= 0 || T <= 0 || C1 < 0 || (C1 > 0) != (cond_nct != nullptr)) return TQ_ERR_ARG;
    if (C0 <= 0 || Cp <= 0 || Cp % 32 != 0 || C0 + C1 > Cp || C0 + C1 > BMAXC) return TQ_ERR_SHAPE;
    const int ntile = (T + BT - 1) / BT;
    if ((size_t)B * ntile > 0x7fffffffull) return TQ_ERR_SHAPE;
    hipLaunchKernelGGL(nct_to_btc_kernel, dim3((unsigned)((size_t)B * ntile)), dim3(256), 0, stream, x_nct, scale, cond_nct, out_btc,
                       C0, C1, T, Cp, ntile);
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tq_btc_to_nct(const float* v_btc, const float* a, const float* s, const float* skip_src, float* y_nct, int B, int T,
                             int Cp, int c_off, int C, hipStream_t stream) {
    if (!v_btc || !y_nct || B <= 0 || T <= 0 || (s == nullptr) != (skip_src == nullptr)) return TQ_ERR_ARG;
    if (C <= 0 || C > BMAXC || c_off < 0 || Cp <= 0 || Cp % 32 != 0 || c_off + C > Cp) return TQ_ERR_SHAPE;
    const int ntile = (T + BT - 1) / BT;
    if ((size_t)B * ntile > 0x7fffffffull) return TQ_ERR_SHAPE;
    hipLaunchKernelGGL(btc_to_nct_kernel, dim3((unsigned)((size_t)B * ntile)), dim3(256), 0, stream, v_btc, a, s, skip_src, y_nct, T,
                       Cp, c_off, C, ntile);
    TQ_CHECK_LAUNCH();
    return 0;
}
