// LogSpectrogram representation (tqdne/representation.py:63-175): the STFT of librosa.stft at its defaults and the whole
// Griffin-Lim inversion of librosa.griffinlim in ONE launch, for n_fft = 256 (the reference's only configuration).
//
// The 256-point transform is a real-input FFT in registers and LDS, not an MFMA DFT: a DFT as a matrix product costs
// 2 * 256 * 129 multiply-adds per frame at the f32 MFMA's vector rate, the FFT below ~2.5 k; and a k-ordered 256-term fmaf
// chain has a larger worst-case rounding error than four radix-4 levels.  Layout of one transform:
//   * two real frames a, b are packed as z = a + i b and transformed by ONE complex 256-point FFT; the two spectra are
//     separated by the Hermitian symmetry  A[k] = (Z[k] + conj Z[256-k]) / 2,  B[k] = (Z[k] - conj Z[256-k]) / 2i  (and merged
//     the same way before the inverse);
//   * the complex FFT is 16 x 16: sixteen lanes own one frame pair, lane q holds elements q + 16 r (r = 0..15) in registers,
//     does a 16-point FFT on them (two radix-4 levels, constants only), multiplies by W256^(q k2), transposes the 16 x 16 block
//     through a padded LDS scratch private to the sixteen lanes, and does the second 16-point FFT.  Input and output are both
//     in the "lane q holds q + 16 r" layout, so the inverse consumes exactly what the forward produced;
//   * Z[256-k] lives in lane (16 - q) & 15: one width-16 shuffle per value (lane 0 keeps its own).
// Twiddles W256^m, the periodic Hann window and the window sum-square come from a table that tq_spectrogram_tables() computes
// in double on the host.  No fast-math functions, no atomics; every sum has a fixed order, so results are bit-reproducible and
// independent of the rest of the batch.
//
// tq_griffinlim: one workgroup of 512 threads per waveform, every iteration inside the launch.  Each of the 32 sixteen-lane
// groups owns two frame pairs (2p, 2p+1), p = group and group + 32, handled in two passes per iteration (hence the limit of
// 128 frames).  On-chip state, all in registers: per lane and pass the 8 bins x 2 frames it owns of S (16 registers) and of the
// previous rebuilt spectrum (32), plus the 32 windowed output samples of each pass that wait for the overlap-add: 160 of the 256
// registers a thread of a 512-thread workgroup may have (1024 threads x one pass spilled 120 registers at the 128-register cap).
// The current estimate A never exists as a whole: it is formed in registers and goes straight into the inverse FFT.  LDS: the
// padded time signal y and the window sum-square (L = hop (F - 1) + 256 floats each), the transposition scratch (32 x 272 floats)
// and the tables (768 floats): 72 KB at hop 32, F = 128; 105 KB at hop 64, F = 128.  The overlap-add runs in n_fft / hop phases
// separated by barriers (frames f and f + n_fft / hop do not overlap): no atomics, fixed order.
#include <cfloat>
#include <cmath>

#include "common.hpp"
#include "../../include/tqdne_hip.h"

namespace {

constexpr int NFFT = 256, NBIN = 128;
constexpr int GRP_PITCH = 17;        // pitch of the 16 x 16 transposition block: conflict-free rows and columns
constexpr int GRP_WORDS = 272;       // 16 * 17; 272 = 16 mod 32, so the two groups of a 32-lane half use disjoint banks
constexpr int TAB_WIN = 0, TAB_COS = NFFT, TAB_SIN = 2 * NFFT, TAB_WSS = 3 * NFFT;
constexpr int GL_THREADS = 512, GL_GROUPS = GL_THREADS / 16, GL_PASSES = 2, GL_MAX_FRAMES = 2 * GL_GROUPS * GL_PASSES;
constexpr int FWD_THREADS = 256, FWD_GROUPS = FWD_THREADS / 16, FWD_FRAMES = 2 * FWD_GROUPS, FWD_PITCH = FWD_FRAMES + 1;

// cos / sin of 2 pi m / 16, m = 0..9 (the products n1 * k2 of a 4 x 4 decomposition)
__device__ constexpr float C16[10] = {1.0f, (float)0.92387953251128674, (float)0.70710678118654752, (float)0.38268343236508977, 0.0f,
                                      (float)-0.38268343236508977, (float)-0.70710678118654752, (float)-0.92387953251128674, -1.0f,
                                      (float)-0.92387953251128674};
__device__ constexpr float S16[10] = {0.0f, (float)0.38268343236508977, (float)0.70710678118654752, (float)0.92387953251128674, 1.0f,
                                      (float)0.92387953251128674, (float)0.70710678118654752, (float)0.38268343236508977, 0.0f,
                                      (float)-0.38268343236508977};

// ordering of LDS traffic among the lanes of ONE wave (the transposition scratch is private to sixteen lanes of a wave): a wave's
// LDS instructions execute in order, so only the compiler has to be held
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 4-point DFT of (a, b, c, d); INV: the conjugate kernel
template <bool INV>
__device__ __forceinline__ void dft4(float ar, float ai, float br, float bi, float cr, float ci, float dr, float di, float& x0r,
                                     float& x0i, float& x1r, float& x1i, float& x2r, float& x2i, float& x3r, float& x3i) {
    const float s0r = ar + cr, s0i = ai + ci, s1r = ar - cr, s1i = ai - ci;
    const float s2r = br + dr, s2i = bi + di, s3r = br - dr, s3i = bi - di;
    x0r = s0r + s2r; x0i = s0i + s2i;
    x2r = s0r - s2r; x2i = s0i - s2i;
    if (!INV) {   // x1 = s1 - i s3, x3 = s1 + i s3
        x1r = s1r + s3i; x1i = s1i - s3r;
        x3r = s1r - s3i; x3i = s1i + s3r;
    } else {
        x1r = s1r - s3i; x1i = s1i + s3r;
        x3r = s1r + s3i; x3i = s1i - s3r;
    }
}

// 16-point FFT in registers, natural order in and out: n = n1 + 4 n2, k = 4 k1 + k2
template <bool INV>
__device__ __forceinline__ void fft16(float (&xr)[16], float (&xi)[16]) {
    float tr[16], ti[16];
#pragma unroll
    for (int n1 = 0; n1 < 4; ++n1) {
        dft4<INV>(xr[n1], xi[n1], xr[n1 + 4], xi[n1 + 4], xr[n1 + 8], xi[n1 + 8], xr[n1 + 12], xi[n1 + 12], tr[4 * n1], ti[4 * n1],
                  tr[4 * n1 + 1], ti[4 * n1 + 1], tr[4 * n1 + 2], ti[4 * n1 + 2], tr[4 * n1 + 3], ti[4 * n1 + 3]);
#pragma unroll
        for (int k2 = 1; k2 < 4; ++k2) {
            const int m = n1 * k2;
            if (m == 0) continue;
            const float c = C16[m], s = INV ? S16[m] : -S16[m];
            const float r = tr[4 * n1 + k2], i = ti[4 * n1 + k2];
            if (m == 4) {   // exactly -+ i
                tr[4 * n1 + k2] = INV ? -i : i;
                ti[4 * n1 + k2] = INV ? r : -r;
            } else {
                tr[4 * n1 + k2] = r * c - i * s;
                ti[4 * n1 + k2] = r * s + i * c;
            }
        }
    }
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2)
        dft4<INV>(tr[k2], ti[k2], tr[4 + k2], ti[4 + k2], tr[8 + k2], ti[8 + k2], tr[12 + k2], ti[12 + k2], xr[k2], xi[k2], xr[4 + k2],
                  xi[4 + k2], xr[8 + k2], xi[8 + k2], xr[12 + k2], xi[12 + k2]);
}

// complex 256-point FFT of sixteen lanes: lane q holds elements q + 16 r on entry and on exit.  ``sc``: the group's scratch.
template <bool INV>
__device__ __forceinline__ void fft256(float (&xr)[16], float (&xi)[16], int q, float* sc, const float* tcos, const float* tsin) {
    fft16<INV>(xr, xi);   // over n2 of x[q + 16 n2]: xr[k2] = Y[n1 = q][k2]
#pragma unroll
    for (int k2 = 1; k2 < 16; ++k2) {
        const float c = tcos[q * k2], s = INV ? tsin[q * k2] : -tsin[q * k2];
        const float r = xr[k2], i = xi[k2];
        xr[k2] = r * c - i * s;
        xi[k2] = r * s + i * c;
    }
    wave_sync();
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) sc[k2 * GRP_PITCH + q] = xr[k2];
    wave_sync();
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) xr[n1] = sc[q * GRP_PITCH + n1];
    wave_sync();
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) sc[k2 * GRP_PITCH + q] = xi[k2];
    wave_sync();
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) xi[n1] = sc[q * GRP_PITCH + n1];
    fft16<INV>(xr, xi);   // over n1: lane k2 = q now holds X[16 k1 + q] in element k1
}

// Z = FFT(a + i b) in the lane layout -> bins k = q + 16 r (r = 0..7) of A = FFT(a), B = FFT(b)
__device__ __forceinline__ void split_pair(const float (&zr)[16], const float (&zi)[16], int q, float (&ar)[8], float (&ai)[8],
                                           float (&br)[8], float (&bi)[8]) {
    const int partner = (16 - q) & 15;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        float pr = __shfl(zr[15 - r], partner, 16), pi = __shfl(zi[15 - r], partner, 16);   // Z[256 - k]
        if (q == 0) {
            pr = zr[(16 - r) & 15];
            pi = zi[(16 - r) & 15];
        }
        ar[r] = 0.5f * (zr[r] + pr);
        ai[r] = 0.5f * (zi[r] - pi);
        br[r] = 0.5f * (zi[r] + pi);
        bi[r] = 0.5f * (pr - zr[r]);
    }
}

// bins k = q + 16 r (r = 0..7) of two Hermitian spectra with a zero Nyquist bin -> Z = A + i B in the lane layout.  The imaginary
// part of DC is ignored, as irfft does.
__device__ __forceinline__ void merge_pair(const float (&ar)[8], const float (&ai)[8], const float (&br)[8], const float (&bi)[8],
                                           int q, float (&zr)[16], float (&zi)[16]) {
    const int partner = (16 - q) & 15;
    float nr[8], ni[8];   // Z[256 - k] = conj A + i conj B
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const bool dc = q == 0 && r == 0;
        const float xai = dc ? 0.f : ai[r], xbi = dc ? 0.f : bi[r];
        zr[r] = ar[r] - xbi;
        zi[r] = xai + br[r];
        nr[r] = ar[r] + xbi;
        ni[r] = br[r] - xai;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float pr = __shfl(nr[7 - j], partner, 16), pi = __shfl(ni[7 - j], partner, 16);
        if (q == 0) {   // lane 0: element 8 is the Nyquist bin (zero), element 8 + j mirrors its own element 8 - j
            pr = j == 0 ? 0.f : nr[(8 - j) & 7];
            pi = j == 0 ? 0.f : ni[(8 - j) & 7];
        }
        zr[8 + j] = pr;
        zi[8 + j] = pi;
    }
}

// ------------------------------------------------------------------------------------------------
// tq_stft_fwd: one workgroup = 32 consecutive frames of one waveform (16 frame pairs, 4 per wave); the results are staged in
// LDS as [bin][frame] so that every output row is written in runs of 32 frames.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FWD_THREADS) void stft_fwd_kernel(const float* __restrict__ x, float* __restrict__ spec,
                                                               float* __restrict__ repr, const float* __restrict__ tab, int T, int F,
                                                               int hop, int n_tiles, float clip, float log_clip, float scale) {
    __shared__ float lds[3 * NFFT + FWD_GROUPS * GRP_WORDS + 2 * NBIN * FWD_PITCH];
    float* win = lds + TAB_WIN;
    float* tcos = lds + TAB_COS;
    float* tsin = lds + TAB_SIN;
    float* tile = lds + 3 * NFFT + FWD_GROUPS * GRP_WORDS;
    const int tid = threadIdx.x, grp = tid >> 4, q = tid & 15;
    float* sc = lds + 3 * NFFT + grp * GRP_WORDS;
    const size_t n = blockIdx.x / n_tiles;
    const int f0 = (int)(blockIdx.x % n_tiles) * FWD_FRAMES;
    for (int i = tid; i < 3 * NFFT; i += FWD_THREADS) lds[i] = tab[i];
    __syncthreads();

    const int fa = f0 + 2 * grp, fb = fa + 1;
    const float* xn = x + n * (size_t)T;
    float zr[16], zi[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int j = q + 16 * r;
        const int ta = fa * hop - NFFT / 2 + j, tb = ta + hop;   // centred: n_fft / 2 zeros on either side
        const float w = win[j];
        zr[r] = (fa < F && ta >= 0 && ta < T) ? xn[ta] * w : 0.f;
        zi[r] = (fb < F && tb >= 0 && tb < T) ? xn[tb] * w : 0.f;
    }
    fft256<false>(zr, zi, q, sc, tcos, tsin);
    float ar[8], ai[8], br[8], bi[8];
    split_pair(zr, zi, q, ar, ai, br, bi);
#pragma unroll
    for (int r = 0; r < 8; ++r) {   // the Nyquist row is never formed
        float* t = tile + 2 * ((q + 16 * r) * FWD_PITCH + 2 * grp);
        t[0] = ar[r]; t[1] = ai[r]; t[2] = br[r]; t[3] = bi[r];
    }
    __syncthreads();
    for (int i = tid; i < NBIN * FWD_FRAMES; i += FWD_THREADS) {
        const int k = i / FWD_FRAMES, fl = i % FWD_FRAMES, f = f0 + fl;
        if (f >= F) continue;
        const float re = tile[2 * (k * FWD_PITCH + fl)], im = tile[2 * (k * FWD_PITCH + fl) + 1];
        const size_t o = (n * NBIN + k) * (size_t)F + f;
        if (spec) {
            spec[2 * o] = re;
            spec[2 * o + 1] = im;
        }
        if (repr) repr[o] = (logf(fmaxf(hypotf(re, im), clip)) - log_clip) * scale - 1.0f;
    }
}

// ------------------------------------------------------------------------------------------------
// tq_griffinlim
// ------------------------------------------------------------------------------------------------
struct GlLds {
    float *win, *tcos, *tsin, *sc, *y, *wss;
};

// A (in registers) -> the windowed frames of istft(A), in the lane layout (wr: frame a, wi: frame b)
__device__ __forceinline__ void gl_inverse(const float (&ar)[8], const float (&ai)[8], const float (&br)[8], const float (&bi)[8],
                                           const GlLds& m, int q, float (&wr)[16], float (&wi)[16]) {
    merge_pair(ar, ai, br, bi, q, wr, wi);
    fft256<true>(wr, wi, q, m.sc, m.tcos, m.tsin);
#pragma unroll
    for (int r = 0; r < 16; ++r) {   // irfft's 1 / n_fft (exact), then the window
        const float w = m.win[q + 16 * r];
        wr[r] = wr[r] * (1.0f / NFFT) * w;
        wi[r] = wi[r] * (1.0f / NFFT) * w;
    }
}

// windowed frames -> y = istft(A) in LDS, padded by n_fft / 2 zeros on either side (what the following stft frames)
__device__ __forceinline__ void gl_overlap_add(const float (&wr)[GL_PASSES][16], const float (&wi)[GL_PASSES][16], const GlLds& m,
                                               int grp, int q, int F, int hop, int L) {
    const int tid = threadIdx.x, nph = NFFT / hop;
    __syncthreads();   // every wave has read the previous y
    for (int i = tid; i < L; i += GL_THREADS) m.y[i] = 0.f;
    __syncthreads();
    for (int ph = 0; ph < nph; ++ph) {   // frames f and f + nph do not overlap: fixed order, no atomics
#pragma unroll
        for (int ps = 0; ps < GL_PASSES; ++ps) {
            const int fa = 2 * (grp + GL_GROUPS * ps), fb = fa + 1;
            if (fa < F && fa % nph == ph) {
#pragma unroll
                for (int r = 0; r < 16; ++r) m.y[fa * hop + q + 16 * r] += wr[ps][r];
            }
            if (fb < F && fb % nph == ph) {
#pragma unroll
                for (int r = 0; r < 16; ++r) m.y[fb * hop + q + 16 * r] += wi[ps][r];
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < L; i += GL_THREADS) {
        const float v = m.y[i], w = m.wss[i];
        const float u = w > FLT_MIN ? v / w : v;
        m.y[i] = (i >= NFFT / 2 && i < L - NFFT / 2) ? u : 0.f;   // trimmed, then zero-padded again for the next stft
    }
    __syncthreads();
}

__global__ __launch_bounds__(GL_THREADS) void griffinlim_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                const float* __restrict__ tab, const float* __restrict__ phase,
                                                                int F, int hop, int n_iter, float alpha, int log_input,
                                                                float log_range, float log_clip) {
    extern __shared__ float gl_lds[];
    const int L = hop * (F - 1) + NFFT;
    GlLds m;
    m.win = gl_lds + TAB_WIN;
    m.tcos = gl_lds + TAB_COS;
    m.tsin = gl_lds + TAB_SIN;
    const int tid = threadIdx.x, grp = tid >> 4, q = tid & 15;
    m.sc = gl_lds + 3 * NFFT + grp * GRP_WORDS;
    m.y = gl_lds + 3 * NFFT + GL_GROUPS * GRP_WORDS;
    m.wss = m.y + L;
    for (int i = tid; i < 3 * NFFT; i += GL_THREADS) gl_lds[i] = tab[i];
    for (int i = tid; i < L; i += GL_THREADS) m.wss[i] = tab[TAB_WSS + i];
    __syncthreads();

    const size_t n = blockIdx.x;
    float sa[GL_PASSES][8], sb[GL_PASSES][8];   // magnitudes of the 8 bins x 2 frames x GL_PASSES pairs this lane owns
    float par[GL_PASSES][8], pai[GL_PASSES][8], pbr[GL_PASSES][8], pbi[GL_PASSES][8];   // previous rebuilt spectrum
    float wr[GL_PASSES][16], wi[GL_PASSES][16];                                         // windowed frames awaiting the overlap-add
#pragma unroll
    for (int ps = 0; ps < GL_PASSES; ++ps) {
        const int fa = 2 * (grp + GL_GROUPS * ps), fb = fa + 1;
        float ar[8], ai[8], br[8], bi[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k = q + 16 * r;
            const size_t o = (n * NBIN + k) * (size_t)F;
            float va = fa < F ? in[o + fa] : 0.f, vb = fb < F ? in[o + fb] : 0.f;
            if (log_input) {   // LogSpectrogram.invert_representation: exp((r + 1) / 2 * (log_max - log clip) + log clip)
                va = fa < F ? expf((va + 1.0f) * 0.5f * log_range + log_clip) : 0.f;
                vb = fb < F ? expf((vb + 1.0f) * 0.5f * log_range + log_clip) : 0.f;
            }
            sa[ps][r] = va;
            sb[ps][r] = vb;
            const size_t p = (size_t)k * F;
            const float ca = fa < F ? phase[2 * (p + fa)] : 0.f, sna = fa < F ? phase[2 * (p + fa) + 1] : 0.f;
            const float cb = fb < F ? phase[2 * (p + fb)] : 0.f, snb = fb < F ? phase[2 * (p + fb) + 1] : 0.f;
            ar[r] = ca * va; ai[r] = sna * va;
            br[r] = cb * vb; bi[r] = snb * vb;
            par[ps][r] = pai[ps][r] = pbr[ps][r] = pbi[ps][r] = 0.f;   // the first iteration has no momentum term
        }
        gl_inverse(ar, ai, br, bi, m, q, wr[ps], wi[ps]);
    }
    gl_overlap_add(wr, wi, m, grp, q, F, hop, L);

    for (int it = 0; it < n_iter; ++it) {
#pragma unroll
        for (int ps = 0; ps < GL_PASSES; ++ps) {
            const int fa = 2 * (grp + GL_GROUPS * ps), fb = fa + 1;
            if (2 * GL_GROUPS * ps >= F) continue;   // (uniform over the workgroup) no frame in this pass: its wr / wi are never added
            float zr[16], zi[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = q + 16 * r;
                const float w = m.win[j];
                zr[r] = fa < F ? m.y[fa * hop + j] * w : 0.f;
                zi[r] = fb < F ? m.y[fb * hop + j] * w : 0.f;
            }
            fft256<false>(zr, zi, q, m.sc, m.tcos, m.tsin);
            float ar[8], ai[8], br[8], bi[8];
            split_pair(zr, zi, q, ar, ai, br, bi);   // R
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float car = ar[r] - alpha * par[ps][r], cai = ai[r] - alpha * pai[ps][r];
                const float cbr = br[r] - alpha * pbr[ps][r], cbi = bi[r] - alpha * pbi[ps][r];
                par[ps][r] = ar[r]; pai[ps][r] = ai[r]; pbr[ps][r] = br[r]; pbi[ps][r] = bi[r];
                const float da = hypotf(car, cai) + FLT_MIN, db = hypotf(cbr, cbi) + FLT_MIN;
                ar[r] = car / da * sa[ps][r]; ai[r] = cai / da * sa[ps][r];
                br[r] = cbr / db * sb[ps][r]; bi[r] = cbi / db * sb[ps][r];
            }
            gl_inverse(ar, ai, br, bi, m, q, wr[ps], wi[ps]);
        }
        gl_overlap_add(wr, wi, m, grp, q, F, hop, L);
    }
    const int T = hop * (F - 1);
    float* o = out + n * (size_t)T;
    for (int i = tid; i < T; i += GL_THREADS) o[i] = m.y[NFFT / 2 + i];
}

bool supported(int n_fft, int hop) { return n_fft == NFFT && (hop == 32 || hop == 64); }

constexpr size_t gl_lds_bytes(int hop, int F) {
    return sizeof(float) * ((size_t)3 * NFFT + (size_t)GL_GROUPS * GRP_WORDS + 2 * ((size_t)hop * (F - 1) + NFFT));
}
// the frame limit is the register layout's (32 sixteen-lane groups x 2 passes, one frame pair each); the LDS of one CU holds it
static_assert(gl_lds_bytes(64, GL_MAX_FRAMES) <= 160 * 1024, "y + window sum-square + scratch must fit one CU's LDS at the widest hop");

}  // namespace

extern "C" int tq_griffinlim_max_frames(int n_fft, int hop) {
    if (n_fft <= 0 || hop <= 0 || n_fft % hop) return TQ_ERR_ARG;
    if (!supported(n_fft, hop)) return TQ_ERR_SHAPE;
    return GL_MAX_FRAMES;
}

extern "C" size_t tq_spectrogram_table_floats(int n_fft, int hop, int F) {
    if (n_fft <= 0 || hop <= 0 || n_fft % hop || !supported(n_fft, hop) || F < 0) return 0;
    return (size_t)3 * n_fft + (F > 0 ? (size_t)hop * (F - 1) + n_fft : 0);
}

extern "C" int tq_spectrogram_tables(int n_fft, int hop, int F, float* host_out) {
    if (!host_out || n_fft <= 0 || hop <= 0 || n_fft % hop || F < 0) return TQ_ERR_ARG;
    if (!supported(n_fft, hop)) return TQ_ERR_SHAPE;
    const double two_pi = 6.283185307179586476925286766559;
    double w2[NFFT];
    for (int i = 0; i < NFFT; ++i) {
        const double w = 0.5 - 0.5 * cos(two_pi * i / NFFT);   // periodic Hann
        w2[i] = w * w;
        host_out[TAB_WIN + i] = (float)w;
        host_out[TAB_COS + i] = (float)cos(two_pi * i / NFFT);
        host_out[TAB_SIN + i] = (float)sin(two_pi * i / NFFT);
    }
    if (F > 0) {
        const int L = hop * (F - 1) + NFFT;
        for (int i = 0; i < L; ++i) {   // sum over the frames that cover sample i, in frame order
            double s = 0.0;
            const int f_lo = i >= NFFT ? (i - NFFT) / hop + 1 : 0;
            for (int f = f_lo; f < F && f * hop <= i; ++f) s += w2[i - f * hop];
            host_out[TAB_WSS + i] = (float)s;
        }
    }
    return 0;
}

extern "C" int tq_stft_fwd(const float* x, float* spec, float* repr, const float* tables, int N, int T, int n_fft, int hop,
                           double clip, double log_max, hipStream_t stream) {
    if (!x || !tables || (!spec && !repr)) return TQ_ERR_ARG;
    if (n_fft <= 0 || hop <= 0 || n_fft % hop) return TQ_ERR_ARG;
    if (repr && !(clip > 0.0 && log_max > log(clip))) return TQ_ERR_ARG;
    if (!supported(n_fft, hop) || N <= 0 || T < n_fft) return TQ_ERR_SHAPE;
    const int F = 1 + T / hop;
    const int n_tiles = (F + FWD_FRAMES - 1) / FWD_FRAMES;
    if ((size_t)n_tiles * N > 0x7fffffffull) return TQ_ERR_SHAPE;
    const double lc = repr ? log(clip) : 0.0;
    hipLaunchKernelGGL(stft_fwd_kernel, dim3((unsigned)((size_t)n_tiles * N)), dim3(FWD_THREADS), 0, stream, x, spec, repr, tables, T,
                       F, hop, n_tiles, (float)clip, (float)lc, repr ? (float)(2.0 / (log_max - lc)) : 0.f);
    TQ_CHECK_LAUNCH();
    return 0;
}

extern "C" int tq_griffinlim(const float* in, float* out, const float* tables, const float* phase, int N, int F, int n_fft, int hop,
                             int n_iter, double momentum, int log_input, double clip, double log_max, hipStream_t stream) {
    if (!in || !out || !tables || !phase || n_iter < 0) return TQ_ERR_ARG;
    if (n_fft <= 0 || hop <= 0 || n_fft % hop || !(momentum >= 0.0)) return TQ_ERR_ARG;
    if (log_input && !(clip > 0.0 && log_max > log(clip))) return TQ_ERR_ARG;
    if (!supported(n_fft, hop) || N <= 0 || F < 1 || hop * (F - 1) < n_fft) return TQ_ERR_SHAPE;
    if (F > tq_griffinlim_max_frames(n_fft, hop)) return TQ_ERR_SHAPE;
    const size_t sh = gl_lds_bytes(hop, F);
    if (sh > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(griffinlim_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    const double lc = log_input ? log(clip) : 0.0;
    hipLaunchKernelGGL(griffinlim_kernel, dim3((unsigned)N), dim3(GL_THREADS), sh, stream, in, out, tables, phase, F, hop, n_iter,
                       (float)(momentum / (1.0 + momentum)), log_input, log_input ? (float)(log_max - lc) : 0.f, (float)lc);
    TQ_CHECK_LAUNCH();
    return 0;
}
