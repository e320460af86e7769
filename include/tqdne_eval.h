/* tqdne_eval.h -- C ABI of libtqdne_eval.so: the MI355X (gfx950) kernels of the evaluation stage that need a Fourier transform at
 * the signal's own length (tqdne/metric.py AmplitudeSpectralDensity; scripts/seismo_evaluations/utils.py integrate_frequency_domain,
 * filter_frequency_domain, fft).  A second library next to libtqdne_hip.so (include/tqdne_hip.h), with the same conventions:
 *   - device pointers only (tqe_rdft_tables: a host pointer), caller-owned memory, nothing allocated or synchronised inside;
 *   - all work is enqueued on the given HIP stream (graph-capture safe);
 *   - return 0 on success, a TQ_ERR_* code (negative) for bad arguments, or a hipError_t (>0) from the launch;
 *   - every argument is checked before the device is touched: a null pointer, an unknown mode or a log_eps that is not > 0 in
 *     TQE_RDFT_LOG mode return TQ_ERR_ARG; R < 1, F < 1, N < 2, N > tqe_rdft_max_length() or ld < N return TQ_ERR_SHAPE;
 *   - fp32 arithmetic without fast-math functions and without atomics, every sum in a fixed order: results are bit-reproducible, and
 *     a row's result does not depend on the rest of the batch.
 */
#ifndef TQDNE_EVAL_H
#define TQDNE_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define TQE_ABI_VERSION 1

#ifndef TQ_ERR_ARG
#define TQ_ERR_ARG (-1)   /* null / inconsistent pointer arguments */
#define TQ_ERR_SHAPE (-2) /* unsupported shape */
#endif

#define TQE_RDFT_COMPLEX 0 /* out (R, N/2+1, 2): re, im */
#define TQE_RDFT_ABS 1     /* out (R, N/2+1): |X| */
#define TQE_RDFT_LOG 2     /* out (R, N/2+1): log(max(|X|, log_eps)) */
#define TQE_RDFT_MAX_LENGTH 4096

int tqe_abi_version(void);

/* ---- real DFT of any length 2 <= N <= 4096 (csrc_eval/spectra.hip) ------------------------------------------------
 * One workgroup owns one row from load to store; the work array lives in LDS.
 *   N a power of two: a radix-2 FFT of M = N points (decimation in frequency; the bit-reversed result is read in place).
 *   any other N: Bluestein.  With the chirp c[n] = exp(-i pi (n^2 mod 2N) / N),
 *       X[k] = c[k] * sum_n (x[n] c[n]) * conj(c[k - n]),
 *     a circular convolution over M, the smallest power of two >= 2N - 1: forward FFT of x c (zero-padded), product with the
 *     transformed chirp filter, inverse FFT.  The forward FFT leaves its result bit-reversed, the filter is stored bit-reversed
 *     and the inverse FFT (decimation in time) consumes that order: no permutation pass.
 * tables (tqe_rdft_tables; evaluated in double on the host and rounded once; tqe_rdft_table_floats(N) floats, 0 where there is no
 * kernel for N), complex entries as (re, im) pairs:
 *     [0, M)                 twiddles exp(-2 pi i j / M), j = 0 .. M/2 - 1
 *   and for an N that is not a power of two
 *     [M, M + 2N)            chirp c[n], n = 0 .. N - 1
 *     [M + 2N, 3M + 2N)      FFT_M(b) / M at the bit-reversed index, b[m] = b[M - m] = conj(c[m]) for m < N, 0 elsewhere
 * tqe_rdft: R rows of N samples, row r at x + r * ld (ld >= N: a channel view of a (B, C, T) tensor goes in as it is); out dense,
 * the N/2 + 1 bins of numpy.fft.rfft in the form that ``mode`` selects.  log_eps is read in TQE_RDFT_LOG mode only.
 * tqe_spectral_filter: y (R, N) = Re IDFT(Hfull . DFT(x)) with Hfull[k] = h[k] on the N/2 + 1 non-negative bins (h (N/2+1, 2)) and
 * conj(h[N - k]) above them; the inverse is the forward transform between two conjugations, then 1 / N.  The imaginary part of
 * h X at DC and at the Nyquist bin contributes nothing (the real part of the full inverse is taken).
 * A row with a non-finite sample comes out all NaN (a workgroup-wide flag, set while the row is loaded); other rows are untouched. */
int tqe_rdft_max_length(void);
size_t tqe_rdft_table_floats(int N);
int tqe_rdft_tables(int N, float* host_out);
int tqe_rdft(const float* x, float* out, const float* tables, int R, int N, int64_t ld, int mode, float log_eps, hipStream_t s);
int tqe_spectral_filter(const float* x, const float* h, float* y, const float* tables, int R, int N, int64_t ld, hipStream_t s);

/* a (R, F) fp32 -> mean (F), std (F) in double: the population standard deviation (ddof = 0), two passes, sums of a column over
 * eight interleaved row classes combined in a fixed order.  Any R >= 1, F >= 1. */
int tqe_column_moments(const float* a, double* mean, double* std, int R, int F, hipStream_t s);

#ifdef __cplusplus
}
#endif
#endif /* TQDNE_EVAL_H */
