/* tqdne_series.h -- C ABI of libtqdne_series.so: the MI355X (gfx950) kernels of the time-domain conditioning that the reference
 * applies before its intensity measures (scripts/seismo_evaluations/utils.py highpass_filter, moving_average_envelope_adaptive;
 * scripts/preprocessing/04_filter_waveforms.py detrend + causal band-pass).  A third library next to libtqdne_hip.so
 * (include/tqdne_hip.h) and libtqdne_eval.so (include/tqdne_eval.h), with the same conventions:
 *   - device pointers only, caller-owned memory, nothing allocated or synchronised inside;
 *   - all work is enqueued on the given HIP stream (graph-capture safe);
 *   - return 0 on success, a TQ_ERR_* code (negative) for bad arguments, or a hipError_t (>0) from the launch;
 *   - every argument is checked before the device is touched: a null pointer, an unknown detrend mode, a jump or add_eps that is not
 *     finite or an envelope asked to overwrite its input return TQ_ERR_ARG; R < 1, T < 1, T > 2^30, ldx < T, ldy < T, window < 1,
 *     n_sections < 1 or n_sections > tqs_sosfilt_max_sections() return TQ_ERR_SHAPE;
 *   - one lane owns one row from its first sample to its last: no LDS, no atomics, every sum in a fixed order.  Results are
 *     bit-reproducible, and a row's result does not depend on the rest of the batch;
 *   - a row with a non-finite sample comes out all NaN (found in a first walk over the row); other rows are untouched.
 */
#ifndef TQDNE_SERIES_H
#define TQDNE_SERIES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define TQS_ABI_VERSION 1

#ifndef TQ_ERR_ARG
#define TQ_ERR_ARG (-1)   /* null / inconsistent pointer arguments */
#define TQ_ERR_SHAPE (-2) /* unsupported shape */
#endif

#define TQS_DETREND_NONE 0   /* the samples as they are */
#define TQS_DETREND_DEMEAN 1 /* minus the row mean */
#define TQS_DETREND_LINEAR 2 /* minus the least-squares line (which contains the mean: demean-then-linear is this mode) */
#define TQS_SOSFILT_MAX_SECTIONS 8

int tqs_abi_version(void);
int tqs_sosfilt_max_sections(void);

/* ---- causal IIR filter as a cascade of second-order sections, after an optional detrend (csrc_series/series.hip) -------------
 * R rows of T samples, row r at x + r * ldx and y + r * ldy (ld >= T: a channel view of a (B, C, T) tensor goes in as it is).
 * sos: a device table (n_sections, 6) of doubles in scipy's layout b0 b1 b2 a0 a1 a2 with a0 == 1 (a0 is not read).  Each section
 * is direct form II transposed, scipy.signal.sosfilt's recurrence, from a zero state:
 *     y = b0 x + z1;   z1 = b1 x - a1 y + z2;   z2 = b2 x - a2 y,
 * the sections cascaded in table order.  State, coefficients and every intermediate signal are fp64 (the poles of a 0.1 Hz corner at
 * 100 Hz sit 0.006 from the unit circle: an fp32 state is off by 7e-5 of the peak); a sample is widened once and a result is rounded
 * to fp32 once.
 * detrend: in a first walk over the row, fp64 sums in sample order; the time axis is centred, tbar = (T - 1) / 2:
 *     mean = sum x / T,   slope = sum (t - tbar) x / sum (t - tbar)^2   (0 for T = 1: the line is the sample itself),
 * and the filter's input is x - mean (DEMEAN) or x - mean - slope (t - tbar) (LINEAR).
 * Any T >= 1 and R >= 1.  In-place use (y == x with ldy == ldx) is allowed; any other overlap of x and y is not. */
int tqs_sosfilt(const float* x, float* y, const double* sos, int R, int T, int64_t ldx, int64_t ldy, int n_sections, int detrend,
                hipStream_t s);

/* ---- the reference's hold-and-recompute envelope (moving_average_envelope_adaptive) ----------------------------------------
 * On a = |x|:  out[0] = a[0];  for i > 0:  out[i] = mean(a[max(0, i - window + 1) .. i]) if a[i] > jump * a[i-1], else out[i-1];
 * env = out + add_eps.  The reference has window 128, jump 5 and add_eps 1e-6 (it adds its ``log_eps`` and takes no logarithm).
 * The jump decision is taken in fp32: the product rounded, then the compare (numpy's decision on a float32 input).  The window sum
 * is carried in fp64 (the entering sample added, the leaving one subtracted), out + add_eps is formed in fp64 and rounded once.
 * window >= 1 and may exceed T.  env must not be x: the leaving sample is read again after the entering one was written. */
int tqs_hold_envelope(const float* x, float* env, int R, int T, int64_t ldx, int64_t ldy, int window, float jump, float add_eps,
                      hipStream_t s);

#ifdef __cplusplus
}
#endif
#endif /* TQDNE_SERIES_H */
