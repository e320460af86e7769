/* tqdne_duration.h -- C ABI of libtqdne_duration.so: the MI355X (gfx950) kernels of the reference's shaking-duration comparison
 * (scripts/seismo_evaluations/arias_intensity_duration.ipynb: calculate_arias_intensity, calculate_signal_duration,
 * compute_time_derivative).  A fourth library next to libtqdne_hip.so (include/tqdne_hip.h), libtqdne_eval.so
 * (include/tqdne_eval.h) and libtqdne_series.so (include/tqdne_series.h), with the conventions of the third:
 *   - device pointers only (the fractions of tqd_arias excepted: a host pointer, read during the call and passed to the kernel by
 *     value), caller-owned memory, nothing allocated or synchronised inside;
 *   - all work is enqueued on the given HIP stream (graph-capture safe);
 *   - return 0 on success, a TQ_ERR_* code (negative) for bad arguments, or a hipError_t (>0) from the launch;
 *   - every argument is checked before the device is touched: a null pointer, a step or dt that is not positive and finite, a fraction
 *     outside [0, 1] or an output that overlaps an input return TQ_ERR_ARG; R < 1, T < 2, T > 2^30, a row stride below T or a number
 *     of fractions outside 1 ... tqd_max_fractions() return TQ_ERR_SHAPE;
 *   - no atomics, every sum in a fixed order that depends on T only.  Results are bit-reproducible, and a row's result does not depend
 *     on the rest of the batch.
 */
#ifndef TQDNE_DURATION_H
#define TQDNE_DURATION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define TQD_ABI_VERSION 1

#ifndef TQ_ERR_ARG
#define TQ_ERR_ARG (-1)   /* null / inconsistent pointer arguments */
#define TQ_ERR_SHAPE (-2) /* unsupported shape */
#endif

#define TQD_MAX_FRACTIONS 8

int tqd_abi_version(void);
int tqd_max_fractions(void);

/* ---- energy, peak, threshold crossings and (optionally) the Husid curve of R rows, one launch (csrc_duration/duration.hip) ----
 * R rows of T fp32 samples, row r at x + r * ldx and, when y is not null, a second component at y + r * ldy (ld >= T: the channel
 * views w[:, 0], w[:, 1] of one (N, 3, T) tensor go in as they are).  Per row, all in fp64:
 *     s[i]   = x[i]^2 (+ y[i]^2)          exact products of the widened samples, their sum rounded once
 *     cum[0] = 0,   cum[i] = cum[i-1] + 0.5 (s[i-1] + s[i]) step          (the cumulative trapezoid rule)
 * summed in the order of the kernel's mapping: with C = ceil(T / 64), chunk l holds the terms of the samples l C ... (l + 1) C - 1;
 * base[0] = 0, base[l+1] = base[l] + (chunk l's terms added in sample order from zero), and cum[i] = base[l] + (chunk l's terms up
 * to i added in sample order from zero).  The sequence is non-decreasing and cum at a chunk's last sample is the next chunk's base.
 *     energy[r]   = cum[T-1]                                             (double)
 *     peak2[r]    = max_i s[i]                                           (double, exact)
 *     index[r, j] = the first i in [0, T) with cum[i] >= fl(fractions[j] * cum[T-1])     (int32, R x n_fractions, dense)
 *     husid[r, i] = cum[i] / cum[T-1], rounded to fp32                   (fp32, R x T, dense; may be null: not written)
 * energy, husid and the crossings use one and the same sequence cum.  fractions: a HOST pointer to n_fractions doubles in [0, 1],
 * in any order.  A row of zero energy gives energy = 0, peak2 = 0, every index -1 and a NaN husid row; a row with a non-finite sample
 * gives energy = peak2 = NaN, every index -1 and a NaN husid row; other rows are untouched by either. */
int tqd_arias(const float* x, const float* y, double* energy, double* peak2, int32_t* index, float* husid, int R, int T, int64_t ldx,
              int64_t ldy, double step, const double* fractions, int n_fractions, hipStream_t s);

/* ---- numpy.gradient(x, dt, axis=-1) of fp32 rows in numpy's float32 arithmetic ------------------------------------------------
 * R rows of T >= 2 samples, input rows at x + r * ldx, output rows at g + r * ldg.  One IEEE rounding per operation, a true
 * division:  g[i] = (x[i+1] - x[i-1]) / fl32(2 dt) inside the row,  g[0] = (x[1] - x[0]) / dt,  g[T-1] = (x[T-1] - x[T-2]) / dt.
 * A non-finite sample propagates as in numpy (to its neighbours' results); there is no row flag.  g must not overlap x. */
int tqd_gradient(const float* x, float* g, int R, int T, int64_t ldx, int64_t ldg, float dt, hipStream_t s);

#ifdef __cplusplus
}
#endif
#endif /* TQDNE_DURATION_H */
