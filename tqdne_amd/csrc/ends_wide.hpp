// Entry points of ends_wide.hip: the stem and head convolutions at the first-level widths the kernels of small_ops.hip / backward.hip
// were not written for (32 | C <= 1024 that is not a power of two, or too wide for one workgroup's LDS).  The public launchers
// (tq_stem_conv_fwd, tq_head_conv_fwd, tq_head_conv_bwd_ws) call these exactly where they used to return TQ_ERR_SHAPE; a shape the
// old kernels take never gets here.  Every function checks its own shape and returns TQ_ERR_SHAPE for what it is not built for.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace tq {
// dynamic LDS bytes of the kernel that would run; 0 = not built for the shape.  Host only (no device needed).
size_t ends_wide_stem_lds(int C_in, int C_out, int ktaps);
size_t ends_wide_head_fwd_lds(int C_in, int C_out, int ktaps);
size_t ends_wide_head_bwd_lds(int C_in, int C_out, int ktaps);

int ends_wide_stem_fwd(const float* x, const float* in_scale, const float* w, const float* bias, float* y, float* stats, int B, int C_in,
                       int T, int C_out, int ktaps, hipStream_t stream);
int ends_wide_head_fwd(const float* x, const float* gscale, const float* gshift, const float* w, const float* bias, const float* c_out,
                       const float* c_skip, const float* skip_src, float* y, int B, int T, int C_in, int C_out, int ktaps,
                       hipStream_t stream);
int ends_wide_head_bwd(const float* dpred_nct, const float* c_out, const float* x, const float* gscale, const float* gshift,
                       const float* w, float* g_out, float* gstats, float* dw, float* db, int B, int T, int C_in, int C_out, int ktaps,
                       void* workspace, size_t ws_bytes, hipStream_t stream);
}  // namespace tq
