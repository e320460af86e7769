// Attention for every head size d with 8 | d and 8 <= d <= 256: the first-generation kernels (attention_g1.hpp) instantiated with PAD = true
// on the smallest tile DT in {32, 64, 128, 256} with DT >= d, the channels >= d zero-filled on load and skipped on store.  A translation
// unit of its own: the code objects of attention.hip (head sizes 32 / 64 / 128, the paper model) do not depend on anything here.
#include "attention_g1.hpp"

namespace {
int head_tile(int d) {
    if (d < 8 || d > 256 || (d & 7)) return 0;
    return d <= 32 ? 32 : d <= 64 ? 64 : d <= 128 ? 128 : 256;
}
}  // namespace

extern "C" int tq_attention_head_tile(int D) { return head_tile(D); }

extern "C" size_t tq_attention_hd_lds_bytes(int D, int pass) {
    const int DT = head_tile(D);
    if (!DT) return 0;
    if (pass == 0) return fwd_lds_bytes(DT);
    if (pass == 1) return dq_lds_bytes(DT);
    if (pass == 2) return dkv_lds_bytes(DT, dkv_queries(DT));
    return 0;
}

extern "C" size_t tq_attention_hd_workspace_bytes(int B, int T, int H, int D) {
    const int DT = head_tile(D);
    if (!DT || B <= 0 || T <= 0 || H <= 0) return 0;
    return (size_t)ATT_KSPLIT_MAX * B * H * T * (DT + 4) * sizeof(float);   // the partial rows of the key split
}

extern "C" int tq_attention_fwd_hd(const float* qkv, float* out, float* lse, void* workspace, int B, int T, int H, int D,
                                   hipStream_t stream) {
    if (!qkv || !out) return TQ_ERR_ARG;
    if (B <= 0 || T <= 0 || H <= 0) return TQ_ERR_SHAPE;
    switch (head_tile(D)) {
        case 32: return launch_fwd<32, true>(qkv, out, lse, workspace, B, T, H, D, stream);
        case 64: return launch_fwd<64, true>(qkv, out, lse, workspace, B, T, H, D, stream);
        case 128: return launch_fwd<128, true>(qkv, out, lse, workspace, B, T, H, D, stream);
        case 256: return launch_fwd<256, true>(qkv, out, lse, workspace, B, T, H, D, stream);
    }
    return TQ_ERR_SHAPE;
}

extern "C" int tq_attention_bwd_hd(const float* qkv, const float* out, const float* dout, const float* lse, float* delta,
                                   float* dqkv, void* workspace, int B, int T, int H, int D, hipStream_t stream) {
    (void)workspace;   // (reserved: these kernels take no scratch)
    if (!qkv || !out || !dout || !lse || !delta || !dqkv) return TQ_ERR_ARG;
    if (B <= 0 || T <= 0 || H <= 0) return TQ_ERR_SHAPE;
    switch (head_tile(D)) {
        case 32: return launch_bwd<32, true>(qkv, out, dout, lse, delta, dqkv, B, T, H, D, stream);
        case 64: return launch_bwd<64, true>(qkv, out, dout, lse, delta, dqkv, B, T, H, D, stream);
        case 128: return launch_bwd<128, true>(qkv, out, dout, lse, delta, dqkv, B, T, H, D, stream);
        case 256: return launch_bwd<256, true>(qkv, out, dout, lse, delta, dqkv, B, T, H, D, stream);
    }
    return TQ_ERR_SHAPE;
}
