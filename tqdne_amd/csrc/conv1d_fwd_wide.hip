// k = 5 forward launches of the fp16 + MX-fp6 scheme over MORE THAN 1024 concatenated input channels (the output blocks of UNets wider
// than the paper's: up to 1024 + 1024): the same tiles with a 2048-entry table of folded GroupNorm coefficients (GTW, conv1d_kernel.hpp),
// in a translation unit of their own so that every established kernel keeps its code object.  Also the width limits the host asks for.
#include "conv1d_kernel.hpp"

namespace {
// 256-channel tile (8 waves), 128-channel tile (4 waves), small tile (32 positions): what dispatch_tile picks for these shapes
template <int KT, int ACT, bool FUSE>
int dispatch_wide(const ConvArgs& a, hipStream_t s) {
    if (a.wfmt != TQ_WFMT_F16_MX6 || (a.flags & TQ_CONV_POLY2)) return TQ_ERR_SHAPE;
    if (a.C0 % 64 || a.C1 % 64 || a.sC0 % 64 || a.sC1 % 64 || a.C_out % 128) return TQ_ERR_SHAPE;
    if (a.t_tile == 32) {
        if constexpr (KT == 5 && ACT >= 2) return launch<KT, 1, 0, 4, 1, 0, ACT, FUSE, 2, false, 2, 2, CONV_GTAB_WIDE>(a, s);
        return TQ_ERR_SHAPE;
    }
    if (a.C_out % 256 == 0) return launch<KT, 1, 0, 8, 1, 0, ACT, FUSE, 2, false, 8, 2, CONV_GTAB_WIDE>(a, s);
    return launch<KT, 1, 0, 4, 1, 0, ACT, FUSE, 2, false, 8, 2, CONV_GTAB_WIDE>(a, s);
}
}  // namespace

namespace tq {
int conv_launch_fwd_wide_k5(const ConvArgs& a, int act, bool fuse, hipStream_t s) {
    if (fuse) {
        if (act == 3) return dispatch_wide<5, 3, true>(a, s);
        if (act == 2) return dispatch_wide<5, 2, true>(a, s);
        return TQ_ERR_SHAPE;
    }
    if (act == 3) return dispatch_wide<5, 3, false>(a, s);
    if (act == 2) return dispatch_wide<5, 2, false>(a, s);
    if (act == 1) return dispatch_wide<5, 1, false>(a, s);
    return TQ_ERR_SHAPE;
}

int conv_launch_fwd_wide(const ConvArgs& a, int ktaps, int act, bool fuse, hipStream_t s) {
    if (ktaps == 5) return conv_launch_fwd_wide_k5(a, act, fuse, s);
    if (fuse) return TQ_ERR_SHAPE;
    return conv_launch_fwd_wide_k13(a, ktaps, act, s);
}
}  // namespace tq

extern "C" int tq_conv1d_max_cin(int wfmt, int C_out) {
    if (C_out < 0 || C_out % 32) return 0;
    switch (wfmt) {
        case TQ_WFMT_F16_MX6:   // wide-table tiles: 128 | C_out; the 64-channel tile has the 1024-entry table only
            return (C_out % 128 == 0) ? CONV_GTAB_WIDE : (C_out % 64 == 0 ? CONV_GTAB_NARROW : 0);
        case TQ_WFMT_F16_MX8: return (C_out % 128 == 0) ? CONV_GTAB_NARROW : 0;
        case TQ_WFMT_BF16X3: return CONV_GTAB_WIDE;   // (no table: the widest concatenation the suite covers)
        default: return 0;
    }
}

// dynamic LDS of the wide-table tile a launch would take (0: no such tile); the prologue and the fused skip conv do not change it
template <int KT>
static size_t wide_lds(int t_tile, int C_out) {
    if (C_out <= 0 || C_out % 128) return 0;
    if (t_tile == 32) return KT == 5 ? (size_t)ConvLds<KT, 1, 0, 4, 1, 0, 2, 2, false, 2, 2, CONV_GTAB_WIDE>::BYTES : 0;
    if (t_tile) return 0;
    return C_out % 256 == 0 ? (size_t)ConvLds<KT, 1, 0, 8, 1, 0, 2, 2, false, 8, 2, CONV_GTAB_WIDE>::BYTES
                            : (size_t)ConvLds<KT, 1, 0, 4, 1, 0, 2, 2, false, 8, 2, CONV_GTAB_WIDE>::BYTES;
}
extern "C" size_t tq_conv1d_wide_lds_bytes(int ktaps, int t_tile, int C_out) {
    return ktaps == 5 ? wide_lds<5>(t_tile, C_out) : ktaps == 3 ? wide_lds<3>(t_tile, C_out) : ktaps == 1 ? wide_lds<1>(t_tile, C_out) : 0;
}

extern "C" int tq_conv1d_gn_table_entries(int wide) { return wide ? CONV_GTAB_WIDE : CONV_GTAB_NARROW; }

extern "C" int tq_conv1d_max_cout(void) { return 3 * CONV_GTAB_NARROW; }   // (the qkv projection of a 1024-channel attention block)

extern "C" int tq_conv1d_gn_fold_max_cin(int wfmt, int t_tile, int C_out) {
    // k = 5, GN + SiLU: the launches the fold is built into (dispatch_tile); the limits are those of launch()
    if (C_out <= 0 || C_out % 32) return 0;
    int lim = 0;
    if (t_tile == 32) {
        if (wfmt == TQ_WFMT_F16_MX6) lim = C_out % 128 ? 0 : ConvLds<5, 1, 0, 4, 1, 0, 2, 2, false, 2, 2, 1024>::FOLD_MAX_CIN;
        else if (wfmt != TQ_WFMT_BF16X3) lim = 0;
        else if (C_out % 128 == 0) lim = ConvLds<5, 1, 0, 4, 1, 0, 2, 0, false, 2, 2, 1024>::FOLD_MAX_CIN;
        else if (C_out % 64 == 0) lim = ConvLds<5, 1, 0, 2, 1, 0, 2, 0, false, 2, 2, 1024>::FOLD_MAX_CIN;
        else lim = ConvLds<5, 1, 0, 1, 1, 0, 2, 0, false, 2, 2, 1024>::FOLD_MAX_CIN;
    } else if (t_tile == 0 && wfmt == TQ_WFMT_F16_MX6) {   // (default tiles: the fp16 + MX-fp6 ones only)
        if (C_out % 256 == 0) lim = ConvLds<5, 1, 0, 8, 1, 0, 2, 2, false, 8, 2, 1024>::FOLD_MAX_CIN;
        else if (C_out % 128 == 0) lim = ConvLds<5, 1, 0, 4, 1, 0, 2, 2, false, 8, 2, 1024>::FOLD_MAX_CIN;
    }
    return lim / 32 * 32;   // GroupNorm32 over whole groups of a 32-channel multiple
}
