// k = 1 and k = 3 forward launches of the fp16 + MX-fp6 scheme over more than 1024 concatenated input channels (wide-table tiles, see
// conv1d_fwd_wide.hip): the ResBlock convs of models built with conv_kernel_size = 3, the Encoder / Decoder convs
#include "conv1d_kernel.hpp"

namespace {
template <int KT, int ACT>
int dispatch_wide13(const ConvArgs& a, hipStream_t s) {
    if (a.wfmt != TQ_WFMT_F16_MX6 || (a.flags & TQ_CONV_POLY2) || a.t_tile) return TQ_ERR_SHAPE;
    if (a.C0 % 64 || a.C1 % 64 || a.sC0 || a.sC1 || a.C_out % 128) return TQ_ERR_SHAPE;
    if (a.C_out % 256 == 0) return launch<KT, 1, 0, 8, 1, 0, ACT, false, 2, false, 8, 2, CONV_GTAB_WIDE>(a, s);
    return launch<KT, 1, 0, 4, 1, 0, ACT, false, 2, false, 8, 2, CONV_GTAB_WIDE>(a, s);
}
template <int KT>
int dispatch_wide13_act(const ConvArgs& a, int act, hipStream_t s) {
    if (act == 3) return dispatch_wide13<KT, 3>(a, s);
    if (act == 2) return dispatch_wide13<KT, 2>(a, s);
    if (act == 1) return dispatch_wide13<KT, 1>(a, s);
    return TQ_ERR_SHAPE;
}
}  // namespace

namespace tq {
int conv_launch_fwd_wide_k13(const ConvArgs& a, int ktaps, int act, hipStream_t s) {
    if (ktaps == 3) return dispatch_wide13_act<3>(a, act, s);
    if (ktaps == 1) return dispatch_wide13_act<1>(a, act, s);
    return TQ_ERR_SHAPE;
}
}  // namespace tq
