// fused 2-D levels, double: analysis (Fwd2S), the rows-in-flight synthesis (Inv2P) and the double entry of the launch layer; Inv2S: ndwt_fused2_f64_inv.hip
#include "ndwt_fused_kernels.h"
namespace ndwt {
static int launch_fwd2_f64(const Fused2Args<double>& a, int Lp, bool vec4, int ew, const void* taps_dev, hipStream_t s) {
    if (Lp > 6) { NDWT_FUSED2_SWITCH_LONG(Fwd2S, double) }
    NDWT_FUSED2_SWITCH_SHORT(Fwd2S, double)
}
int launch_inv2_f64(const Fused2Args<double>& a, int Lp, bool vec4, int ew, const void* taps_dev, hipStream_t s);
int launch_long2_f64(bool inverse, const Fused2Args<double>& a, int Lp, bool vec4, const void* taps_dev, hipStream_t s);   // double real, db7 / db8
static int launch_inv2p_f64(const Fused2PInstance& k, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F64_INV2P(NDWT_LAUNCH_P)
    return -1;
}
// the double entry of the launch layer
int launch_fused2_pick(const Fused2Pick& k, const Fused2Query& q, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s) {
    if (k.family == kInv2P) return launch_inv2p_f64({true, q.Lp, k.pdepth, k.packed != 0}, a, taps_dev, s);
    if (q.Lp > 12) return q.ew != 1 ? -1 : launch_long2_f64(q.inverse, a, q.Lp, q.vec4, taps_dev, s);
    return q.inverse ? launch_inv2_f64(a, q.Lp, q.vec4, q.ew, taps_dev, s) : launch_fwd2_f64(a, q.Lp, q.vec4, q.ew, taps_dev, s);
}
}  // namespace ndwt
