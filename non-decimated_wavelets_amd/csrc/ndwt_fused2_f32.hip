// fused 2-D levels, float: analysis (Fwd2S), and the float entry of the launch layer, which routes to the units by x step and tap length
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_fwd2_f32_long(const Fused2Args<float>& a, int Lp, bool vec4, int ew, const void* taps_dev, hipStream_t s);
int launch_inv2_f32_short(const Fused2Args<float>& a, int Lp, bool vec4, int ew, const void* taps_dev, hipStream_t s);
int launch_inv2_f32_long(const Fused2Args<float>& a, int Lp, bool vec4, int ew, const void* taps_dev, hipStream_t s);
int launch_inv2p_f32(const Fused2PInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch_fwd2_f32_14to20(const Fused2Args<float>& a, int Lp, bool vec4, const void* taps_dev, hipStream_t s);   // float real, db7 .. db10
int launch_inv2_f32_14to20(const Fused2Args<float>& a, int Lp, bool vec4, const void* taps_dev, hipStream_t s);
int launch_fwd2_c64_10to16(const Fused2Args<float>& a, int Lp, bool vec4, const void* taps_dev, hipStream_t s);   // interleaved complex64, db5 .. db8
int launch_inv2_c64_10to16(const Fused2Args<float>& a, int Lp, bool vec4, const void* taps_dev, hipStream_t s);
static int launch_fwd2_f32(const Fused2Args<float>& a, int Lp, bool vec4, int ew, const void* taps_dev, hipStream_t s) {
    if (Lp > 6) return launch_fwd2_f32_long(a, Lp, vec4, ew, taps_dev, s);
    NDWT_FUSED2_SWITCH_SHORT(Fwd2S, float)
}
static int launch_inv2_f32(const Fused2Args<float>& a, int Lp, bool vec4, int ew, const void* taps_dev, hipStream_t s) {
    return Lp > 6 ? launch_inv2_f32_long(a, Lp, vec4, ew, taps_dev, s) : launch_inv2_f32_short(a, Lp, vec4, ew, taps_dev, s);
}
int launch_fused2_pick(const Fused2Pick& k, const Fused2Query& q, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s) {
    const int Lp = q.Lp, ew = q.ew;
    if (k.family == kInv2P) return launch_inv2p_f32({false, Lp, k.pdepth, k.packed != 0}, a, taps_dev, s);
    if (ew == 2 && Lp > 8) return q.inverse ? launch_inv2_c64_10to16(a, Lp, q.vec4, taps_dev, s) : launch_fwd2_c64_10to16(a, Lp, q.vec4, taps_dev, s);
    if (Lp > 12) return ew != 1 ? -1 : (q.inverse ? launch_inv2_f32_14to20(a, Lp, q.vec4, taps_dev, s) : launch_fwd2_f32_14to20(a, Lp, q.vec4, taps_dev, s));
    return q.inverse ? launch_inv2_f32(a, Lp, q.vec4, ew, taps_dev, s) : launch_fwd2_f32(a, Lp, q.vec4, ew, taps_dev, s);
}
}  // namespace ndwt
