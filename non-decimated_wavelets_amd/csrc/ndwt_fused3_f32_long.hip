// fused 3-D analysis, float, 14 / 16 taps (db7, db8) on the tall 64x32 tile.  The 512-thread instances of 14 .. 20 taps are in
// ndwt_fused3_f32_longb.hip, the lane-shift synthesis (14 / 16 taps: the fallback of the pair-packed kernel for mixed wavelets with odd tap
// padding) in ndwt_fused3_f32_longi.hip.
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_long(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_LONG(NDWT_LAUNCH_F)
    return -1;
}
}  // namespace ndwt
