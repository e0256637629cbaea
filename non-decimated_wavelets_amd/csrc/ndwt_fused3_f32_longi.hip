// fused 3-D synthesis, float, 14 / 16 taps: the lane-shift kernel on the 64x32 tile with 512 threads x 2 items (mixed wavelets with odd tap
// padding, which the pair-packed kernel does not take)
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_longi(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_LONGI(NDWT_LAUNCH_S)
    return -1;
}
}  // namespace ndwt
