// fused 3-D inv level, float, the lane-shift kernel Inv3S with the x taps stepping over 2 (interleaved complex, a level dilated by 2) or 4
// (a level dilated by 4) scalars
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_inve(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_INVE(NDWT_LAUNCH_S)
    return -1;
}
}  // namespace ndwt
