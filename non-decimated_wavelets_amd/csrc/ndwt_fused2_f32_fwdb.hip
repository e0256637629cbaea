// fused 2-D analysis (Fwd2S), float, 8 .. 12 taps
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch2_f32_fwdb(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_2S_MID(NDWT_LAUNCH_W, Fwd2S)
    return -1;
}
}  // namespace ndwt
