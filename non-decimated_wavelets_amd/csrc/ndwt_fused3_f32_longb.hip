// fused 3-D analysis, float, 14 .. 20 taps on the 512-thread 64x16 tile (256-register budget): the kernels of 18 / 20 taps, and of 14 / 16
// taps on request
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_longb(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_LONGB(NDWT_LAUNCH_F)
    return -1;
}
}  // namespace ndwt
