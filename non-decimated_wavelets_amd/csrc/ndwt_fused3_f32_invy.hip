// fused 3-D inv level, float, real data, stride 1: the pair-packed lane-shift kernel (Inv3Y), tap lengths 2..20
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_invy(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_INVY(NDWT_LAUNCH_Y)
    return -1;
}
}  // namespace ndwt
