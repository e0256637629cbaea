// fused 3-D inv level, float, real undilated data: the lane-shift kernel Inv3S (what the pair-packed kernel does not cover) and the LDS kernel
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_inv(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_INV(NDWT_LAUNCH_S)
    return -1;
}
}  // namespace ndwt
