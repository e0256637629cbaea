// fused 3-D inv level, float, stride 1: the pair-packed lane-shift kernel on interleaved complex data (Inv3Y, EW = 2, tap lengths 2..16)
// and on a level dilated by 4 (EW = 4), both also with the x stage in scatter form
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_invyc(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_INVYC(NDWT_LAUNCH_Y)
    return -1;
}
}  // namespace ndwt
