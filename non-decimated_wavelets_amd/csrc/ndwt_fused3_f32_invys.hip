// fused 3-D inv level, float, real data, stride 1: the pair-packed kernel with its x stage in SCATTER form (Inv3Y<..., XSC>):
// partial sums travel between lanes (v_add_f32_dpp) instead of samples (v_mov_b32_dpp)
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_invys(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_INVYS(NDWT_LAUNCH_Y)
    return -1;
}
}  // namespace ndwt
