// fused 2-D synthesis (Inv2S), float, 2 .. 6 taps
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch2_f32_inva(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_2S_SHORT(NDWT_LAUNCH_W, Inv2S)
    return -1;
}
}  // namespace ndwt
