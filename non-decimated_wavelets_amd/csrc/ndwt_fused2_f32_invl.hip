// fused 2-D synthesis (Inv2S), float real data, 14 / 16 taps (db7, db8; 18 / 20 taps: ndwt_fused2_f32_invm.hip)
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch2_f32_invl(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_2S_14_16(NDWT_LAUNCH_W, Inv2S)
    return -1;
}
}  // namespace ndwt
