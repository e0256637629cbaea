// fused 2-D analysis (Fwd2S), float real data, 14 .. 20 taps (db7 .. db10)
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch2_f32_fwdl(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_2S_14_16(NDWT_LAUNCH_W, Fwd2S) NDWT_LIST_F32_2S_18_20(NDWT_LAUNCH_W, Fwd2S)
    return -1;
}
}  // namespace ndwt
