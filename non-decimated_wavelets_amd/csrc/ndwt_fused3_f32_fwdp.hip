// fused 3-D fwd level, float real, 10 / 12 / 14 taps: tall tile with y items of 2 rows, taps pinned in SGPRs (Fwd3 PIN)
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_fwdp(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_FWDP(NDWT_LAUNCH_F)
    return -1;
}
}  // namespace ndwt
