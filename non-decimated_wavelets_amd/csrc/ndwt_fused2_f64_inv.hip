// fused 2-D synthesis (Inv2S), double, 2 .. 12 taps
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch2_f64_inv(const Fused2SInstance& k, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F64_2S(NDWT_LAUNCH_W, Inv2S)
    return -1;
}
}  // namespace ndwt
