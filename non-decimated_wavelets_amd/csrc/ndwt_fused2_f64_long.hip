// fused 2-D levels, double real data, 14 and 16 taps (db7, db8), both directions
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch2_f64_long(const Fused2SInstance& k, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F64_2S_LONG(NDWT_LAUNCH_W, Fwd2S) NDWT_LIST_F64_2S_LONG(NDWT_LAUNCH_W, Inv2S)
    return -1;
}
}  // namespace ndwt
