// fused 3-D inv level, double
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f64_inv(const Fused3Instance& k, const Fused3Args<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F64_INV(NDWT_LAUNCH_S)
    return -1;
}
}  // namespace ndwt
