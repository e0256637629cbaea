// fused 3-D levels, double real, 14 and 16 taps (db7, db8): 64x8 tiles with 512 threads and the 256-register budget.  18 and 20 taps spill
// 400+ registers in this form and stay on the per-axis path.
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f64_long(const Fused3Instance& k, const Fused3Args<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F64_LONG(NDWT_LAUNCH_F, NDWT_LAUNCH_S)
    return -1;
}
}  // namespace ndwt
