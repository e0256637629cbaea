// cascaded 2-D synthesis, double real data (Inv2C with scalar FMAs), tap lengths 2 .. 8
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_cascade2_c128(const Cascade2Instance& k, const Fused2CIArgs<double>& a, const void* taps_dev, hipStream_t s);   // complex128
int launch_cascade2(const Cascade2Instance& k, const Fused2CIArgs<double>& a, const void* taps_dev, hipStream_t s) {
    if (k.ew != 1) return launch_cascade2_c128(k, a, taps_dev, s);
    NDWT_LIST_F64_INV2C(NDWT_LAUNCH_R)
    return -1;
}
}  // namespace ndwt
