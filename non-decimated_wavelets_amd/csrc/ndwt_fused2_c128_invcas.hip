// cascaded 2-D synthesis, interleaved complex128 (Inv2C with scalar FMAs, the x taps stepping over the (re, im) pairs), tap lengths 2 .. 8
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_cascade2_c128(const Cascade2Instance& k, const Fused2CIArgs<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_C128_INV2C(NDWT_LAUNCH_R)
    return -1;
}
}  // namespace ndwt
