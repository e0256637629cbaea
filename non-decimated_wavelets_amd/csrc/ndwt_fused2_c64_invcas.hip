// cascaded 2-D synthesis, interleaved complex64 (Inv2C, packed FMAs on (re, im) pairs), tap lengths 2 .. 8
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_cascade2_c64(const Cascade2Instance& k, const Fused2CIArgs<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_C64_INV2C(NDWT_LAUNCH_R)
    return -1;
}
}  // namespace ndwt
