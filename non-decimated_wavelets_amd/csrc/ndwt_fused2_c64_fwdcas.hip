// cascaded 2-D analysis, interleaved complex64 (Fwd2C with the x taps stepping over the (re, im) pairs), tap lengths 2 .. 8
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_cascade2_c64(const Cascade2Instance& k, const Fused2CArgs<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_C64_FWD2C(NDWT_LAUNCH_A)
    return -1;
}
}  // namespace ndwt
