// cascaded 2-D analysis, float real data: two or three levels of an image in one launch (Fwd2C), tap lengths 2 .. 8 and 12
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_cascade2_c64(const Cascade2Instance& k, const Fused2CArgs<float>& a, const void* taps_dev, hipStream_t s);   // interleaved complex64
int launch_cascade2(const Cascade2Instance& k, const Fused2CArgs<float>& a, const void* taps_dev, hipStream_t s) {
    if (k.ew != 1) return launch_cascade2_c64(k, a, taps_dev, s);
    NDWT_LIST_F32_FWD2C(NDWT_LAUNCH_A)
    return -1;
}
}  // namespace ndwt
