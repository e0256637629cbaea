// one-launch denoise of a batched 1-D plan (Den1C), interleaved complex64, tap lengths 2 .. 8, 1 .. 4 levels
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_den1_c64(const Den1Instance& k, const Den1CArgs<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_C64_DEN1(NDWT_LAUNCH_D)
    return -1;
}
}  // namespace ndwt
