// one-launch denoise of a batched 1-D plan with a threshold row per signal (Den1C<.., ROWTHR = true>), complex64 data
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_den1r_c64(const Den1Instance& k, const Den1CArgs<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_C64_DEN1R(NDWT_LAUNCH_DR)
    return -1;
}
}  // namespace ndwt
