// one-launch denoise of a batched 1-D plan with a threshold row per signal (Den1C<.., ROWTHR = true>), complex128 data (the table: ndwt_fused_list.h)
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_den1r_c128(const Den1Instance& k, const Den1CArgs<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_C128_DEN1R(NDWT_LAUNCH_DR)
    return -1;
}
}  // namespace ndwt
