// one-launch denoise of a batched 1-D plan with a threshold row per signal (Den1C<.., ROWTHR = true>), double real data, tap lengths 2 .. 8, 1 .. 4 levels
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_den1r_c128(const Den1Instance& k, const Den1CArgs<double>& a, const void* taps_dev, hipStream_t s);
int launch_den1r(const Den1Instance& k, const Den1CArgs<double>& a, const void* taps_dev, hipStream_t s) {
    if (k.ew != 1) return launch_den1r_c128(k, a, taps_dev, s);
    NDWT_LIST_F64_DEN1R(NDWT_LAUNCH_DR)
    return -1;
}
}  // namespace ndwt
