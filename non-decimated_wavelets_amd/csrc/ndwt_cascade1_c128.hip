// cascaded 1-D analysis and synthesis of a batched plan (Fwd1C / Inv1C), complex128 data, tap lengths 2 .. 8, 2 .. 4 levels
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_cascade1_c128(const Cascade1Instance& k, const Fused1CArgs<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_C128_1C(NDWT_LAUNCH_C, Fwd1C) NDWT_LIST_C128_1C(NDWT_LAUNCH_C, Inv1C)
    return -1;
}
}  // namespace ndwt
