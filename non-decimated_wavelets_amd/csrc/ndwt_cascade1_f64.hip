// cascaded 1-D analysis and synthesis of a batched plan (Fwd1C / Inv1C), double real data, tap lengths 2 .. 8, 2 .. 4 levels
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_cascade1_c128(const Cascade1Instance& k, const Fused1CArgs<double>& a, const void* taps_dev, hipStream_t s);
int launch_cascade1(const Cascade1Instance& k, const Fused1CArgs<double>& a, const void* taps_dev, hipStream_t s) {
    if (k.ew != 1) return launch_cascade1_c128(k, a, taps_dev, s);
    NDWT_LIST_F64_1C(NDWT_LAUNCH_C, Fwd1C) NDWT_LIST_F64_1C(NDWT_LAUNCH_C, Inv1C)
    return -1;
}
}  // namespace ndwt
