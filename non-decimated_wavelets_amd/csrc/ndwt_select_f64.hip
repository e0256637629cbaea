// order statistics of a band (BandHist, ndwt_device_select.h): double and complex128 data
#include "ndwt_device_select.h"
#include "ndwt_fused_kernels.h"
namespace ndwt {
#define NDWT_LAUNCH_H(T, COMP, VEC, AGG) \
    if (comp == COMP && vec == VEC && agg == AGG) return launch_select_k<BandHist<T, COMP, VEC, AGG>>(a, a.nblocks, buf_dev, s);
int launch_band_hist(const BandHistArgs<double>& a, int comp, bool vec, int agg, const void* buf_dev, hipStream_t s) {
    NDWT_LAUNCH_H(double, 1, true, 2) NDWT_LAUNCH_H(double, 1, false, 2) NDWT_LAUNCH_H(double, 2, true, 2) NDWT_LAUNCH_H(double, 2, false, 2)
    NDWT_LAUNCH_H(double, 1, true, 0) NDWT_LAUNCH_H(double, 1, false, 0) NDWT_LAUNCH_H(double, 2, true, 0) NDWT_LAUNCH_H(double, 2, false, 0)
    return -1;
}
}  // namespace ndwt
