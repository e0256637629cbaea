// order statistics of a band (BandHist / BandPick, ndwt_device_select.h): float and complex64 data, and the pick step of both key widths
#include "ndwt_device_select.h"
#include "ndwt_fused_kernels.h"
namespace ndwt {
#define NDWT_LAUNCH_H(T, COMP, VEC, AGG) \
    if (comp == COMP && vec == VEC && agg == AGG) return launch_select_k<BandHist<T, COMP, VEC, AGG>>(a, a.nblocks, buf_dev, s);
int launch_band_hist(const BandHistArgs<float>& a, int comp, bool vec, int agg, const void* buf_dev, hipStream_t s) {
    NDWT_LAUNCH_H(float, 1, true, 2) NDWT_LAUNCH_H(float, 1, false, 2) NDWT_LAUNCH_H(float, 2, true, 2) NDWT_LAUNCH_H(float, 2, false, 2)
    NDWT_LAUNCH_H(float, 1, true, 0) NDWT_LAUNCH_H(float, 1, false, 0) NDWT_LAUNCH_H(float, 2, true, 0) NDWT_LAUNCH_H(float, 2, false, 0)
    return -1;
}
int launch_band_pick(bool f64, const BandPickArgs& a, const void* buf_dev, hipStream_t s) {
    return f64 ? launch_select_k<BandPick<double>>(a, 1, buf_dev, s) : launch_select_k<BandPick<float>>(a, 1, buf_dev, s);
}
}  // namespace ndwt
