// the SURE statistics (BandRisk, ndwt_device_risk.h): float and complex64 data
#include "ndwt_device_risk.h"
#include "ndwt_fused_kernels.h"
namespace ndwt {
#define NDWT_LAUNCH_H(T, COMP, VEC) \
    if (comp == COMP && vec == VEC) return launch_select_k<BandRisk<T, COMP, VEC>>(a, (int)(a.nbands * a.items * a.chunks), buf_dev, s);
int launch_band_risk(const BandRiskArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s) {
    if (a.nbands < 1 || a.items < 1 || a.chunks < 1 || (long long)a.nbands * a.items * a.chunks > 0x7fffffffLL) return -2;
    if (a.nc < 1 || a.nc > kRiskMaxCand) return -2;
    NDWT_LAUNCH_H(float, 1, true) NDWT_LAUNCH_H(float, 1, false) NDWT_LAUNCH_H(float, 2, true) NDWT_LAUNCH_H(float, 2, false)
    return -1;
}
}  // namespace ndwt
