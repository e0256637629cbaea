// one pass along one axis (ndwt_device.h): the register-window march of a strided axis (AxisMarch) and the contiguous axis of 1-D signals
// and interleaved complex arrays (AxisX).  axis_select (ndwt_select.h) names the instance; -1: not in the lists
#include "ndwt_fused_kernels.h"

namespace ndwt {

int launch_axis_march(const AxisMarchInstance& k, const MarchArgs<float>& a, const double* lo, const double* hi, hipStream_t s) {
    NDWT_LIST_F32_AXIS_MARCH(NDWT_LAUNCH_N)
    return -1;
}
int launch_axis_march(const AxisMarchInstance& k, const MarchArgs<double>& a, const double* lo, const double* hi, hipStream_t s) {
    NDWT_LIST_F64_AXIS_MARCH(NDWT_LAUNCH_N)
    return -1;
}
int launch_axisx(const AxisXInstance& k, const AxisXArgs<float>& a, const double* lo, const double* hi, hipStream_t s) {
    NDWT_LIST_F32_AXISX(NDWT_LAUNCH_X)
    return -1;
}
int launch_axisx(const AxisXInstance& k, const AxisXArgs<double>& a, const double* lo, const double* hi, hipStream_t s) {
    NDWT_LIST_F64_AXISX(NDWT_LAUNCH_X)
    return -1;
}

}  // namespace ndwt
