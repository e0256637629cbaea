// all levels of one strided axis inside one march (ndwt_device_axis.h: FwdMC / InvMC), float (and interleaved complex64: the factor 2
// in the inner block)
#include "ndwt_fused_kernels.h"

namespace ndwt {

int launch_cascadem(const CascadeMInstance& k, const MarchCArgs<float>& a, const double* lo, const double* hi, hipStream_t s) {
    NDWT_LIST_F32_FWDMC(NDWT_LAUNCH_M) NDWT_LIST_F32_INVMC(NDWT_LAUNCH_M)
    return -1;
}

}  // namespace ndwt
