// all levels of one strided axis inside one march (ndwt_device_axis.h: FwdMC / InvMC), double (and interleaved complex128: the factor 2
// in the inner block)
#include "ndwt_fused_kernels.h"

namespace ndwt {

int launch_cascadem(const CascadeMInstance& k, const MarchCArgs<double>& a, const double* lo, const double* hi, hipStream_t s) {
    NDWT_LIST_F64_FWDMC(NDWT_LAUNCH_M) NDWT_LIST_F64_INVMC(NDWT_LAUNCH_M)
    return -1;
}

}  // namespace ndwt
