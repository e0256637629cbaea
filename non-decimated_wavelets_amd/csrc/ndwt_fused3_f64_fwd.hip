// fused 3-D fwd level, double; and the double entry of the launch layer
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f64_fwd(const Fused3Instance& k, const Fused3Args<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F64_FWD(NDWT_LAUNCH_F)
    return -1;
}

int launch3_f64_inv(const Fused3Instance& k, const Fused3Args<double>& a, const void* taps_dev, hipStream_t s);
int launch3_f64_long(const Fused3Instance& k, const Fused3Args<double>& a, const void* taps_dev, hipStream_t s);
int launch_fused3_pick(const Fused3Pick& k, const Fused3Args<double>& a, const void* taps_dev, hipStream_t s) {
    for (auto unit : {launch3_f64_fwd, launch3_f64_inv, launch3_f64_long}) {
        const int rc = unit(k, a, taps_dev, s);
        if (rc != -1) return rc;
    }
    return -1;
}
}  // namespace ndwt
