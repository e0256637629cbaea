// fused 2-D levels, double: analysis (Fwd2S) of 2 .. 12 taps, the rows-in-flight synthesis (Inv2P); and the double entry of the launch layer
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch2_f64(const Fused2SInstance& k, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F64_2S(NDWT_LAUNCH_W, Fwd2S)
    return -1;
}
static int launch_inv2p_f64(const Fused2PInstance& k, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F64_INV2P(NDWT_LAUNCH_P)
    return -1;
}

int launch2_f64_inv(const Fused2SInstance& k, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s);
int launch2_f64_long(const Fused2SInstance& k, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s);
int launch_fused2_pick(const Fused2Pick& k, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s) {
    if (k.family == kInv2P) return launch_inv2p_f64(k.inv2p(), a, taps_dev, s);
    const Fused2SInstance ks = k.fused2s();
    for (auto unit : {launch2_f64, launch2_f64_inv, launch2_f64_long}) {
        const int rc = unit(ks, a, taps_dev, s);
        if (rc != -1) return rc;
    }
    return -1;
}
}  // namespace ndwt
