// fused 3-D fwd level, float; and the float entry of the launch layer: the units asked in turn
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch3_f32_fwd(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_FWD(NDWT_LAUNCH_F)
    return -1;
}

int launch3_f32_fwdp(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch3_f32_inv(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch3_f32_inve(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch3_f32_invy(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch3_f32_invys(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch3_f32_invyc(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch3_f32_long(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch3_f32_longb(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch3_f32_longi(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch3_f32_den(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch_fused3_pick(const Fused3Pick& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    for (auto unit : {launch3_f32_invy, launch3_f32_invys, launch3_f32_fwd, launch3_f32_fwdp, launch3_f32_invyc, launch3_f32_long, launch3_f32_longb,
                      launch3_f32_inv, launch3_f32_inve, launch3_f32_longi, launch3_f32_den}) {
        const int rc = unit(k, a, taps_dev, s);
        if (rc != -1) return rc;
    }
    return -1;
}
}  // namespace ndwt
