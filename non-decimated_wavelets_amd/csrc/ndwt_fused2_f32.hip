// fused 2-D levels, float: analysis (Fwd2S) of 2 .. 6 taps; and the float entry of the launch layer: the units asked in turn
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch2_f32(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_2S_SHORT(NDWT_LAUNCH_W, Fwd2S)
    return -1;
}

int launch2_f32_fwdb(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch2_f32_fwdl(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch2_f32_fwdc(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch2_f32_inva(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch2_f32_invb(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch2_f32_invc(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch2_f32_invl(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch2_f32_invm(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch_inv2p_f32(const Fused2PInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch_fused2_pick(const Fused2Pick& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s) {
    if (k.family == kInv2P) return launch_inv2p_f32(k.inv2p(), a, taps_dev, s);
    const Fused2SInstance ks = k.fused2s();
    for (auto unit : {launch2_f32_fwdb, launch2_f32_invb, launch2_f32, launch2_f32_inva, launch2_f32_fwdl, launch2_f32_invl, launch2_f32_invm,
                      launch2_f32_fwdc, launch2_f32_invc}) {
        const int rc = unit(ks, a, taps_dev, s);
        if (rc != -1) return rc;
    }
    return -1;
}
}  // namespace ndwt
