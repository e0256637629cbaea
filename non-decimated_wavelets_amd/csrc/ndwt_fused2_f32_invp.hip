// fused 2-D synthesis with rows of band loads in flight (Inv2P), float
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch_inv2p_f32(const Fused2PInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_INV2P(NDWT_LAUNCH_P)
    return -1;
}
}  // namespace ndwt
