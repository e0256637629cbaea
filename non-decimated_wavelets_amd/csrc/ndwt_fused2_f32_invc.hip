// fused 2-D synthesis (Inv2S), interleaved complex64 data, 10 .. 16 taps (db5 .. db8)
#include "ndwt_fused_kernels.h"
namespace ndwt {
int launch2_f32_invc(const Fused2SInstance& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_C64_2S_LONG(NDWT_LAUNCH_W, Inv2S)
    return -1;
}
}  // namespace ndwt
