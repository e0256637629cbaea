// joint shrinkage across items and the group norms (JointShrink / GroupNorms, ndwt_device_joint.h): float and complex64 data
#include "ndwt_device_joint.h"
#include "ndwt_fused_kernels.h"
namespace ndwt {
#define NDWT_LAUNCH_J(T, COMP, VEC) \
    if (comp == COMP && vec == VEC) return reg ? launch_select_k<JointShrink<T, COMP, VEC, true>>(a, a.nb * a.chunks, buf_dev, s) \
                                               : launch_select_k<JointShrink<T, COMP, VEC, false>>(a, a.nb * a.chunks, buf_dev, s);
#define NDWT_LAUNCH_G(T, COMP, VEC) \
    if (comp == COMP && vec == VEC) return launch_select_k<GroupNorms<T, COMP, VEC>>(a, a.nb * a.chunks, buf_dev, s);
int launch_joint_shrink(const JointShrinkArgs<float>& a, int comp, bool vec, bool reg, const void* buf_dev, hipStream_t s) {
    if (a.nb < 1 || a.items < 1 || a.chunks < 1 || (long long)a.nb * a.chunks > 0x7fffffffLL || (reg && a.items > kJointReg)) return -2;
    NDWT_LAUNCH_J(float, 1, true) NDWT_LAUNCH_J(float, 1, false) NDWT_LAUNCH_J(float, 2, true) NDWT_LAUNCH_J(float, 2, false)
    return -1;
}
int launch_group_norms(const GroupNormsArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s) {
    if (a.nb < 1 || a.items < 1 || a.chunks < 1 || (long long)a.nb * a.chunks > 0x7fffffffLL) return -2;
    NDWT_LAUNCH_G(float, 1, true) NDWT_LAUNCH_G(float, 1, false) NDWT_LAUNCH_G(float, 2, true) NDWT_LAUNCH_G(float, 2, false)
    return -1;
}
}  // namespace ndwt
