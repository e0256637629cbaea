// the tile form of the joint shrinkage and the group norms (JointTile / GroupNormsTile, ndwt_device_joint_tile.h): float and complex64 data
#include "ndwt_device_joint_tile.h"
#include "ndwt_fused_kernels.h"
namespace ndwt {
#define NDWT_LAUNCH_JT(T, COMP, VEC) \
    if (comp == COMP && vec == VEC) return launch_select_k<JointTile<T, COMP, VEC>>(a, a.nb * a.chunks, buf_dev, s);
#define NDWT_LAUNCH_GT(T, COMP, VEC) \
    if (comp == COMP && vec == VEC) return launch_select_k<GroupNormsTile<T, COMP, VEC>>(a, a.nb * a.chunks, buf_dev, s);
// the host's strips against the kernels' own, and a grid the launch can number
template <class A> static bool tile_grid_ok(const A& a, int comp, bool vec) {
    return (comp == 1 || comp == 2) && a.nb >= 1 && a.items >= 1 && a.n >= comp && a.chunks == joint_tile_strips(a.n, comp, vec) &&
           (long long)a.nb * a.chunks <= 0x7fffffffLL;
}
int launch_joint_tile(const JointShrinkArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s) {
    if (!tile_grid_ok(a, comp, vec)) return -2;
    NDWT_LAUNCH_JT(float, 1, true) NDWT_LAUNCH_JT(float, 1, false) NDWT_LAUNCH_JT(float, 2, true) NDWT_LAUNCH_JT(float, 2, false)
    return -1;
}
int launch_group_norms_tile(const GroupNormsArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s) {
    if (!tile_grid_ok(a, comp, vec)) return -2;
    NDWT_LAUNCH_GT(float, 1, true) NDWT_LAUNCH_GT(float, 1, false) NDWT_LAUNCH_GT(float, 2, true) NDWT_LAUNCH_GT(float, 2, false)
    return -1;
}
}  // namespace ndwt
