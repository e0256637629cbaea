// neighbourhood shrinkage (NeighShrink, ndwt_device_neigh.h): float and complex64 data, 1 to 3 filtered axes, radius 1 to 3
#include "ndwt_device_neigh.h"
#include "ndwt_fused_kernels.h"
namespace ndwt {
#define NDWT_LAUNCH_NEIGH(T, COMP, ND, R) \
    if (comp == COMP && nd == ND && r == R) return launch_select_k<NeighShrink<T, COMP, ND, R>>(a, (int)blocks, buf_dev, s);
#define NDWT_LAUNCH_NEIGH_R(T, COMP, ND) NDWT_LAUNCH_NEIGH(T, COMP, ND, 1) NDWT_LAUNCH_NEIGH(T, COMP, ND, 2) NDWT_LAUNCH_NEIGH(T, COMP, ND, 3)
int launch_neigh_shrink(const NeighArgs<float>& a, int comp, int nd, int r, const void* buf_dev, hipStream_t s) {
    long long blocks = 0;
    if (!neigh_launch_ok(a, comp, nd, r, &blocks)) return -2;
    NDWT_LAUNCH_NEIGH_R(float, 1, 1) NDWT_LAUNCH_NEIGH_R(float, 1, 2) NDWT_LAUNCH_NEIGH_R(float, 1, 3)
    NDWT_LAUNCH_NEIGH_R(float, 2, 1) NDWT_LAUNCH_NEIGH_R(float, 2, 2) NDWT_LAUNCH_NEIGH_R(float, 2, 3)
    return -1;
}
}  // namespace ndwt
