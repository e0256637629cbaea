// the per-item kernels (ItemSelect / ShrinkItems, ndwt_device_items.h): double and complex128 data
#include "ndwt_device_items.h"
#include "ndwt_fused_kernels.h"
namespace ndwt {
#define NDWT_LAUNCH_H(T, COMP, VEC) \
    if (comp == COMP && vec == VEC) return launch_select_k<ItemSelect<T, COMP, VEC>>(a, items, buf_dev, s);
int launch_item_select(const ItemSelectArgs<double>& a, int comp, bool vec, int items, const void* buf_dev, hipStream_t s) {
    NDWT_LAUNCH_H(double, 1, true) NDWT_LAUNCH_H(double, 1, false) NDWT_LAUNCH_H(double, 2, true) NDWT_LAUNCH_H(double, 2, false)
    return -1;
}
#undef NDWT_LAUNCH_H
#define NDWT_LAUNCH_H(T, COMP, VEC) \
    if (comp == COMP && vec == VEC) return launch_select_k<ShrinkItems<T, COMP, VEC>>(a, (int)(a.nbands * a.items * a.chunks), buf_dev, s);
int launch_shrink_items(const ShrinkItemsArgs<double>& a, int comp, bool vec, const void* buf_dev, hipStream_t s) {
    if (a.nbands < 1 || a.items < 1 || a.chunks < 1 || (long long)a.nbands * a.items * a.chunks > 0x7fffffffLL) return -2;
    NDWT_LAUNCH_H(double, 1, true) NDWT_LAUNCH_H(double, 1, false) NDWT_LAUNCH_H(double, 2, true) NDWT_LAUNCH_H(double, 2, false)
    return -1;
}
}  // namespace ndwt
