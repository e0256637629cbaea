// C entry points to the host-side decisions of the per-item calls (csrc/ndwt_select.h: select_items_route, shrink_items_chunks and the
// constant the route is written in) for tests/test_items_select.py and tests/test_gpu_items.py
// (host C++ only: g++ -std=c++17 -Wall -Wextra -Werror -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

// 1: every item in one launch (ItemSelect), 0: the band-wide passes once per item
extern "C" int sel_items_one_launch(long long item_scalars, long long items, int num_cus, int variant_inv) {
    return select_items_route(item_scalars, items, num_cus, variant_inv) == kItemsOneLaunch;
}
// which: 0 the item count from which items of up to (1) scalars take the one launch unasked, 2 / 3 the same for the larger items, 4 the
// largest item that takes it from num_cus items on
extern "C" long long sel_items_route_const(int which) {
    return which == 0 ? kItemsFewFrom : which == 1 ? kItemsOneLaunchMaxScalars : which == 2 ? kItemsManyFrom : which == 3 ? kItemsOneLaunchMaxScalarsMany : kItemsOneLaunchMaxScalarsFull;
}
// the one-launch denoise: the instance with a threshold row per signal exists / the uniform one does (ndwt_fused_list.h)
extern "C" int sel_den1r_listed(int f64, int ew, int Lp, int nlev) { return den1r_instantiated({f64 != 0, ew, Lp, nlev}); }
extern "C" int sel_den1_listed_too(int f64, int ew, int Lp, int nlev) { return den1_instantiated({f64 != 0, ew, Lp, nlev}); }
extern "C" long long sel_shrink_items_chunks(long long item_scalars, int comp, int vec, long long bands, long long items, int num_cus) {
    return shrink_items_chunks(item_scalars, comp, vec != 0, bands, items, num_cus);
}
