// C entry points to cascade1_levels (csrc/ndwt_select.h) and the 1-D cascade's instance table (csrc/ndwt_fused_list.h) for
// tests/test_batch1d_select.py (host C++ only: g++ -std=c++17 -Wall -Wextra -Werror -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

// v: ndim, comp, f64, real, path_auto, atrous, fp64_fused, dims[4], len[4], variant_fwd, variant_inv (as tests/select/select_shim.cpp)
static SelPlan plan_of(const int* v) {
    SelPlan p = {v[0], v[1], v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, {v[7], v[8], v[9], v[10]}, {v[11], v[12], v[13], v[14]}, v[15], v[16]};
    return p;
}

// levels the next launch takes (0: one launch per level); *L: the tap length it answered for
extern "C" int sel_cascade1_levels(const int* plan, long long howmany, int inverse, int left, int* L) {
    *L = 0;
    SelPlan p = plan_of(plan);
    p.howmany = howmany;
    return cascade1_levels(p, inverse != 0, left, L);
}
// dims[0] as a 64-bit number (rows of 2^30 scalars and beyond)
extern "C" int sel_cascade1_levels_n(const int* plan, long long n, long long howmany, int inverse, int left) {
    SelPlan p = plan_of(plan);
    p.dims[0] = n;
    p.howmany = howmany;
    int L = 0;
    return cascade1_levels(p, inverse != 0, left, &L);
}
// the route of the next launch of the level walk (cascade_route): its CascadeKind; *nlev: the levels it takes (0: one launch for one level)
extern "C" int sel_cascade_route(const int* plan, long long howmany, int inverse, int left, int* nlev) {
    SelPlan p = plan_of(plan);
    p.howmany = howmany;
    const CascadeRoute r = cascade_route(p, inverse != 0, left);
    *nlev = r.nlev;
    return (int)r.kind;
}
extern "C" int sel_cascade1_listed(int inverse, int f64, int ew, int Lp, int nlev) { return cascade1_instantiated({inverse != 0, f64 != 0, ew, Lp, nlev}); }
extern "C" int sel_cascade1_tile_width(int inverse, int f64, int ew, int Lp, int nlev) { return cascade1_tile_width({inverse != 0, f64 != 0, ew, Lp, nlev}); }
