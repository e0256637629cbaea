// C entry points to denoise1_levels (csrc/ndwt_select.h) and the instance table of the one-launch denoise (csrc/ndwt_fused_list.h) for
// tests/test_denoise1_select.py (host C++ only: g++ -std=c++17 -Wall -Wextra -Werror -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

// v: ndim, comp, f64, real, path_auto, atrous, fp64_fused, dims[4], len[4], variant_fwd, variant_inv (as tests/select/select_shim.cpp)
static SelPlan plan_of(const int* v) {
    SelPlan p = {v[0], v[1], v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, {v[7], v[8], v[9], v[10]}, {v[11], v[12], v[13], v[14]}, v[15], v[16]};
    return p;
}

// levels the one launch takes (0: the general route); inner: elements of a sample that lie together (1: not interleaved)
extern "C" int sel_denoise1_levels(const int* plan, long long howmany, long long inner, int level) {
    SelPlan p = plan_of(plan);
    p.howmany = howmany;
    p.inner = inner;
    return denoise1_levels(p, level);
}
// dims[0] as a 64-bit number (rows of 2^30 scalars and beyond)
extern "C" int sel_denoise1_levels_n(const int* plan, long long n, long long howmany, int level) {
    SelPlan p = plan_of(plan);
    p.dims[0] = n;
    p.howmany = howmany;
    return denoise1_levels(p, level);
}
// the launch is taken unasked (the data kind's default) or was asked for (variant 11 / 11)
extern "C" int sel_denoise1_wanted(const int* plan) { return denoise1_wanted(plan_of(plan)); }
extern "C" int sel_denoise1_default(int f64, int comp) { return denoise1_default(f64 != 0, comp); }
extern "C" int sel_den1_listed(int f64, int ew, int Lp, int nlev) { return den1_instantiated({f64 != 0, ew, Lp, nlev}); }
extern "C" int sel_den1_tile_width(int Lp, int ew, int f64, int nlev) { return den1_tile_width(Lp, ew, f64 != 0, nlev); }
