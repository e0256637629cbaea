// C entry points to csrc/ndwt_select.h for tests/test_interleaved_select.py (host C++ only: g++ -std=c++17 -shared -fPIC): the selectors
// as a plan over interleaved samples (ndwt_plan_create_interleaved) asks them -- a SelPlan with its item count and its `inner`.
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

// v: ndim, comp, f64, real, path_auto, atrous, fp64_fused, dims[4], len[4], variant_fwd, variant_inv (one ITEM); howmany: the items,
// 0 = an unbatched plan; inner: elements of a sample
static SelPlan plan_of(const int* v, long long howmany, long long inner) {
    SelPlan p = {v[0], v[1], v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, {v[7], v[8], v[9], v[10]}, {v[11], v[12], v[13], v[14]}, v[15], v[16]};
    p.howmany = howmany;
    p.inner = inner;
    return p;
}

extern "C" int il_default_inner() {                      // a SelPlan written the positional way has inner = 1
    const SelPlan p = {1, 1, false, true, true, false, true, {64, 1, 1, 1}, {4, 2, 2, 2}, 0, 0};
    const SelPlan q = {1, 1, false, true, true, false, true, {64, 1, 1, 1}, {4, 2, 2, 2}, 0, 0, 3};
    return (int)p.inner * 10 + (int)q.inner + (q.howmany == 3 ? 100 : 0);
}

extern "C" int il_level_route(const int* plan, long long howmany, long long inner, int stride, int dir, int slab, int* Lp) {
    const LevelRoute r = level_route(plan_of(plan, howmany, inner), stride, dir, (SlabMode)slab);
    *Lp = r.Lp;
    return (int)r.kind;
}
extern "C" int il_cascade1_levels(const int* plan, long long howmany, long long inner, int inverse, int left, int* L) {
    *L = 0;
    return cascade1_levels(plan_of(plan, howmany, inner), inverse != 0, left, L);
}
extern "C" int il_cascade2_levels(const int* plan, long long howmany, long long inner, int inverse, int left, int* Lp) {
    *Lp = 0;
    return cascade2_levels(plan_of(plan, howmany, inner), inverse != 0, left, Lp);
}
extern "C" int il_shrink_capable(const int* plan, long long howmany, long long inner) { return fused_shrink_capable(plan_of(plan, howmany, inner)); }

// levels the next launch of the cascaded march takes (0: one launch per level); *L: its tap length; *listed: the instance table holds the pick
extern "C" int il_cascadem_levels(const int* plan, long long howmany, long long inner, int inverse, int left, int* L, int* listed) {
    *L = 0;
    const SelPlan p = plan_of(plan, howmany, inner);
    const int n = cascadem_levels(p, inverse != 0, left, L);
    *listed = n ? cascadem_instantiated({inverse != 0, p.f64, *L, n}) : 0;
    return n;
}
extern "C" int il_cascadem_instantiated(int inverse, int f64, int L, int nlev) { return cascadem_instantiated({inverse != 0, f64 != 0, L, nlev}); }
// whether the cascade is taken unasked: data kind, direction, bytes of the whole array; and the threshold itself (LLONG_MAX: never)
extern "C" int il_cascadem_default(int f64, int comp, int inverse, long long bytes) { return cascadem_default(f64 != 0, comp, inverse != 0, bytes); }
extern "C" long long il_cascadem_min_bytes(int f64, int comp, int inverse) { return cascadem_min_bytes(f64 != 0, comp, inverse != 0); }
