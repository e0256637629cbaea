// C entry points to csrc/ndwt_select.h for tests/test_stack_select.py (host C++ only: g++ -std=c++17 -shared -fPIC): the selectors as a
// stack plan (ndwt_plan_create_axes) asks them -- a SelPlan with its item count, a Fused2Query with its batch count.
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

// v: ndim, comp, f64, real, path_auto, atrous, fp64_fused, dims[4], len[4], variant_fwd, variant_inv (one ITEM of the stack); howmany: its
// items, 0 = an unbatched plan
static SelPlan plan_of(const int* v, long long howmany) {
    SelPlan p = {v[0], v[1], v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, {v[7], v[8], v[9], v[10]}, {v[11], v[12], v[13], v[14]}, v[15], v[16]};
    p.howmany = howmany;
    return p;
}

extern "C" int stk_level_route(const int* plan, long long howmany, int stride, int dir, int slab, int* Lp) {
    const LevelRoute r = level_route(plan_of(plan, howmany), stride, dir, (SlabMode)slab);
    *Lp = r.Lp;
    return (int)r.kind;
}

extern "C" int stk_cascade2_levels(const int* plan, long long howmany, int inverse, int left, int* Lp) {
    *Lp = 0;
    return cascade2_levels(plan_of(plan, howmany), inverse != 0, left, Lp);
}

extern "C" int stk_shrink_capable(const int* plan, long long howmany) { return fused_shrink_capable(plan_of(plan, howmany)); }

// v: f64, inverse, vec4, Lp, ew, dil, n1, n2, variant_inv; nbatch: images of the launch
// out: family, inverse, f64, vec4, Lp, ew, WPE (Fwd2S / Inv2S) or pdepth (Inv2P), packed, waves, and whether the instance lists hold the pick
extern "C" void stk_fused2(const int* v, int nbatch, int* out) {
    Fused2Query q = {v[0] != 0, v[1] != 0, v[2] != 0, v[3], v[4], v[5], v[6], v[7], v[8]};
    q.nbatch = nbatch;
    const Fused2Pick k = fused2_select(q);
    const bool deep = k.family == kInv2P;
    const int r[10] = {(int)k.family, k.inverse, k.f64, k.vec4, k.Lp, k.ew, deep ? k.pdepth : k.wpe, k.packed, k.waves,
                       deep ? inv2p_instantiated(k.inv2p()) : fused2s_instantiated(k.fused2s())};
    for (int i = 0; i < 10; ++i) out[i] = r[i];
}
extern "C" int stk_fused2_tile_width(int inverse, int Lp, int ew) { return fused2_tile_width(inverse != 0, Lp, ew); }
// whether a stack takes the cascade unasked: data kind, direction, rows of an item, bytes of all items
extern "C" int stk_cascade2_stack_default(int f64, int comp, int inverse, long long n2, long long total_bytes) {
    return cascade2_stack_default(f64 != 0, comp, inverse != 0, n2, total_bytes);
}
