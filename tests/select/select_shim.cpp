// C entry points to csrc/ndwt_select.h for tests/test_dispatch_select.py (host C++ only: g++ -std=c++17 -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

static SelPlan plan_of(const int* v) {   // ndim, comp, f64, real, path_auto, atrous, fp64_fused, dims[4], len[4], variant_fwd, variant_inv
    SelPlan p = {v[0], v[1], v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, {v[7], v[8], v[9], v[10]}, {v[11], v[12], v[13], v[14]}, v[15], v[16]};
    return p;
}

// the route of a level at tap stride `stride` (dir: 0 analysis, 1 synthesis; slab: a SlabMode): its LevelRouteKind
extern "C" int sel_level_path(const int* plan, int stride, int dir, int slab, int* Lp) {
    const LevelRoute r = level_route(plan_of(plan), stride, dir, (SlabMode)slab);
    *Lp = r.Lp;
    return (int)r.kind;
}

extern "C" int sel_cascade2_levels(const int* plan, int inverse, int left) { int Lp = 0; return cascade2_levels(plan_of(plan), inverse != 0, left, &Lp); }

// The plan with `howmany` items and samples of `inner` elements, under every pair of the `nvar` variants, both directions and
// left = 1 .. nleft: what the three cascade predicates answer, each asked on its own, and what cascade_route makes of them.  out: 9 ints
// per case, variant_fwd slowest, then variant_inv, the direction, left -- (n, L) of cascade1_levels, of cascadem_levels, of
// cascade2_levels (L = 0 where n = 0), then cascade_route's kind, nlev, L
extern "C" void sel_cascade_routes(const int* plan, long long howmany, long long inner, const int* variants, int nvar, int nleft, int* out) {
    SelPlan p = plan_of(plan);
    p.howmany = howmany;
    p.inner = inner;
    for (int f = 0; f < nvar; ++f)
        for (int i = 0; i < nvar; ++i)
            for (int inverse = 0; inverse < 2; ++inverse)
                for (int left = 1; left <= nleft; ++left, out += 9) {
                    p.variant_fwd = variants[f];
                    p.variant_inv = variants[i];
                    int L[3] = {0, 0, 0};
                    const int n[3] = {cascade1_levels(p, inverse != 0, left, &L[0]), cascadem_levels(p, inverse != 0, left, &L[1]),
                                      cascade2_levels(p, inverse != 0, left, &L[2])};
                    for (int k = 0; k < 3; ++k) { out[2 * k] = n[k]; out[2 * k + 1] = n[k] ? L[k] : 0; }
                    const CascadeRoute r = cascade_route(p, inverse != 0, left);
                    out[6] = (int)r.kind; out[7] = r.nlev; out[8] = r.L;
                }
}

// v: f64, inverse, vec4, uniform_yz, tfold, Lp, len[3], ew, dil, n1, n2, nbatch, variant_fwd, variant_inv, num_cus, target_blocks
// out: the pick in full -- V, TX, TY, NT, RY, WPE, PIN, TPRE, WLDS, DEPTH, ZLDS, UNIYZ, XSC, per_cu, target, VEC4, EW, Lp, f64, and whether
// the instance lists (ndwt_fused_list.h) hold it;  returns the kernel's name as the launch trace spells it
extern "C" const char* sel_fused3(const int* v, int* out) {
    const Fused3Query q = {v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0, v[5], {v[6], v[7], v[8]}, v[9], v[10], v[11], v[12], v[13],
                           v[14], v[15], v[16], v[17]};
    const Fused3Pick k = fused3_select(q);
    const TileShape t = fused3_tile_shape(k.kernel, k.f64, k.V, k.Lp, k.ew);
    const int r[20] = {k.V, k.TX, k.TY, t.NT, t.RY, t.WPE, k.pin, k.tpre, k.wlds, k.depth, k.kernel == kInv3Y ? inv3y_zlds(k.Lp, k.depth, k.ew) : 0,
                       k.uniyz, k.scatter, k.per_cu, k.target, k.vec4, k.ew, k.Lp, k.f64, fused3_instantiated(k)};
    for (int i = 0; i < 20; ++i) out[i] = r[i];
    switch (k.kernel) {
        case kFwd3: return "Fwd3";
        case kInv3Y: return "Inv3Y";
        case kInv3S: return "Inv3S";
        case kInv3: return "Inv3";
        default: return "none";
    }
}

// v: f64, inverse, vec4, Lp, ew, dil, n1, n2, variant_inv
// out: the pick in full -- family, inverse, f64, vec4, Lp, ew, WPE (Fwd2S / Inv2S) or pdepth (Inv2P), packed (Inv2P), waves, and whether
// the instance lists (ndwt_fused_list.h) hold it
extern "C" void sel_fused2(const int* v, int* out) {
    const Fused2Query q = {v[0] != 0, v[1] != 0, v[2] != 0, v[3], v[4], v[5], v[6], v[7], v[8]};
    const Fused2Pick k = fused2_select(q);
    const bool deep = k.family == kInv2P;
    const int r[10] = {(int)k.family, k.inverse, k.f64, k.vec4, k.Lp, k.ew, deep ? k.pdepth : k.wpe, k.packed, k.waves,
                       deep ? inv2p_instantiated(k.inv2p()) : fused2s_instantiated(k.fused2s())};
    for (int i = 0; i < 10; ++i) out[i] = r[i];
}
// One pass along one axis.  v: f64, syn, path_auto, wrap, L, stride, comp, inner, n, outer, contiguous, aligned
// out: the pick in full -- kernel (AxisKernel), grid; the march's inner, n, n_in, ngroups, chunk, nchunks; AxisX's ew, vec4, row, nseg;
// AxisX's segment width by wave_row_width; whether the instance lists (ndwt_fused_list.h) hold the instance (the element-wise kernels: 1)
extern "C" void sel_axis(const long long* v, long long* out) {
    const AxisQuery q = {v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, (int)v[4], v[5], (int)v[6], v[7], v[8], v[9], v[10] != 0, v[11] != 0};
    const AxisPick k = axis_select(q);
    const long long r[14] = {(long long)k.kernel, k.grid, k.inner, k.n, k.n_in, k.ngroups, k.chunk, k.nchunks, k.ew, k.vec4, k.row, k.nseg,
                             wave_row_width(q.syn, q.L, q.comp, q.f64, 1),
                             k.kernel == kAxisMarch ? axis_march_instantiated(k.march()) : k.kernel == kAxisX ? axisx_instantiated(k.axisx()) : true};
    for (int i = 0; i < 14; ++i) out[i] = r[i];
}
// the same for `count` queries of 12 values each, 14 answers each
extern "C" void sel_axis_many(const long long* v, long long count, long long* out) {
    for (long long i = 0; i < count; ++i) sel_axis(v + 12 * i, out + 14 * i);
}
// whether the lists hold AxisMarch<T, L, SYN> / AxisX<T, L, SYN, EW, VEC4>
extern "C" int sel_axis_march_listed(int f64, int syn, int L) { return axis_march_instantiated({f64 != 0, syn != 0, L}); }
extern "C" int sel_axisx_listed(int f64, int syn, int vec4, int L, int ew) { return axisx_instantiated({f64 != 0, syn != 0, vec4 != 0, L, ew}); }
// whether the lists hold the Fwd2S / Inv2S instance v: inverse, f64, vec4, Lp, ew, wpe
extern "C" int sel_fused2s_listed(const int* v) { return fused2s_instantiated({v[0] != 0, v[1] != 0, v[2] != 0, v[3], v[4], v[5]}); }
extern "C" int sel_cascade2_rec_depth(int variant_inv) { return cascade2_rec_depth(variant_inv); }
