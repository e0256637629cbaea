// ndwt_select.h -- which kernel a level runs: plain host C++ on integers (no HIP header; any host compiler takes it).
// ndwt_api.hip fills the queries from the plan and the launch's pointers, asks here, and launches what the pick names.
#pragma once
#include "ndwt_fused_list.h"

namespace ndwt {

// ---- the A/B variants of ndwt_plan_set_variant (tools/: interleaved A/B runs).  The C ABI, api.py, tools/ and the tests pass the numbers;
// every variant computes the same values.  A number that a column does not name selects that column's default.
//  fwd | 3-D analysis (fused3_select)                                        | 2-D
//   0  | default: tall tile for 6 / 8 taps on volumes that fill the chip, pinned taps for 10 .. 14
//   1  | 64x16 tile, 512 threads, one column per thread (float 10 .. 16 taps, double 6 / 8)
//   2  | float: the tall 64x32 tile whatever the volume; ndwt_denoise: its band-0 analysis on the tall tile
//   3  | keeps the small tile (float 64x16, double 64x8); 16 / 20 taps: the spilling forms without window slots in LDS
//   6  | float: tall tile with y items of 2 rows (8 .. 12 taps)
//   7  | 4-D: the t axis folded into the fused launches (Fwd3 TPRE)
//   8  | as 0 without the pinned taps
//   9  |                                                                     | no cascade (analysis AND synthesis): one launch per level
//  10  |                                                                     | cascade whatever the image size, kernel mode 1 (no take-in-only steps)
//  11  |                                                                     | cascade whatever the image size
//      (a batched 1-D plan, cascade1_levels: fwd 9 = one launch per level in the analysis, inv 9 = in the synthesis; nothing else applies)
//      (ndwt_denoise_bands / ndwt_denoise_bands_items of a batched 1-D plan, denoise1_levels: fwd 11 AND inv 11 = the one-launch Den1C wherever it exists, 9 in either slot = off)
//      (interleaved samples, one axis, cascadem_levels: fwd / inv 9 = one launch per level, 11 = the cascaded march wherever it exists)
//      (ndwt_band_select, select_agg: fwd 9 = the histogram passes without the wave-wide combining of equal digits)
//      (ndwt_band_select_items, select_items_route: inv 11 = every item in one launch (ItemSelect), inv 9 = the BandHist / BandPick passes once per item)
//  inv | 3-D synthesis (fused3_select)                                       | 2-D (fused2_select)                | 2-D cascade (cascade2_levels)
//   0  | default: Inv3Y (gather <= 8 taps, scatter from 10), else Inv3S      | Inv2P depth 4 packed, 1024 waves, where the image fits one round
//   1  |                                                                     | keeps Inv2S
//   2  | dilated levels keep Inv3S                                           | Inv2P depth 2 on Inv2S's geometry  |
//   3  | the LDS kernel Inv3 (8 taps); otherwise Inv3S                       | (>= 2: Inv2P whatever the size)    |
//   4  | Inv3S, the lane-shift kernel                                        | Inv2P depth 4 on Inv2S's geometry  |
//   5  | Inv3Y with one register set of band loads (depth 1)                 |                                    |
//   6  |                                                                     | Inv2P depth 2, 1024 waves          |
//   7  |                                                                     | Inv2P with scalar FMAs (unpacked)  |
//   9  | Inv3Y gather form without the shared y / z tap pairs                |                                    | off
//  10  | Inv3Y scatter form wherever it exists (8 taps; EW 4: 4 / 6 too)     |                                    |
//  11  | Inv3Y gather form for every tap length                              |                                    | whatever the image size
//  12  |                                                                     |                                    | ... with two rows of band loads in flight
// (tests/emu/ndwt_emu.cpp takes a `variant` of its own -- 5 / 8 / 10 pick the emulated kernel form; that numbering is local to the emulator.)
enum FwdVariant { kFwdDefault = 0, kFwdOneColumn = 1, kFwdTall = 2, kFwdSmallTile = 3, kFwdTallRY2 = 6, kFwdFoldT = 7, kFwdNoPin = 8,
                  kFwdNoCascade = 9, kFwdCascadeMode1 = 10, kFwdCascadeAlways = 11 };
enum InvVariant { kInvDefault = 0, kInvDilatedKeep3S = 2, kInvLds = 3, kInvLaneShift = 4, kInvDepth1 = 5, kInvNoUniYZ = 9, kInvScatter = 10, kInvGather = 11,   // 3-D
                  kInv2Keep2S = 1, kInv2Depth2Geom = 2, kInv2Depth4Geom = 4, kInv2Depth2Round = 6, kInv2Unpacked = 7,                                        // 2-D
                  kInvCascadeOff = 9, kInvCascadeAlways = 11, kInvCascadeDepth2 = 12 };                                                                       // 2-D cascade

// ---- what the predicates need of a plan
struct SelPlan {
    int ndim, comp;                    // comp: scalars per element (2: interleaved complex)
    bool f64, real, path_auto, atrous, fp64_fused;
    long long dims[4];
    int len[4];                        // tap length per axis
    int variant_fwd, variant_inv;
    long long howmany = 0;             // items of a batched plan: the signals of ndwt_plan_create_many, or the images / volumes of a stack
                                       // (ndwt_plan_create_axes: ndim and dims are those of ONE item); 0 = not batched
    long long inner = 1;               // ndwt_plan_create_interleaved: elements of a sample that lie together, faster in memory than dims[0];
                                       // every filtered axis is then strided: the per-axis kernels, and for one axis the cascaded march
};
constexpr bool is_stack(const SelPlan& p) { return p.howmany > 0 && p.ndim >= 2; }
constexpr bool is_interleaved(const SelPlan& p) { return p.inner > 1; }

inline int padded_len(const int* len) { int Lp = 2; for (int a = 0; a < 3; ++a) Lp = len[a] > Lp ? len[a] : Lp; return Lp; }
// the zero padding (Lp - len) / 2 of every axis' taps is even: the kernels that derive the high-pass taps from the low-pass ones
// (mirror + alternating signs) need it
inline bool padding_even(const int* len, int Lp) {
    for (int a = 0; a < 3; ++a)
        if (((Lp - len[a]) / 2) % 2 != 0) return false;
    return true;
}
// the fused kernels keep intra-plane offsets in 32-bit ints
inline bool fused3_fits(long long n1, long long n2, long long n3, long long nbatch) {
    return n1 * n2 < (1LL << 31) && n3 < (1LL << 30) && nbatch < (1LL << 20) && n1 >= 1 && n2 >= 1 && n3 >= 1;
}

// Float synthesis default: the pair-packed kernel Inv3Y.  It derives the high-pass taps from the low-pass ones and keeps plane offsets in
// 32-bit BYTE counts (plane = scalars per undilated plane).  kInvLds / kInvLaneShift force the older kernels for A/B runs.
inline bool inv3y_ok(bool f64, int comp, const int* len, int Lp, long long plane, int variant_inv) {
    if (f64 || Lp > (comp == 1 ? 20 : 16) || variant_inv == kInvLds || variant_inv == kInvLaneShift) return false;
    return padding_even(len, Lp) && plane < (1LL << 30);
}
inline bool inv3y_plan_ok(const SelPlan& p, int Lp) { return inv3y_ok(p.f64, p.comp, p.len, Lp, p.dims[0] * p.comp * p.dims[1], p.variant_inv); }

// dir: 0 analysis, 1 synthesis, -1 both.  Instantiated tap lengths: 2..12 (db1..db6) for every data kind the checks below let
// through; float real data also 14 .. 20 (db7 .. db10; 18- and 20-tap synthesis with the pair-packed kernel only), double real data 14 and 16.
inline bool fused3_eligible(const SelPlan& p, long long stride, int* Lp_out, int dir = -1) {
    if (!p.path_auto || stride != 1 || p.ndim < 3) return false;
    if (p.f64 && !p.fp64_fused) return false;
    const int Lp = padded_len(p.len);
    const int lmax = !p.real ? (!p.f64 && dir == 0 ? 16 : 12) : (!p.f64 ? (dir == 0 ? 20 : 16) : 16);
    // 18- and 20-tap synthesis exist as the pair-packed kernel only (uniform wavelets, or mixed ones with even padding on every axis)
    if (Lp > lmax && !(dir == 1 && Lp <= 20 && inv3y_plan_ok(p, Lp))) return false;
    if (p.f64 && Lp > 16) return false;   // double: up to db8 (64x8 tiles with 512 threads keep 10 .. 16 taps in 256 registers)
    // interleaved complex: the fused kernels with the x taps stepping over (re, im) pairs, tap lengths <= 8 (float: <= 12); rows of an
    // odd number of elements run the VEC4 = false instances (one access per lane wherever its 4 scalars are contiguous)
    // (complex128: 10 taps both ways, 12 taps analysis only -- its synthesis spills 500+ registers on every tile)
    // (complex64: 14 / 16 taps in the analysis, and in the synthesis through the pair-packed kernel -- the Lp > lmax clause above)
    if (!p.real && Lp > (!p.f64 ? 16 : (dir == 0 ? 12 : 10))) return false;
    if (!fused3_fits(p.dims[0] * p.comp, p.dims[1], p.dims[2] + 64, p.ndim == 4 ? p.dims[3] + 64 : is_stack(p) ? p.howmany : 1)) return false;
    *Lp_out = Lp;
    return true;
}

// A dilated (a-trous) 3-D level whose axes all divide by the tap stride s is s^3 independent stride-1 problems on the
// sub-lattices: the fused kernels take x with the taps stepping over s interleaved scalars (the EW parameter, as for
// interleaved complex data) and the s^2 (y, z) sub-lattices as batch items with row / plane strides s*n1, s*n1*n2.
inline bool fused3_dilated_eligible(const SelPlan& p, long long stride, int* Lp_out) {
    if (!p.path_auto || p.ndim != 3 || !p.real) return false;
    if (stride != 2 && !(stride == 4 && !p.f64)) return false;   // instantiated: EW = 2 (float, double), EW = 4 (float)
    if (p.f64 && !p.fp64_fused) return false;
    const int Lp = padded_len(p.len);
    if (Lp > 8 || p.dims[0] % stride != 0 || p.dims[1] % stride != 0 || p.dims[2] % stride != 0 || p.dims[0] % 4 != 0) return false;
    if (!fused3_fits(p.dims[0], p.dims[1], p.dims[2] + 64, stride * stride)) return false;
    *Lp_out = Lp;
    return true;
}

// the 2-D analogue: x through EW = stride, the `stride` row sub-lattices as batch items.  Which strides and scalar types have the
// instances is the table's answer (ndwt_fused_list.h); the float lists of EW = 2 go on to 16 taps for complex64, and a dilated level
// has only ever run, and been checked, up to kFused2DilatedMaxTaps
constexpr int kFused2DilatedMaxTaps = 8;
inline bool fused2_dilated_eligible(const SelPlan& p, long long stride, int* Lp_out) {
    if (!p.path_auto || p.ndim != 2 || !p.real || stride < 2) return false;
    const int Lp = p.len[0] > p.len[1] ? p.len[0] : p.len[1];
    if (p.dims[0] % stride != 0 || p.dims[1] % stride != 0 || p.dims[0] % 4 != 0) return false;
    if (p.dims[0] >= (1LL << 30) || p.dims[1] >= (1LL << 30)) return false;
    if (Lp > kFused2DilatedMaxTaps || !fused2s_both_ways(p.f64, Lp, (int)stride)) return false;
    *Lp_out = Lp;
    return true;
}

// one level at tap stride 1: the tap lengths the table has both ways for the plan's scalar type and x step (float real up to db10,
// complex64 and double real up to db8, complex128 up to db4)
inline bool fused2_eligible(const SelPlan& p, long long stride, int* Lp_out) {
    if (!p.path_auto || stride != 1 || p.ndim != 2) return false;
    const int Lp = p.len[0] > p.len[1] ? p.len[0] : p.len[1];
    if (!fused2s_both_ways(p.f64, Lp, p.real ? 1 : 2)) return false;
    if (p.dims[0] >= (1LL << 30) || p.dims[1] >= (1LL << 30)) return false;
    *Lp_out = Lp;
    return true;
}

// ---- the route of one level: which fused form it takes, or the per-axis passes, and with which padded tap length.  ndwt_api.hip asks
// once per level and switches on the answer; the predicates above are what the answer is written in.
enum LevelRouteKind {
    kRouteFused3Dilated,               // a dilated 3-D level: the fused 3-D kernels on its sub-lattices
    kRouteFused3,                      // one fused 3-D launch
    kRouteFused3T,                     // 4-D (nd_dwt_4D.m dec / rec): the t filter pair as a per-axis pass, the 3-D level of both t-bands as two fused
                                       // launches batched over the frames.  t stays whole on a slab sharded on z: the pass is periodic over the
                                       // z-extended frames (nt, nz + L_z - 1, ny, nx), and the fused launches take the halo on z with per-frame strides
    kRouteFused3FoldT,                 // 4-D analysis, kFwdFoldT: t folded into those two launches (16-byte-aligned pointers only: the caller falls back to kRouteFused3T)
    kRouteFused2Dilated,               // a dilated 2-D level: the fused 2-D kernels on its row sub-lattices
    kRouteFused2,                      // one fused 2-D launch
    kRoutePerAxis                      // one pass per axis; on a slab, the halo treatment on the sharded axis
};
struct LevelRoute { LevelRouteKind kind; int Lp; };   // Lp: the padded tap length of the fused forms, 0 for the per-axis passes
constexpr bool route_fused3(LevelRouteKind k) { return k == kRouteFused3 || k == kRouteFused3T || k == kRouteFused3FoldT; }

// On a slab the input (every synthesis input) carries the halo planes of the sharded axis: the outermost one, or z of a 4-D volume.
enum SlabMode { kWholeArray, kSlabOuter, kSlabZ };
// Slabs have no sub-lattice form, and a fused kernel marches exactly Lp - 1 halo planes: where the halo is on the kernel's own outer axis
// (z of a 3-D slab or of a 4-D volume sharded on z, y of an image) that axis' filter has to be the longest.  (A 4-D slab on t: t is the
// per-axis pass.)
// A stack (ndwt_plan_create_axes) takes the one-launch forms with its items in the batch slot of the launch.  The sub-lattice forms of a
// dilated level use that slot themselves: they are not offered, and a dilated level of a stack runs the per-axis passes.
inline LevelRoute level_route(const SelPlan& p, long long stride, int dir, SlabMode mode) {
    const bool slab = mode != kWholeArray, halo_on_z = mode == kSlabZ || (mode == kSlabOuter && p.ndim == 3);
    int Lp = 0;
    if (is_interleaved(p)) return {kRoutePerAxis, 0};     // no fused form reads samples of `inner` elements
    if (is_stack(p)) {
        if (slab || stride != 1 || p.howmany >= (1LL << 20)) return {kRoutePerAxis, 0};
        if (p.ndim == 3 && fused3_eligible(p, stride, &Lp, dir)) return {kRouteFused3, Lp};
        if (p.ndim == 2 && fused2_eligible(p, stride, &Lp)) return {kRouteFused2, Lp};
        return {kRoutePerAxis, 0};
    }
    if (!slab && fused3_dilated_eligible(p, stride, &Lp)) return {kRouteFused3Dilated, Lp};
    if (fused3_eligible(p, stride, &Lp, dir) && !(halo_on_z && p.len[2] != Lp)) {
        if (p.ndim == 3) return {kRouteFused3, Lp};
        const bool fold = p.variant_fwd == kFwdFoldT && dir == 0 && !slab && stride == 1 && !p.f64 && p.real && Lp <= 8 && p.len[3] <= Lp &&
                          p.dims[0] % 4 == 0 && (p.comp * p.dims[0] * p.dims[1] * p.dims[2]) % 4 == 0 && p.dims[3] >= 2;
        return {fold ? kRouteFused3FoldT : kRouteFused3T, Lp};
    }
    if (!slab && fused2_dilated_eligible(p, stride, &Lp)) return {kRouteFused2Dilated, Lp};
    if (fused2_eligible(p, stride, &Lp) && !(slab && p.len[1] != Lp)) return {kRouteFused2, Lp};
    return {kRoutePerAxis, 0};
}
// a slab level on the fused 3-D kernel with the halo on z (what the split-halo / zero-extended slab entry points need): its Lp, else 0
inline int slab_fused3(const SelPlan& p, long long stride, int dir, SlabMode mode) {
    const LevelRoute r = level_route(p, stride, dir, mode);
    return (r.kind == kRouteFused3 || (r.kind == kRouteFused3T && mode == kSlabZ)) ? r.Lp : 0;
}

// true when every synthesis level of this plan runs a kernel that can shrink its inputs on load (Inv3S / Inv3Y / Inv2S / Inv2P)
inline bool fused_shrink_capable(const SelPlan& p) {
    if (p.atrous || is_interleaved(p)) return false;                  // dilated levels, interleaved samples: the per-axis kernels
    const LevelRoute r = level_route(p, 1, -1, kWholeArray);
    return r.kind == kRouteFused2 || (route_fused3(r.kind) && !(p.variant_inv == kInvLds && r.Lp == 8));   // the LDS synthesis kernel does not
}

// ---- two or three levels of an image in one launch (Fwd2C / Inv2C) at tap stride 1: rows of whole groups of 4 SCALARS (interleaved
// complex: two per element), the tap lengths and level counts of the instance table (ndwt_fused_list.h: NDWT_LIST_*2C -- float real up to
// 8 taps, analysis also 12 at two levels; which double and complex forms fit the registers is written there).  By default for images
// from a size per data kind and direction on, in BYTES (cascade2_min_bytes: below it the rows a wave reads before its chunk produces
// anything outweigh the volumes saved), or on request.  `left` = levels still to do; returns how many the next launch takes (and the padded tap length),
// 0 = one launch per level.
// The smallest image, in bytes, that takes the cascade unasked (db4, 3 levels, against the build before these kinds had
// the cascade, at 2048^2 / 4096^2 / 8192^2; a kind and direction takes it from the smallest measured size on at which it won by more than
// the 5 % spread between boxes).  float real: beyond 2048 x 3072 (equal at 2048^2, -33 % / -22 % at 4096^2), as ever; complex64 from
// 2048^2 = 32 MiB (-20 % / -28 %); double real: the analysis from 2048^2 = 32 MiB (-17 %), the synthesis from 4096^2 = 128 MiB (-14 %;
// at 2048^2 its one wave per SIMD is 24 % SLOWER than three launches); complex128 from 2048^2 = 64 MiB (-37 % / -10 %)
constexpr long long cascade2_min_bytes(bool f64, int comp, bool inverse) {
    return !f64 ? (comp == 1 ? (24LL << 20) + 1 : (32LL << 20)) : comp == 1 ? (inverse ? (128LL << 20) : (32LL << 20)) : (64LL << 20);
}
// A stack of images takes the cascade under the same conditions, which are per item (one wave marches rows of ONE item).  Whether it
// does so unasked is measured per data kind and direction (tools/bench2d_stack.py: db4, 3 levels, forced cascade against
// one launch per level on stack plans): from the smallest measured (item height, bytes of all items) on at which the cascade won by more
// than the 5 % spread between boxes.  float real: the analysis from 128 rows (-30 % at 1024 x 128^2, -35 % at 256 x 256^2, -33 % at
// 64 x 512^2), the synthesis from 256 rows (-0.3 % at 128 rows -- its march-in reads every band --, -7 % at 256, -21 % at 512), both at
// 64 MiB; complex64 (-25 % / -7 %), double (-23 % / -18 %) and complex128 (-19 % / -24 %) from 512 rows at 128 MiB, the smallest measured.
// Below these nothing is known and nothing is taken unasked: variants 10 / 11 / 12 force the cascade, 9 switches it off.
constexpr bool cascade2_stack_default(bool f64, int comp, bool inverse, long long n2, long long total_bytes) {
    return (!f64 && comp == 1) ? n2 >= (inverse ? 256 : 128) && total_bytes >= (64LL << 20) : n2 >= 512 && total_bytes >= (128LL << 20);
}
inline int cascade2_levels(const SelPlan& p, bool inverse, int left, int* Lp_out) {
    int& Lp = *Lp_out;
    if (left < 2 || p.atrous || is_interleaved(p) || p.variant_fwd == kFwdNoCascade || (p.comp != 1 && p.comp != 2) || !fused2_eligible(p, 1, &Lp)) return 0;
    const long long n1 = p.dims[0] * p.comp;              // scalars along x
    if (n1 % 4 != 0 || p.dims[1] < 3 * (Lp - 1)) return 0;
    if (n1 * p.dims[1] >= (1LL << 31)) return 0;          // the kernel's row * row-stride products are formed in 64 bits, offsets in int
    const auto exists = [&](int nlev) { return cascade2_instantiated({inverse, p.f64, p.comp, Lp, nlev, inverse ? 1 : 0}); };
    const int n = (left >= 3 && exists(3)) ? 3 : exists(2) ? 2 : 0;
    if (!n) return 0;
    const long long bytes = n1 * p.dims[1] * (p.f64 ? 8 : 4);
    const bool big = is_stack(p) ? cascade2_stack_default(p.f64, p.comp, inverse, p.dims[1], bytes * p.howmany) : bytes >= cascade2_min_bytes(p.f64, p.comp, inverse);
    if (inverse ? (p.variant_inv == kInvCascadeOff || !(big || p.variant_inv == kInvCascadeAlways || p.variant_inv == kInvCascadeDepth2))
                : !(big || p.variant_fwd == kFwdCascadeAlways || p.variant_fwd == kFwdCascadeMode1)) return 0;
    return n;
}
constexpr int cascade2_rec_depth(int variant_inv) { return variant_inv == kInvCascadeDepth2 ? 2 : 1; }   // Inv2C: rows of band loads in flight per level
// ... of the launch of `nlev` levels: the depth asked for where the instance exists, one row otherwise
inline int cascade2_rec_depth(const SelPlan& p, int Lp, int nlev) {
    const int want = cascade2_rec_depth(p.variant_inv);
    return cascade2_instantiated({true, p.f64, p.comp, Lp, nlev, want}) ? want : 1;
}

// ---- two to four levels of the signals of a batched 1-D plan in one launch (Fwd1C / Inv1C, ndwt_device_1d.h) at the reference's
// dilation: rows of whole groups of 4 scalars, at least 8 L of them (AxisX's own floor: whichever way a level goes, it runs the lane-shift
// kernel), tap lengths 2 .. 8.  p.howmany = signals of the plan (0: not a batched plan); `left` = levels still to do.  Returns how many
// the next launch takes -- the largest instantiated count <= left -- and the tap length; 0 = one launch per level.  kFwdNoCascade takes
// the analysis off, kInvCascadeOff the synthesis (A/B runs: tools/bench1d_batch.py).
// what Fwd1C / Inv1C and Den1C ask of a plan alike: batched 1-D signals at the reference's dilation, rows as described above
inline bool rows1_plan_ok(const SelPlan& p) {
    if (p.howmany < 1 || p.ndim != 1 || p.atrous || is_interleaved(p) || !p.path_auto || (p.comp != 1 && p.comp != 2)) return false;
    const int L = p.len[0];
    const long long n1 = p.dims[0] * p.comp;              // scalars per row
    return L >= 2 && L <= 8 && n1 % 4 == 0 && n1 >= 8LL * L && n1 < (1LL << 30);
}
inline int cascade1_levels(const SelPlan& p, bool inverse, int left, int* L_out) {
    if (!rows1_plan_ok(p)) return 0;
    if (inverse ? p.variant_inv == kInvCascadeOff : p.variant_fwd == kFwdNoCascade) return 0;
    const int L = p.len[0];
    for (int n = left < 4 ? left : 4; n >= 2; --n)
        if (cascade1_instantiated({inverse, p.f64, p.comp, L, n})) { *L_out = L; return n; }
    return 0;
}

// ---- ndwt_denoise_bands of a batched 1-D plan in ONE launch (Den1C, ndwt_device_1d.h): dec, the per-band thresholding and rec of all
// `level` levels with the coefficients in registers, under cascade1_levels' conditions, 1 <= level <= 4 (deeper transforms take the
// general route: dec, one shrink pass per band, rec).  Returns `level` if the whole depth fits one launch, else 0.  Either A/B switch
// (kFwdNoCascade, kInvCascadeOff) takes it off.
inline int denoise1_levels(const SelPlan& p, int level) {
    if (level < 1 || level > 4 || !rows1_plan_ok(p)) return 0;
    if (p.variant_fwd == kFwdNoCascade || p.variant_inv == kInvCascadeOff) return 0;
    return den1_instantiated({p.f64, p.comp, p.len[0], level}) ? level : 0;
}
// Whether ndwt_denoise_bands takes that launch unasked.  The rule of DESIGN.md 4.3b: a data kind takes it by default only if it was
// measured to win by more than the 5 % spread between boxes on every measured shape of the kind.  Measured on the MI355X
// (tools/bench1d_denoise.py, profiles/bench1d_denoise.txt; the table is in DESIGN.md 4.3d), one launch against the parent's
// ndwt_denoise with one threshold / against the general route of ndwt_denoise_bands, db4 at 4 levels and db2 at 3:
//   float      4096 x 4096, 65536 x 256, 16 x 2^20:  0.49 .. 0.57 / 0.31 .. 0.39 (db4),  0.36 .. 0.42 / 0.23 .. 0.30 (db2)
//   complex64  4096 x 2048:                          0.75 / 0.48 (db4),  0.41 / 0.27 (db2)
//   double     4096 x 4096:                          0.28 / 0.18 (db4),  0.18 / 0.12 (db2)
// so float, complex64 and double take it unasked.  complex128 was not measured (and three of its instances are not built): on request
// only, ndwt_plan_set_variant(plan, 11, 11, ...).
constexpr bool denoise1_default(bool f64, int comp) { return !(f64 && comp == 2); }
inline bool denoise1_wanted(const SelPlan& p) {
    return (p.variant_fwd == kFwdCascadeAlways && p.variant_inv == kInvCascadeAlways) || denoise1_default(p.f64, p.comp);
}

// ---- two to four levels of ONE strided axis inside one march (FwdMC / InvMC, ndwt_device_axis.h): a plan over interleaved samples
// (ndwt_plan_create_interleaved) with one filtered axis, at the reference's dilation, tap lengths 2 .. 8, sample blocks of whole groups
// of 4 scalars.  `left` = levels still to do.  Returns how many the next launch takes -- the largest instantiated count <= left -- and
// the tap length; 0 = one launch per level.
// Unasked, the cascade is taken only where it has been measured to win (cascadem_default); kFwdCascadeAlways /
// kInvCascadeAlways force it wherever it exists, kFwdNoCascade / kInvCascadeOff switch it off, each for its own direction.
// Measured on the MI355X, db2 and db4, 3 levels, forced cascade against one launch per level on the same plan (tools/bench_interleaved.py,
// DESIGN.md 4.3c).  The rule of 4.3b: a data kind and direction takes the cascade unasked from the smallest measured size on at which it
// won by more than the 5 % spread between boxes, for both wavelets -- `bytes` = bytes of the whole array.  float real, both directions:
// from 256 MiB (-41 % / -22 % dec, -34 % / -33 % rec for db2 / db4); at 64 MiB db4 is SLOWER in the analysis (+7 %, +15 %) and equal in
// the synthesis of the channels-first shape, at 8 MiB db2 is equal (dec) and slower (rec, +23 %).  double at 16 MiB: db2 -4 % / +33 %,
// db4 -27 % / +6 % -- no size measured to win both ways; complex64 was measured at 16 MiB only (dec -10 % / -39 %, rec +10 % / -19 %) and
// complex128 not at all: on request only (kCascadeMNever).
constexpr long long kCascadeMNever = 0x7fffffffffffffffLL;
constexpr long long cascadem_min_bytes(bool f64, int comp, bool inverse) {
    (void)inverse;
    return (!f64 && comp == 1) ? (256LL << 20) : kCascadeMNever;
}
constexpr bool cascadem_default(bool f64, int comp, bool inverse, long long bytes) { return bytes >= cascadem_min_bytes(f64, comp, inverse); }
inline int cascadem_levels(const SelPlan& p, bool inverse, int left, int* L_out) {
    if (p.ndim != 1 || !is_interleaved(p) || p.atrous || !p.path_auto || left < 2) return 0;
    if (inverse ? p.variant_inv == kInvCascadeOff : p.variant_fwd == kFwdNoCascade) return 0;
    const int L = p.len[0];
    if (L < 2 || L > 8 || (p.comp * p.inner) % 4 != 0) return 0;
    const long long items = p.howmany > 0 ? p.howmany : 1;
    const long long bytes = p.comp * p.inner * p.dims[0] * items * (p.f64 ? 8 : 4);
    if (!(inverse ? p.variant_inv == kInvCascadeAlways : p.variant_fwd == kFwdCascadeAlways) && !cascadem_default(p.f64, p.comp, inverse, bytes)) return 0;
    for (int n = left < 4 ? left : 4; n >= 2; --n)
        if (cascadem_instantiated({inverse, p.f64, L, n})) { *L_out = L; return n; }
    return 0;
}

// ---- the route of the next launch of a multi-level transform with `left` levels still to do: the cascade that takes `nlev` of them in
// one launch, or kCascadeNone -- one launch for one level, by level_route.  dec_impl / rec_impl (ndwt_api.hip) ask once per launch and
// switch on the answer; the three predicates above are what the answer is written in.  At most one of them claims a plan: a batched
// 1-D plan, one axis of interleaved samples, an image (tests/test_dispatch_select.py holds them to that), so the order of the questions
// decides nothing.  A further cascade family is one more question here and one more case in each walk.
enum CascadeKind { kCascadeNone, kCascadeRows1, kCascadeMarch, kCascadeImage2 };   // none | Fwd1C / Inv1C | FwdMC / InvMC | Fwd2C / Inv2C
struct CascadeRoute { CascadeKind kind; int nlev; int L; };   // L: the tap length (padded, for the 2-D family); kCascadeNone: nlev = L = 0
inline CascadeRoute cascade_route(const SelPlan& p, bool inverse, int left) {
    int L = 0;
    if (const int n = cascade1_levels(p, inverse, left, &L)) return {kCascadeRows1, n, L};
    if (const int n = cascadem_levels(p, inverse, left, &L)) return {kCascadeMarch, n, L};
    if (const int n = cascade2_levels(p, inverse, left, &L)) return {kCascadeImage2, n, L};
    return {kCascadeNone, 0, 0};
}

// ---- the chunks of a marched axis (AxisMarch, FwdMC / InvMC): a thread marches `chunk` planes of the n, and a launch has `iblocks`
// workgroups per chunk.  About 4096 workgroups in all, chunks of at least `floor` planes (the march-in of a chunk re-reads planes of its
// neighbour), or of `forced` planes where that is set (ndwt_plan_set_tuning: the floor does not apply), and at most the axis.
struct MarchChunks { int chunk, nchunks; };
inline MarchChunks march_chunks(long long n, long long iblocks, long long floor, long long forced) {
    long long want = (4096 + iblocks - 1) / iblocks;
    if (want < 1) want = 1;
    long long chunk = (n + want - 1) / want;
    if (chunk < floor) chunk = floor;
    if (forced > 0) chunk = forced;
    if (chunk > n) chunk = n;
    return {(int)chunk, (int)((n + chunk - 1) / chunk)};
}

// ---- one pass along one axis (axis_pass, ndwt_api.hip): the route every plan can fall back to -- 1-D signals, interleaved samples, the t
// axis of 4-D, dilated levels without a sub-lattice form, long double filters, thin slabs, NDWT_PATH_GENERIC.  The array is
// [outer][n][inner] scalars and the filter runs along n.  Three kernels, asked in this order:
//   AxisMarch  the filter window in registers, a thread owning 4 consecutive scalars of `inner`: whole groups of 4 below the filtered index
//              and every pointer on such a group.  A dilated periodic axis whose length is a multiple of the tap stride s, with at least
//              L samples per sub-lattice, is s interleaved unit-stride problems: [outer][n / s][s * inner] -- the contiguous axis for
//              s >= 4 included.  Any other dilated pass has no march.
//   AxisX      the contiguous axis of a plan without interleaved samples, periodic at tap stride 1, up to 12 taps, rows of at least 8 L
//              scalars: one wave per row segment of wave_row_width scalars, four to the workgroup
//   the element-wise kernels (axis_analysis_kernel / axis_synthesis_kernel): anything, a grid-stride loop over at most 256 * 64 workgroups
// A kernel is passed over where it has no instance (ndwt_fused_list.h) or the launch cannot express its grid, so the pick is final:
// after it, "no instance" and "geometry mismatch" are internal errors of the launch.
enum AxisKernel { kAxisMarch, kAxisX, kAxisPlain };
struct AxisQuery {
    bool f64, syn, path_auto, wrap;    // wrap: periodic; else the input starts `left` planes before output plane 0 and has n + (L - 1) stride planes (a slab)
    int L;                             // tap length
    long long stride;                  // tap stride
    int comp;                          // scalars per element
    long long inner, n, outer;         // the view, in scalars (inner carries comp and the plan's sample block); all >= 1
    bool contiguous;                   // the filtered axis is axis 0 of a plan without interleaved samples: inner == comp
    bool aligned;                      // every pointer the pass reads or writes lies on a group of 4 scalars
};
struct AxisPick {
    AxisKernel kernel;
    bool f64, syn;
    int L;
    long long grid;                    // workgroups of the launch (of 256 threads, whichever the kernel)
    long long inner, n, n_in, ngroups; // kAxisMarch: the view it marches (a sub-lattice view where the pass is dilated) and inner / 4
    int chunk, nchunks;                //             march_chunks
    int ew;                            // kAxisX: scalars per element
    bool vec4;                         //         rows of whole groups of 4 scalars on aligned pointers
    long long row, nseg;               //         scalars of a row, wave segments per row
    constexpr AxisMarchInstance march() const { return {f64, syn, L}; }
    constexpr AxisXInstance axisx() const { return {f64, syn, vec4, L, ew}; }
};
inline AxisPick axis_select(const AxisQuery& q) {
    AxisPick k = {kAxisPlain, q.f64, q.syn, q.L, 0, 0, 0, 0, 0, 0, 0, q.comp, false, 0, 0};
    if (q.inner < 1 || q.n < 1 || q.outer < 1) return k;  // (nothing to do: axis_pass does not ask)
    const long long kMaxGrid = 0x7fffffffLL;
    long long m_inner = q.inner, m_n = q.n, m_n_in = q.wrap ? q.n : q.n + (long long)(q.L - 1) * q.stride;
    bool march_ok = q.path_auto;
    if (q.stride > 1) {
        if (q.wrap && q.n % q.stride == 0 && q.n / q.stride >= q.L) { m_inner = q.inner * q.stride; m_n = q.n / q.stride; m_n_in = m_n; }
        else march_ok = false;
    }
    if (march_ok && m_inner % 4 == 0 && q.aligned && axis_march_instantiated(k.march())) {
        const long long ngroups = m_inner / 4, iblocks = (ngroups * q.outer + 255) / 256;
        const MarchChunks c = march_chunks(m_n, iblocks, 4LL * (q.L - 1) > 8 ? 4LL * (q.L - 1) : 8, 0);
        if (iblocks * c.nchunks <= kMaxGrid) {
            k.kernel = kAxisMarch; k.grid = iblocks * c.nchunks;
            k.inner = m_inner; k.n = m_n; k.n_in = m_n_in; k.ngroups = ngroups; k.chunk = c.chunk; k.nchunks = c.nchunks;
            return k;
        }
    }
    if (q.path_auto && q.contiguous && q.stride == 1 && q.wrap && q.L <= 12 && q.n * q.comp >= 8LL * q.L) {
        const long long row = q.n * q.comp;
        k.vec4 = row % 4 == 0 && q.aligned;
        if (axisx_instantiated(k.axisx()) && row < (1LL << 30)) {
            const long long WX = axisx_tile_width(k.axisx()), nseg = (row + WX - 1) / WX, grid = (q.outer * nseg + 3) / 4;
            if (grid <= kMaxGrid) {
                k.kernel = kAxisX; k.grid = grid; k.row = row; k.nseg = nseg;
                return k;
            }
        }
    }
    const long long nb = (q.outer * q.n * q.inner + 255) / 256;
    k.grid = nb > 256LL * 64 ? 256LL * 64 : nb;           // grid-stride beyond 64 blocks per CU
    return k;
}

// ---- exact order statistics of a band's |c| (ndwt_band_select; BandHist / BandPick, ndwt_device_select.h): a radix select on the bit
// pattern of |c|, most significant digit first.  A non-negative IEEE value orders as its unsigned bit pattern, so the key has 32 bits
// (float, complex64: the magnitude is a float) or 64 (double, complex128).  A pass reads the band once and counts one digit of the keys
// that carry the digits found so far; digits are kSelectDigitBits wide (2048 counters = 8 KB of LDS per rank), the last one is what is
// left: float 11 + 11 + 10 bits = 3 passes, double 5 x 11 + 9 = 6.
constexpr int kSelectDigitBits = 11, kSelectBins = 1 << kSelectDigitBits, kSelectMaxRanks = 4;
constexpr int select_key_bits(bool f64) { return f64 ? 64 : 32; }
constexpr int select_passes(bool f64) { return (select_key_bits(f64) + kSelectDigitBits - 1) / kSelectDigitBits; }
// the digit of pass `pass` (0 = most significant) is bits [shift, shift + bits) of the key
constexpr int select_digit_shift(bool f64, int pass) {
    return select_key_bits(f64) - kSelectDigitBits * (pass + 1) > 0 ? select_key_bits(f64) - kSelectDigitBits * (pass + 1) : 0;
}
constexpr int select_digit_bits(bool f64, int pass) { return select_key_bits(f64) - kSelectDigitBits * pass - select_digit_shift(f64, pass); }
// counters are 32-bit: a band of 2^32 elements or more is refused before any launch
constexpr bool select_fits(long long n_elements) { return n_elements >= 1 && n_elements < (1LL << 32); }
// 16- / 32-byte loads where the band's address is a multiple of 4 scalars and so is its length, one element at a time otherwise (the
// rule of shrink_run)
constexpr bool select_vec(unsigned long long addr, long long n_scalars, int scalar_bytes) {
    return addr % (4ULL * scalar_bytes) == 0 && n_scalars % 4 == 0;
}
// workgroups of 256 threads of a pass: enough for kSelectTurns turns of the grid-stride loop per thread where the band has them (a
// workgroup zeroes and flushes 2048 counters whatever it read: 8 turns of the 4-scalar form are 8192 keys per 2048 counters), capped
// as shrink_run caps its grid (num_cus * 16); target_blocks > 0 (ndwt_plan_set_tuning) is an upper bound on top of that
constexpr int kSelectTurns = 8;
constexpr long long select_grid(long long n_scalars, int comp, bool vec, int num_cus, int target_blocks) {
    long long blocks = ((vec ? n_scalars / 4 : n_scalars / comp) + 256 * kSelectTurns - 1) / (256 * kSelectTurns);
    const long long cap = (long long)num_cus * 16;
    if (blocks > cap) blocks = cap;
    if (target_blocks > 0 && blocks > target_blocks) blocks = target_blocks;
    return blocks < 1 ? 1 : blocks;
}
// rounds of the wave-wide combining of equal digits before the LDS atomics (BandHist AGG): 2 by default, kFwdNoCascade = none (A/B runs:
// tools/bench_select.py; the counts are integers, so every setting gives the same values)
constexpr int select_agg(int variant_fwd) { return variant_fwd == kFwdNoCascade ? 0 : 2; }

// ---- the order statistics of every ITEM of a band (ndwt_band_select_items): two routes to the same keys
//   kItemsOneLaunch  ItemSelect (ndwt_device_items.h): one workgroup runs all passes of one item, every item in one launch
//   kItemsLoop       the BandHist / BandPick passes above once per item, on that item's sub-range; one copy back at the end
// With at least as many items as CUs the one launch fills the chip and moves the same bytes with 2 * passes * items - 1 fewer launches:
// taken unasked (derived, not measured; 4096 x 4096 float: 251 us against 198 ms for the loop).  With fewer items one workgroup per item
// leaves CUs idle while the loop spreads every item over the chip: the one launch takes about as long as ONE item takes one workgroup,
// the loop about items x passes x 21 us of launches.  Measured on the MI355X (tools/bench_select_items.py, real data, us per call, one
// launch / loop; the table is in DESIGN.md 4.3f):
//   items   2^14 scalars            2^18 scalars             2^22 scalars
//   8       float 124 / 534  (0.23) float  681 /  511 (1.33) float  9981 /  650 (15.3)
//           double 171 / 1021 (0.17) double 1234 / 1047 (1.18) double 18333 / 1224 (15.0)
//   64      float 125 / 3797 (0.03) float  758 / 3777 (0.20) float 10469 / 5062 (2.07)
//           double 182 / 8041 (0.02) double 1299 / 8176 (0.16) double 19017 / 9644 (1.97)
// By the rule of DESIGN.md 4.3b -- a size takes the one launch unasked only where it was measured to beat the loop by more than the 5 %
// spread between boxes, and what was not shown to win keeps the loop -- items of up to 2^14 scalars take it from 8 items on, items of
// up to 2^18 scalars from 64 items on; fewer than 8 items, 2^18 scalars on fewer than 64 items (it lost at 8; 16 and 32 were not
// measured) and anything larger keep the loop.  Complex data were not measured: the sizes count scalars.
// items >= num_cus is bounded too: one workgroup needs about 10 ms for 2^22 float scalars (above) and grows with the item, while the loop
// costs about 0.08 ms per item of that size, so at 256 items the one launch wins by 2 at 2^22 scalars and ties near 2^24.  Items beyond
// 2^22 scalars, the largest size measured, keep the loop whatever their number.
// variant_inv 11 forces the one launch, 9 the loop (A/B runs and the tests).
enum ItemsRoute { kItemsOneLaunch, kItemsLoop };
constexpr long long kItemsFewFrom = 8, kItemsOneLaunchMaxScalars = 1LL << 14;          // from 8 items on: items of up to 2^14 scalars
constexpr long long kItemsManyFrom = 64, kItemsOneLaunchMaxScalarsMany = 1LL << 18;    // from 64 items on: items of up to 2^18 scalars
constexpr long long kItemsOneLaunchMaxScalarsFull = 1LL << 22;                         // from num_cus items on: items of up to 2^22 scalars
constexpr ItemsRoute select_items_route(long long item_scalars, long long items, int num_cus, int variant_inv) {
    return variant_inv == kInvCascadeAlways ? kItemsOneLaunch : variant_inv == kInvCascadeOff ? kItemsLoop
         : ((items >= num_cus && item_scalars <= kItemsOneLaunchMaxScalarsFull) || (items >= kItemsFewFrom && item_scalars <= kItemsOneLaunchMaxScalars) ||
            (items >= kItemsManyFrom && item_scalars <= kItemsOneLaunchMaxScalarsMany)) ? kItemsOneLaunch : kItemsLoop;
}
// ... and the workgroups per (band, item) block of ShrinkItems: at least one, as many as the block has steps of 256 threads for, all
// blocks together capped as shrink_run caps its grid (num_cus * 16) wherever bands * items is below that cap
constexpr long long shrink_items_chunks(long long item_scalars, int comp, bool vec, long long bands, long long items, int num_cus) {
    const long long steps = ((vec ? item_scalars / 4 : item_scalars / comp) + 255) / 256, room = (long long)num_cus * 16 / (bands * items);
    const long long c = steps < room ? steps : room;
    return c < 1 ? 1 : c;
}
// ... and the workgroups per (band, item) block of BandNorms (ndwt_device_norms.h): at least one; a further chunk only while every
// thread of 256 still has kSelectTurns turns of its loop (a workgroup that reads too little is all prologue, LDS combine and flush:
// DESIGN.md 4.3e); all blocks together capped at num_cus * 16 wherever bands * items is below that cap; target_blocks > 0
// (ndwt_plan_set_tuning) is an upper bound on all blocks on top of that.  More than one chunk means a second launch (NormsFinish).
constexpr long long norms_chunks(long long item_scalars, int comp, bool vec, long long bands, long long items, int num_cus, int target_blocks) {
    const long long steps = vec ? item_scalars / 4 : item_scalars / comp, blocks = bands * items;
    long long c = steps / (256 * kSelectTurns);
    const long long room = (long long)num_cus * 16 / blocks;
    if (c > room) c = room;
    if (target_blocks > 0 && c > target_blocks / blocks) c = target_blocks / blocks;
    return c < 1 ? 1 : c;
}
// past 2^31 - 1 (band, item) blocks a launch cannot number its workgroups: one launch per band (items < 2^31: a band alone always fits,
// and has one chunk)
constexpr bool norms_per_band(long long bands, long long items) { return bands * items > 0x7fffffffLL; }
// ... and the workgroups per band of JointShrink / GroupNorms (ndwt_device_joint.h), whose step moves one load of every item: at least
// one; a further chunk only while every thread of 256 keeps max(1, kSelectTurns / items) steps; all bands together within num_cus * 16;
// target_blocks > 0 is an upper bound on all workgroups on top of that, as for norms_chunks.
constexpr long long joint_chunks(long long item_scalars, int comp, bool vec, long long bands, long long items, int num_cus, int target_blocks) {
    const long long steps = vec ? item_scalars / 4 : item_scalars / comp, turns = kSelectTurns / items < 1 ? 1 : kSelectTurns / items;
    long long c = steps / (256 * turns);
    const long long room = (long long)num_cus * 16 / bands;
    if (c > room) c = room;
    if (target_blocks > 0 && c > target_blocks / bands) c = target_blocks / bands;
    return c < 1 ? 1 : c;
}
// JointShrink keeps the group of a step in registers up to this many items (the instance is compiled for exactly this many: the
// largest of 4, 8 and 16 that leaves complex128 in the 4-scalar form without scratch and without spills -- 16 spills scalar registers, one address per item)
constexpr int kJointReg = 8;
// ---- the tile form of the same two calls (JointTile / GroupNormsTile, ndwt_device_joint_tile.h): a workgroup takes a STRIP of
// kJointTileSW consecutive steps of one band and walks all items, kJointTileJ of them at a time through an LDS tile, so that a band of
// short items gets steps / kJointTileSW workgroups whose 256 threads all load, where joint_chunks gives it steps / 256 whose threads each
// chase the items one behind the other.  The values are the same bits (the sum of a group still runs over the items in ascending order).
constexpr int kJointTileSW = 8, kJointTileJ = 128;
// the strips (workgroups) per band
constexpr long long joint_tile_strips(long long item_scalars, int comp, bool vec) {
    return ((vec ? item_scalars / 4 : item_scalars / comp) + kJointTileSW - 1) / kJointTileSW;
}
// Which form a launch takes.  variant_inv 11 forces the tile form wherever a launch can number its workgroups, 9 never takes it (A/B
// runs and the tests), anything else is the measured default.  With fewer than kJointTileFrom items the tile form is never taken
// unasked: up to kJointReg items the register form runs at the copy rate, and a pass of the tile form loads 256 / kJointTileSW items.
// Measured on the MI355X (tools/bench_joint_tile.py, batches of real signals in the 4-scalar form, us per call, tile form / chunk form,
// ONE rule for the shrink and for the norms; the full table is in DESIGN.md 4.3h and profiles/bench_joint_tile.txt).  Float, level 1:
//   items   1024 scalars               4096 scalars               16384 scalars              65536 scalars
//   16      shrink 16.5 / 21.4 (0.77)  16.3 / 22.2 (0.73)         16.2 / 22.4 (0.73)         22.6 / 22.2 (1.02)
//           norms   9.9 /  8.2 (1.20)   9.7 / 11.6 (0.84)         11.5 / 11.6 (0.99)         26.3 / 11.6 (2.27)
//   64      shrink 16.4 / 41.9 (0.39)  16.4 / 45.0 (0.36)         18.3 / 42.0 (0.43)         26.6 / 40.8 (0.65)
//           norms  10.5 / 17.9 (0.58)   9.7 / 21.0 (0.46)         12.1 / 21.2 (0.57)         29.3 / 22.2 (1.32)
//   256     shrink 18.9 / 125.1 (0.15) 19.8 / 120.9 (0.16)        22.7 / 121.1 (0.19)        62.5 / 167.6 (0.37)
//           norms  11.6 / 54.9 (0.21)  11.8 / 58.6 (0.20)         14.6 / 62.4 (0.23)         42.8 / 91.8 (0.47)
//   4096    shrink 78.4 / 2386.6 (0.03) 95.3 / 2209.1 (0.04)      (1024 items: 71.6 / 583.5 (0.12); norms 35.7 / 336.5 (0.11))
//           norms  59.2 / 1315.2 (0.05) 55.0 / 1342.0 (0.04)
// Double and level 4 (5 bands) give the same picture; the worst ratios of the cells the rule takes are the norms of 64 items of 16384
// scalars at level 4, 0.86 (float) and 0.68 (double), and of 256 items of 65536, 0.56 (double).  By the rule of DESIGN.md 4.3b -- a
// form is taken unasked only where it was measured at least 10 % below the other, twice the 5 % spread between boxes -- the tile form
// takes bands of up to kJointTileMaxSteps steps from kJointTileFrom items on and bands of up to kJointTileMaxStepsMany steps from
// kJointTileManyFrom items on.  At 64 items of 65536 scalars the shrink wins (0.63 .. 0.74) but the norms lose (1.03 .. 1.47: thousands
// of strips of 64 items each end in a tree and a partial), and the rule is one for both.  With 16 items only the 4096-scalar cells
// qualify (0.72 .. 0.88); fewer than kJointTileFrom items keep the chunk form whatever was measured.  Longer items than 65536 scalars were not measured and keep the
// chunk form; more items than measured at a length take the tile form (the chunk form's chain of loads grows with the items, a
// strip's work does not change shape).  The element-wise form was not measured and is on request only; complex data were not
// measured: their steps are counted like those of real data.
enum JointRoute { kJointChunks, kJointTile };
constexpr long long kJointTileFrom = 64, kJointTileMaxSteps = 4096;                    // from 64 items on: bands of up to 4096 steps
constexpr long long kJointTileManyFrom = 256, kJointTileMaxStepsMany = 16384;          // from 256 items on: bands of up to 16384 steps
constexpr JointRoute joint_route(long long item_scalars, int comp, bool vec, long long bands, long long items, int num_cus, int variant_inv) {
    if (variant_inv == kInvCascadeOff || bands < 1 || bands * joint_tile_strips(item_scalars, comp, vec) > 0x7fffffffLL) return kJointChunks;
    if (variant_inv == kInvCascadeAlways) return kJointTile;
    (void)num_cus;                                            // (the table holds for the one device it was measured on)
    const long long steps = vec ? item_scalars / 4 : item_scalars / comp;
    return vec && ((items >= kJointTileFrom && steps <= kJointTileMaxSteps) || (items >= kJointTileManyFrom && steps <= kJointTileMaxStepsMany)) ? kJointTile
                                                                                                                                                  : kJointChunks;
}
// ---- neighbourhood shrinkage (NeighShrink, ndwt_device_neigh.h): a workgroup of 256 threads owns a tile of the leading filtered axes of
// one item of one band and marches along the last one.  The tile: a row of a wave along axis 0; for 3 filtered axes 64 x 16 positions,
// 4 a thread -- 64 x 8 for elements of 16 bytes (complex128), and for elements of 8 bytes at radius 3, whose ring and waiting centres
// would not fit the 128 registers of 4 waves per SIMD otherwise (they spill 16); below 3 axes a line of 256 positions, one a thread.  What the halo costs is in DESIGN.md 4.3j.
constexpr int neigh_tx(int nd) { return nd == 3 ? 64 : 256; }
constexpr int neigh_ty(int nd, int elem_bytes, int r) { return nd != 3 ? 1 : elem_bytes <= 4 || (elem_bytes <= 8 && r < 3) ? 16 : 8; }
// The grid: the tiles of an item, and the chunks of the march.  A chunk reads 2r planes more than it writes, so the march is split only
// while the launch has fewer workgroups than kNeighRounds per compute unit -- ndwt_plan_set_tuning's target_blocks > 0 stands in for
// that count -- and never into chunks of fewer than 2r + 1 planes.  One filtered axis: no march, one chunk.  blocks: bands * items of
// the launch.
struct NeighGeom { long long ntx, nty, chunk, nchunks; };
constexpr int kNeighRounds = 8;
constexpr NeighGeom neigh_geometry(int nd, long long n0, long long n1, long long n2, int elem_bytes, int r, long long blocks, int num_cus, int target_blocks) {
    const long long tx = neigh_tx(nd), ty = neigh_ty(nd, elem_bytes, r);
    const long long ntx = (n0 + tx - 1) / tx, nty = nd == 3 ? (n1 + ty - 1) / ty : 1, nm = nd == 1 ? 1 : nd == 2 ? n1 : n2;
    const long long tiles = ntx * nty * blocks, want = target_blocks > 0 ? target_blocks : (long long)num_cus * kNeighRounds;
    long long c = (want + tiles - 1) / tiles;
    if (c > nm / (2 * r + 1)) c = nm / (2 * r + 1);
    if (c < 1) c = 1;
    const long long chunk = (nm + c - 1) / c;
    return {ntx, nty, chunk, (nm + chunk - 1) / chunk};
}

// ---- one fused 3-D launch
struct Fused3Query {
    bool f64, inverse, vec4, uniform_yz, tfold;   // vec4: rows, strides and pointers in whole groups of 4 scalars; tfold: 4-D analysis with the t axis folded in
    int Lp, len[3];                    // padded tap length; the three axes' own
    int ew, dil;                       // scalars per x element (2: interleaved complex or a level dilated by 2, 4: dilated by 4); tap stride
    int n1, n2, nbatch;                // scalars along x, rows and batch items of the launch (one sub-lattice of a dilated level)
    int variant_fwd, variant_inv, num_cus, target_blocks;
};
// what a launch runs: the instance by its full name (ndwt_fused_list.h), and the geometry the host lays out for it
struct Fused3Pick : Fused3Instance {
    int TX, TY;                        // the instance's tile
    int per_cu, target;                // workgroups per CU the grid is sized for; target workgroups of fused3_geometry
};

// the tile an instance runs on: read from the table the kernels are compiled from (Inv3Y: 1024 threads, 4 waves per SIMD, no y items)
struct TileShape { int TX, TY, NT, RY, WPE; };
template <typename T, bool INV, int V> constexpr TileShape tile_of() {
    return {Fused3Tile<T, INV, V>::TX, Fused3Tile<T, INV, V>::TY, Fused3Tile<T, INV, V>::NT, Fused3Tile<T, INV, V>::RY, Fused3Tile<T, INV, V>::WPE};
}
template <typename T, int V> constexpr TileShape tile_of(bool inverse) { return inverse ? tile_of<T, true, V>() : tile_of<T, false, V>(); }
constexpr TileShape fused3_tile_shape(Fused3Kernel kernel, bool f64, int V, int Lp, int ew) {
    const bool inverse = kernel != kFwd3;
    if (kernel == kInv3Y) return {inv3y_tx(Lp, ew), inv3y_ty(Lp, ew), 1024, 0, 4};
    if (f64) return V == 0 ? tile_of<double, 0>(inverse) : V == 1 ? tile_of<double, 1>(inverse) : V == 3 ? tile_of<double, 3>(inverse)
                  : V == 5 ? tile_of<double, 5>(inverse) : TileShape{0, 0, 0, 0, 0};
    if (V == 4 || V == 6) return (V == 4) != inverse ? TileShape{0, 0, 0, 0, 0} : inverse ? tile_of<float, true, 4>() : tile_of<float, false, 6>();
    return V == 0 ? tile_of<float, 0>(inverse) : V == 1 ? tile_of<float, 1>(inverse) : V == 2 ? tile_of<float, 2>(inverse)
         : V == 3 ? tile_of<float, 3>(inverse) : TileShape{0, 0, 0, 0, 0};   // no such tile: the launcher's geometry check answers -2
}

inline Fused3Pick fused3_select(const Fused3Query& q) {
    const int L = q.Lp, vf = q.variant_fwd, vi = q.variant_inv;
    const bool f32 = !q.f64, plain = q.ew == 1;
    Fused3Instance k = fwd3_instance(q.f64, L, 0, q.vec4, q.ew, false, false, 0);
    if (q.inverse) {
        // A level dilated by 2 on real data is the interleaved-pair form of Inv3Y (the two x sub-lattices are its (re, im) halves); the
        // whole-lane-shift form of tap stride 4 exists for 16-byte-aligned data only: anything else keeps Inv3S<.., EW = 4>
        const bool use_y = (q.dil == 1 || ((q.dil == 2 || (q.dil == 4 && q.vec4)) && vi != kInvDilatedKeep3S)) &&
                           inv3y_ok(q.f64, q.dil > 1 ? 1 : q.ew, q.len, L, (long long)q.n1 * q.n2 * q.dil, vi);
        const int want = vi == kInvDepth1 ? 1 : 2;          // register sets of band loads, where the instance has them
        const auto y = [&](int depth, bool uniyz, bool scatter) { return inv3y_instance(L, q.vec4, q.ew, depth, uniyz, scatter); };
        if (use_y) {
            // the x stage in scatter form: real data from 10 taps on rows of whole groups of 4, interleaved pairs the same, tap stride 4 for
            // 8 taps; kInvScatter: wherever the form exists, kInvGather: nowhere (measurements: DESIGN.md 4, "how a kernel is chosen").
            // Which depths and forms exist, and why, is in the lists of ndwt_fused_list.h: the wanted depth where there is such an instance,
            // one register set otherwise (a scatter form of 8 .. 12 taps has two sets only: kInvDepth1 runs the gather form there); the
            // shared y / z tap pairs wherever the instance has them (gather form: unless kInvNoUniYZ)
            const bool ask = vi == kInvScatter || (vi != kInvGather && L >= (q.ew == 4 ? 8 : 10));
            const bool scatter = ask && (inv3y_instantiated(y(want, false, true)) || inv3y_instantiated(y(1, false, true)));
            const int depth = (want == 2 && inv3y_instantiated(y(2, false, scatter))) ? 2 : 1;
            k = y(depth, q.uniform_yz && (scatter || vi != kInvNoUniYZ) && inv3y_instantiated(y(depth, true, scatter)), scatter);
        } else if (L > 12 && plain) {
            k = inv3s_instance(kInv3S, q.f64, L, f32 ? 2 : 5, q.vec4, 1);   // 14 / 16 taps
        } else if (plain && vi == kInvLds && L == 8) {
            k = inv3s_instance(kInv3, q.f64, L, 3, q.vec4, 1);
        } else {
            // the lane-shift kernel: float on the tall tile (x taps over 4 scalars: 64x16, 512 threads; long filters: 512 threads x 2 items),
            // double 64x16 (10 / 12 taps: 64x8)
            k = inv3s_instance(kInv3S, q.f64, L, f32 ? (q.ew == 4 ? 4 : (L == 12 || (q.ew == 2 && L == 10)) ? 2 : 1) : (L >= 10 ? 5 : 1), q.vec4, q.ew);
        }
    } else if (q.f64) {
        // double, 6 / 8 taps: 64x16 tile with 512 threads, one column per thread; kFwdSmallTile keeps 64x8 / 256.  Complex db4 the same; 10 taps 64x16, 12: 64x8 / 512
        const bool col68 = (vf == kFwdDefault || vf == kFwdOneColumn) && L >= 6 && L <= 8;
        if (L > 12 && plain) k.V = 5;
        else k.V = q.ew == 2 ? (L >= 10 ? 5 : L == 8 ? 1 : 0) : (L == 12 ? 5 : (L == 10 || col68) ? 1 : 0);
        // two of the z-window slots in LDS (Fwd3 WLDS) on rows of whole groups of 4: 16 taps -- no spills (13 without); complex128 db6 --
        // 2 spilled registers instead of 16
        k.wlds = (q.vec4 && (plain ? L == 16 : L == 12)) ? 2 : 0;
    } else {
        // float (and complex64), 6 / 8 taps: the tall 64x32 tile with 1024 threads where the volume has the tiles to fill the chip with it
        const bool tall68 = L >= 6 && L <= 8 && (long long)((q.n1 + 63) / 64) * ((q.n2 + 31) / 32) * q.nbatch >= 32;
        const int v = (vf == kFwdDefault || vf == kFwdNoPin) ? (tall68 ? kFwdTall : kFwdDefault) : vf;
        if (q.tfold) {
            if (!q.vec4) k.kernel = kNoFused3;
            k.V = 6, k.tpre = true;                           // the folded t axis runs on the tall tile with y items of 2 rows
        } else if (plain && vf == kFwdDefault && L >= 10 && L <= 14 && q.vec4 && padding_even(q.len, L)) {
            // real data, 10 / 12 / 14 taps, rows of whole groups of 4, even padding: the tall-tile kernel with its taps pinned in SGPRs
            k.V = 6, k.pin = true;
        } else if (plain && L > 12) {
            // 14 / 16 taps: the tall tile with y items of 2 rows; 18 / 20 (kFwdOneColumn: all): 64x16 with 512 threads, one column per thread
            k.V = (vf != kFwdOneColumn && L <= 16) ? 6 : 1;
            // Slots of the z window in LDS (Fwd3 WLDS) take the spills out; kFwdSmallTile: the spilling forms without them.
            // tall tile, 16 taps on rows of whole groups of 4: two of the 16 slots -- 512^3 db8 analysis 1.53 -> 1.16 ms per launch,
            // bit-identical (pinned taps on top: 1.20, not used).
            // 512 threads, 20 taps: 4 of the 20 slots of each of a thread's two columns -- the tile without its 18 spilled registers:
            // 512^3 db10 analysis 2.79 -> 1.95 ms per launch, bit-identical; 18 taps do not spill and gain nothing from it.  Ragged rows:
            // 2 / 6 slots for 18 / 20 taps, no spills (8 / 33 without)
            if (vf != kFwdSmallTile) k.wlds = k.V == 6 ? ((L == 16 && q.vec4) ? 2 : 0) : L == 20 ? (q.vec4 ? 4 : 6) : (L == 18 && !q.vec4) ? 2 : 0;
        } else if (q.ew == 4) k.V = 1;
        else if (q.ew == 2) k.V = L >= 10 ? 1 : (q.dil == 1 && vf == kFwdDefault && tall68) ? 2 : 0;
        // real data by tap length: 256 threads up to 8 taps, the tall tile for 10, with y items of 2 rows for 12; on request the tall tile
        // (any length), one column per thread (10 / 12 taps) or y items of 2 rows (8 .. 12 taps: no other instance exists)
        else if (v == kFwdTallRY2 && L < 8) k.kernel = kNoFused3;
        else k.V = v == kFwdTall ? 2 : (v == kFwdOneColumn && L >= 10) ? 1 : v == kFwdTallRY2 ? 6 : (L <= 8 ? 0 : L == 10 ? 2 : 6);
    }
    const TileShape tile = fused3_tile_shape(k.kernel, q.f64, k.V, L, q.ew);
    // one round of resident workgroups: synthesis 1 per CU (the 256-thread LDS kernel 3), analysis 2, 1024-thread tiles 1
    const int per_cu = q.inverse ? ((k.kernel == kInv3 && f32) ? 3 : 1) : ((q.dil == 4 || (f32 && tile.TY == 32)) ? 1 : 2);
    return {k, tile.TX, tile.TY, per_cu, q.target_blocks > 0 ? q.target_blocks : q.num_cus * per_cu};
}

// ---- one fused 2-D launch
constexpr int fused2_tile_width(bool inverse, int Lp, int ew) { return wave_row_width(inverse, Lp, ew, false, 1); }
struct Fused2Query {
    bool f64, inverse, vec4;
    int Lp, ew, dil, n1, n2;           // n1: scalars along x; n2: rows of the whole (undilated) image
    int variant_inv;
    int nbatch = 1;                    // images of the launch (a stack: its items)
};
enum Fused2Family { kFused2S, kInv2P };   // Fwd2S / Inv2S by direction, or the synthesis with rows of band loads in flight
// what a launch runs: the instance by its full name (ndwt_fused_list.h), flat as Fused3Pick is -- every template argument of Fwd2S /
// Inv2S (family kFused2S) or of Inv2P (kInv2P: synthesis of real data, rows of whole groups of 4) -- and the waves fused2_geometry aims at
struct Fused2Pick {
    Fused2Family family;
    bool inverse, f64, vec4;
    int Lp, ew;
    int wpe;                           // Fwd2S / Inv2S: waves per SIMD (fused2s_wpe)
    int pdepth;                        // Inv2P: rows of band loads in flight
    bool packed;                       // Inv2P: packed FMAs
    int waves;
    constexpr Fused2SInstance fused2s() const { return {inverse, f64, vec4, Lp, ew, wpe}; }
    constexpr Fused2PInstance inv2p() const { return {f64, Lp, pdepth, packed}; }
};
// synthesis of real data in rows of whole groups of 4 scalars, images whose 70-row chunks fit one round of 1024 waves (up to 4096^2): Inv2P,
// 4 rows of band loads in flight per wave, packed FMAs where that form exists (float 4 / 8 / 12 taps); double up to 8 taps, depth 4 for 4 taps.
// A stack: the waves of all its items count against the round.
inline Fused2Pick fused2_select(const Fused2Query& q) {
    const int vi = q.variant_inv, WX = fused2_tile_width(q.inverse, q.Lp, q.ew), L = q.Lp;
    const bool deep = q.inverse && L <= 12 && (!q.f64 || L <= 8) && q.ew == 1 && q.dil == 1 && q.vec4 && vi != kInv2Keep2S && q.n2 >= 64 &&
                      ((long long)((q.n1 + WX - 1) / WX) * ((q.n2 + 69) / 70) * (q.nbatch > 1 ? q.nbatch : 1) <= 1280 || vi != kInvDefault);
    const int waves = (deep && vi != kInv2Depth2Geom && vi != kInv2Depth4Geom) ? 1024 : 2048;
    if (!deep) return {kFused2S, q.inverse, q.f64, q.vec4, L, q.ew, fused2s_wpe(q.f64, L, q.ew), 0, false, waves};
    const bool d4 = q.f64 ? L == 4 : (vi != kInv2Depth2Geom && vi != kInv2Depth2Round && (L == 4 || L == 8 || L == 12));
    return {kInv2P, true, q.f64, true, L, 1, 0, d4 ? 4 : 2, !q.f64 && d4 && vi != kInv2Unpacked, waves};
}

}  // namespace ndwt
