// ndwt_fused_list.h -- the instances of the fused kernels that kernel selection can name, one list per launch unit (no HIP header: the
// launch units expand a list into launches, ndwt_select.h and the host tests into questions).  An instance lives in exactly one list: the
// unit decides how its device code is compiled (csrc/Makefile: NOSLP), and the split over units is what keeps the build parallel.  Every
// fused family is here: the 3-D kernels, the one-level 2-D ones (Fwd2S / Inv2S, Inv2P) and the 2-D cascade -- and, since a pass along one
// axis is picked the same way (ndwt_select.h: axis_select), the two per-axis families AxisMarch and AxisX.
#pragma once
#include "ndwt_fused_tile.h"

namespace ndwt {

// ---- the full name of a fused 3-D instance: every template argument of the kernel that runs
enum Fused3Kernel { kFwd3, kInv3, kInv3S, kInv3Y, kNoFused3 };
struct Fused3Instance {
    Fused3Kernel kernel;
    bool f64, vec4;                    // vec4: rows, strides and pointers in whole groups of 4 scalars
    int Lp, ew;                        // padded tap length; scalars the x taps step over
    int V;                             // Fwd3 / Inv3 / Inv3S: index into Fused3Tile (TX, TY, NT, RY, WPE)
    bool pin, tpre;                    // Fwd3: taps pinned in SGPRs; the t axis of a 4-D level folded in
    int wlds;                          // Fwd3: slots of the z window kept in LDS
    int depth;                         // Inv3Y: register sets of band loads (ZLDS follows: inv3y_zlds)
    bool uniyz, scatter;               // Inv3Y: shared y / z tap pairs; the x stage in scatter form
};
constexpr bool operator==(const Fused3Instance& a, const Fused3Instance& b) {
    return a.kernel == b.kernel && a.f64 == b.f64 && a.vec4 == b.vec4 && a.Lp == b.Lp && a.ew == b.ew && a.V == b.V && a.pin == b.pin &&
           a.tpre == b.tpre && a.wlds == b.wlds && a.depth == b.depth && a.uniyz == b.uniyz && a.scatter == b.scatter;
}
constexpr Fused3Instance fwd3_instance(bool f64, int L, int V, bool vec4, int ew, bool pin, bool tpre, int wlds) {
    return {kFwd3, f64, vec4, L, ew, V, pin, tpre, wlds, 0, false, false};
}
constexpr Fused3Instance inv3s_instance(Fused3Kernel kernel, bool f64, int L, int V, bool vec4, int ew) {
    return {kernel, f64, vec4, L, ew, V, false, false, 0, 0, false, false};
}
constexpr Fused3Instance inv3y_instance(int L, bool vec4, int ew, int depth, bool uniyz, bool scatter) {
    return {kInv3Y, false, vec4, L, ew, 0, false, false, 0, depth, uniyz, scatter};
}
// Fwd2S / Inv2S<T, Lp, VEC4, WPE, EW>: one level of an image, one wave per tile, registers only
enum Fused2SKind { kFwd2S, kInv2S };
struct Fused2SInstance { bool inverse, f64, vec4; int Lp, ew, wpe; };
constexpr bool operator==(const Fused2SInstance& a, const Fused2SInstance& b) {
    return a.inverse == b.inverse && a.f64 == b.f64 && a.vec4 == b.vec4 && a.Lp == b.Lp && a.ew == b.ew && a.wpe == b.wpe;
}
// waves per SIMD an instance is compiled for (its register budget: 4 -> 128, 2 -> 256): the y window / the pending sums of a wave grow
// with the tap length, twice as fast in double and with the x taps stepping over pairs; the 128-register forms of these would spill
constexpr int fused2s_wpe(bool f64, int Lp, int ew) { return (f64 || (ew == 1 ? Lp >= 14 : (ew == 2 && Lp >= 10))) ? 2 : 4; }
struct Fused2PInstance { bool f64; int Lp, pdepth; bool packed; };   // Inv2P<T, Lp, PD, 2, PK>
constexpr bool operator==(const Fused2PInstance& a, const Fused2PInstance& b) {
    return a.f64 == b.f64 && a.Lp == b.Lp && a.pdepth == b.pdepth && a.packed == b.packed;
}
// Fwd2C<T, Lp, nlev, WPE, ew> (pd = 0) / Inv2C<T, Lp, nlev, pd, WPE, ew>: two or three levels of an image in one launch
struct Cascade2Instance { bool inverse, f64; int ew, Lp, nlev, pd; };
constexpr bool operator==(const Cascade2Instance& a, const Cascade2Instance& b) {
    return a.inverse == b.inverse && a.f64 == b.f64 && a.ew == b.ew && a.Lp == b.Lp && a.nlev == b.nlev && a.pd == b.pd;
}
// Fwd1C / Inv1C<T, Lp, nlev, ew> (ndwt_device_1d.h): two to four levels of many 1-D signals in one launch
struct Cascade1Instance { bool inverse, f64; int ew, Lp, nlev; };
constexpr bool operator==(const Cascade1Instance& a, const Cascade1Instance& b) {
    return a.inverse == b.inverse && a.f64 == b.f64 && a.ew == b.ew && a.Lp == b.Lp && a.nlev == b.nlev;
}
// Den1C<T, Lp, nlev, ew> (ndwt_device_1d.h): dec, per-band thresholding and rec of one to four levels of many 1-D signals in one launch
struct Den1Instance { bool f64; int ew, Lp, nlev; };
constexpr bool operator==(const Den1Instance& a, const Den1Instance& b) { return a.f64 == b.f64 && a.ew == b.ew && a.Lp == b.Lp && a.nlev == b.nlev; }
// FwdMC / InvMC<T, L, nlev> (ndwt_device_axis.h): two to four levels of one strided axis inside one march (interleaved complex: the
// factor 2 in the inner block, no instance of its own)
struct CascadeMInstance { bool inverse, f64; int L, nlev; };
constexpr bool operator==(const CascadeMInstance& a, const CascadeMInstance& b) {
    return a.inverse == b.inverse && a.f64 == b.f64 && a.L == b.L && a.nlev == b.nlev;
}
// AxisMarch<T, L, SYN> (ndwt_device.h): one pass along one strided axis, the filter window in registers
struct AxisMarchInstance { bool f64, syn; int L; };
constexpr bool operator==(const AxisMarchInstance& a, const AxisMarchInstance& b) { return a.f64 == b.f64 && a.syn == b.syn && a.L == b.L; }
// AxisX<T, L, SYN, EW, VEC4> (ndwt_device.h): one pass along the contiguous axis, one wave per row segment
struct AxisXInstance { bool f64, syn, vec4; int L, ew; };
constexpr bool operator==(const AxisXInstance& a, const AxisXInstance& b) {
    return a.f64 == b.f64 && a.syn == b.syn && a.vec4 == b.vec4 && a.L == b.L && a.ew == b.ew;
}

// ---- the lists.  Entries:  F(T, L, V, VEC4, EW, PIN, TPRE, WLDS)  Fwd3 on tile V
//                            S(KIND, T, L, V, VEC4, EW)             Inv3 / Inv3S on tile V
//                            Y(L, VEC4, EW, DEPTH, UNIYZ, XSC)      Inv3Y (float)
//                            W(KIND, T, L, VEC4, WPE, EW)           Fwd2S / Inv2S
//                            P(T, L, PD, PK)                        Inv2P
//                            A(T, EW, L, NLEV, WPE)                 Fwd2C
//                            R(T, EW, L, NLEV, PD, WPE)             Inv2C
//                            C(KIND, T, EW, L, NLEV)                Fwd1C / Inv1C
//                            M(KIND, T, L, NLEV)                    FwdMC / InvMC
//                            D(T, EW, L, NLEV)                      Den1C
//                            N(T, L, SYN)                           AxisMarch
//                            X(T, L, SYN, EW, VEC4)                 AxisX
// NDWT_F2 / NDWT_S2 / NDWT_Y2 / NDWT_W2: the plain form of an entry for rows of whole groups of 4 scalars and for the rest
#define NDWT_F2(F, T, L, V, EW) F(T, L, V, true, EW, false, false, 0) F(T, L, V, false, EW, false, false, 0)
#define NDWT_S2(S, KIND, T, L, V, EW) S(KIND, T, L, V, true, EW) S(KIND, T, L, V, false, EW)
#define NDWT_Y2(Y, L, EW, DEPTH) Y(L, true, EW, DEPTH, false, false) Y(L, false, EW, DEPTH, false, false)
#define NDWT_W2(W, KIND, T, L, WPE, EW) W(KIND, T, L, true, WPE, EW) W(KIND, T, L, false, WPE, EW)

// float analysis: 256-thread kernel for tap lengths <= 8, the tall 64x32 tile with 1024 threads for 10 and 12 (and 14, 16:
// ndwt_fused3_f32_long.hip); tile 1 = 512 threads, one column per thread (A/B; the kernel of interleaved complex data with 10 .. 16 taps)
#define NDWT_LIST_F32_FWD(F)                                                                                              \
    NDWT_F2(F, float, 2, 1, 4) NDWT_F2(F, float, 4, 1, 4) NDWT_F2(F, float, 6, 1, 4) NDWT_F2(F, float, 8, 1, 4)           \
    NDWT_F2(F, float, 6, 2, 2) NDWT_F2(F, float, 8, 2, 2)   /* interleaved complex on the tall tile */                    \
    NDWT_F2(F, float, 2, 0, 2) NDWT_F2(F, float, 4, 0, 2) NDWT_F2(F, float, 6, 0, 2) NDWT_F2(F, float, 8, 0, 2)           \
    NDWT_F2(F, float, 10, 1, 2) NDWT_F2(F, float, 12, 1, 2) NDWT_F2(F, float, 14, 1, 2) NDWT_F2(F, float, 16, 1, 2)       \
    NDWT_F2(F, float, 2, 0, 1) NDWT_F2(F, float, 4, 0, 1) NDWT_F2(F, float, 6, 0, 1) NDWT_F2(F, float, 8, 0, 1)           \
    NDWT_F2(F, float, 2, 2, 1) NDWT_F2(F, float, 4, 2, 1) NDWT_F2(F, float, 6, 2, 1) NDWT_F2(F, float, 8, 2, 1)           \
    NDWT_F2(F, float, 10, 2, 1)   /* 10 .. 16 taps: the tall tile (db6 analysis 1.33 -> 1.02 ms per launch) */            \
    NDWT_F2(F, float, 12, 2, 1)                                                                                           \
    NDWT_F2(F, float, 10, 1, 1) NDWT_F2(F, float, 12, 1, 1)                                                               \
    NDWT_F2(F, float, 8, 6, 1) NDWT_F2(F, float, 10, 6, 1)                                                                \
    NDWT_F2(F, float, 12, 6, 1)   /* 12 .. 16 taps: y items of 2 rows (10 of the 16 waves in the y stage instead of 5: db6 -6 %) */
// float real, 10 / 12 / 14 taps: tall tile with y items of 2 rows, taps pinned in SGPRs (Fwd3 PIN)
#define NDWT_LIST_F32_FWDP(F) F(float, 10, 6, true, 1, true, false, 0) F(float, 12, 6, true, 1, true, false, 0) F(float, 14, 6, true, 1, true, false, 0)
// 4-D analysis with the t axis folded in (Fwd3 TPRE): the tall tile with y items of 2 rows (the 8 prefetched frames fit its register
// budget), rows of whole groups of 4 scalars
#define NDWT_LIST_F32_DEN(F) \
    F(float, 2, 6, true, 1, false, true, 0) F(float, 4, 6, true, 1, false, true, 0) F(float, 6, 6, true, 1, false, true, 0) F(float, 8, 6, true, 1, false, true, 0)
// float analysis, 14 / 16 taps on the tall 64x32 tile with 1024 threads (db7 analysis 1.45 -> 1.15 ms per launch; 16 taps on ragged rows
// spill 8 registers); 16 taps on rows of whole groups of 4 with two of the 16 slots of the z window in LDS
#define NDWT_LIST_F32_LONG(F) NDWT_F2(F, float, 14, 6, 1) NDWT_F2(F, float, 16, 6, 1) F(float, 16, 6, true, 1, false, false, 2)
// float analysis, 14 .. 20 taps on the 512-thread 64x16 tile (256-register budget); 20 taps with 4 (ragged rows: 6) window slots of each of
// a thread's two columns in LDS, 18 taps on ragged rows with 2 (the plain 20-tap form spills 18 of its 256 registers)
#define NDWT_LIST_F32_LONGB(F)                                                                                            \
    NDWT_F2(F, float, 14, 1, 1) NDWT_F2(F, float, 16, 1, 1) NDWT_F2(F, float, 18, 1, 1) NDWT_F2(F, float, 20, 1, 1)       \
    F(float, 20, 1, true, 1, false, false, 4) F(float, 18, 1, false, 1, false, false, 2) F(float, 20, 1, false, 1, false, false, 6)
// float synthesis other than the pair-packed kernel (ndwt_fused3_f32_invy*.hip, the default wherever it applies): the lane-shift
// kernel Inv3S on a tall 64x32 tile (1024 threads, one workgroup per CU; db6: 512 threads with two items each -- the 1024-thread
// form spills there) for mixed wavelets with odd tap padding, dilated levels and A/B runs; the LDS kernel Inv3 (A/B, db4 only)
#define NDWT_LIST_F32_INV(S)                                                                                              \
    NDWT_S2(S, Inv3, float, 8, 3, 1)                                                                                      \
    NDWT_S2(S, Inv3S, float, 2, 1, 1) NDWT_S2(S, Inv3S, float, 4, 1, 1) NDWT_S2(S, Inv3S, float, 6, 1, 1) NDWT_S2(S, Inv3S, float, 8, 1, 1) \
    NDWT_S2(S, Inv3S, float, 10, 1, 1)                                                                                    \
    NDWT_S2(S, Inv3S, float, 12, 2, 1)   /* db6: 512 threads x 2 items, no spills (1.78 vs 2.05 ms) */
#define NDWT_LIST_F32_INVE(S)                                                                                             \
    NDWT_S2(S, Inv3S, float, 2, 4, 4) NDWT_S2(S, Inv3S, float, 4, 4, 4) NDWT_S2(S, Inv3S, float, 6, 4, 4) NDWT_S2(S, Inv3S, float, 8, 4, 4) \
    NDWT_S2(S, Inv3S, float, 2, 1, 2) NDWT_S2(S, Inv3S, float, 4, 1, 2) NDWT_S2(S, Inv3S, float, 6, 1, 2) NDWT_S2(S, Inv3S, float, 8, 1, 2) \
    NDWT_S2(S, Inv3S, float, 10, 2, 2)   /* complex db5 / db6: 512 threads x 2 items (db6 spills 42 of 256 registers) */  \
    NDWT_S2(S, Inv3S, float, 12, 2, 2)
// float synthesis, 14 / 16 taps: the lane-shift kernel on the 64x32 tile with 512 threads x 2 items
#define NDWT_LIST_F32_LONGI(S) NDWT_S2(S, Inv3S, float, 14, 2, 1) NDWT_S2(S, Inv3S, float, 16, 2, 1)

// The pair-packed synthesis, real data.  Depth 2 (two register sets of band loads, staggered refill) exists where it fits the 128
// registers of a 1024-thread workgroup without spills: tap lengths 2, 8 and 10 as they are; 12 with 6 of the pending z sums in LDS
// (inv3y_zlds; 4 and 6 taps fit that way too and run slower than depth 1; a spill reload in the plane loop would wait vmcnt(0), i.e. for
// every load in flight).  On rows that are not whole groups of 4 scalars (the VEC4 = false instance keeps 4 offsets per lane) 2 and 8
// taps fit, 10 and 12 would spill.
// UNIYZ (the same taps on the y and z axes, rows of whole groups of 4, 12 .. 20 taps): the z stage reads the y tap pairs (L fewer SGPRs
// held: 512^3 synthesis db6 -1.8 %, db10 -2.4 % per launch, identical results).  8 taps: -0.6 % on cfg3 and +1.2 % on cfg5's batched
// volumes in interleaved A/B runs -- within noise of each other, so the 8- and 10-tap kernels stay as they were.
#define NDWT_LIST_F32_INVY_DB4(Y) NDWT_Y2(Y, 8, 1, 2) NDWT_Y2(Y, 8, 1, 1)
#ifdef NDWT_INVY_DB4_ONLY
#define NDWT_LIST_F32_INVY(Y) NDWT_LIST_F32_INVY_DB4(Y)
#else
#define NDWT_LIST_F32_INVY(Y)                                                                                             \
    NDWT_LIST_F32_INVY_DB4(Y)                                                                                             \
    Y(12, true, 1, 2, true, false) Y(14, true, 1, 1, true, false) Y(16, true, 1, 1, true, false) Y(18, true, 1, 1, true, false) \
    Y(20, true, 1, 1, true, false)                                                                                        \
    NDWT_Y2(Y, 2, 1, 2) NDWT_Y2(Y, 2, 1, 1) NDWT_Y2(Y, 4, 1, 1) NDWT_Y2(Y, 6, 1, 1)                                        \
    Y(10, true, 1, 2, false, false) NDWT_Y2(Y, 10, 1, 1) Y(12, true, 1, 2, false, false) NDWT_Y2(Y, 12, 1, 1)             \
    NDWT_Y2(Y, 14, 1, 1) NDWT_Y2(Y, 16, 1, 1)                                                                             \
    NDWT_Y2(Y, 18, 1, 1)   /* 64 x 24 tile: 41 haloed rows on 14 waves */                                                 \
    NDWT_Y2(Y, 20, 1, 1)   /* 48 x 28 tile: 47 haloed rows on 16 waves (3 spilled registers, reloaded once per plane) */
#endif
// ... with its x stage in scatter form: rows of whole groups of 4 scalars; two register sets up to 12 taps, one from 14
#define NDWT_LIST_F32_INVYS(Y)                                                                                            \
    Y(8, true, 1, 2, false, true) Y(10, true, 1, 2, false, true) Y(12, true, 1, 2, false, true) Y(12, true, 1, 2, true, true) \
    Y(14, true, 1, 1, false, true) Y(14, true, 1, 1, true, true) Y(16, true, 1, 1, false, true) Y(16, true, 1, 1, true, true) \
    Y(18, true, 1, 1, false, true) Y(18, true, 1, 1, true, true) Y(20, true, 1, 1, false, true) Y(20, true, 1, 1, true, true)
// ... on interleaved complex data (EW = 2, tap lengths 2 .. 16; depth 2 where it fits 128 registers without spills, as for real data --
// 10 taps: 1 spilled register; 14 / 16 taps: 48-wide tiles), its scatter form on rows of whole groups of 4 scalars from 8 taps, and on a
// level dilated by 4 (EW = 4, rows of whole groups of 4 scalars only; scatter form: the sums walk from lane to lane instead of the samples)
#define NDWT_LIST_F32_INVYC(Y)                                                                                            \
    Y(8, true, 2, 2, false, true) Y(8, true, 2, 1, false, true) Y(10, true, 2, 1, false, true) Y(12, true, 2, 1, false, true) \
    Y(14, true, 2, 1, false, true) Y(16, true, 2, 1, false, true)                                                         \
    Y(2, true, 2, 2, false, false) NDWT_Y2(Y, 2, 2, 1) NDWT_Y2(Y, 4, 2, 1) NDWT_Y2(Y, 6, 2, 1)                             \
    Y(8, true, 2, 2, false, false) NDWT_Y2(Y, 8, 2, 1) NDWT_Y2(Y, 10, 2, 1) NDWT_Y2(Y, 12, 2, 1) NDWT_Y2(Y, 14, 2, 1) NDWT_Y2(Y, 16, 2, 1) \
    Y(4, true, 4, 1, false, true) Y(6, true, 4, 1, false, true) Y(8, true, 4, 2, false, true) Y(8, true, 4, 1, false, true) \
    Y(2, true, 4, 2, false, false) Y(2, true, 4, 1, false, false) Y(4, true, 4, 1, false, false) Y(6, true, 4, 1, false, false) \
    Y(8, true, 4, 2, false, false) Y(8, true, 4, 1, false, false)

// double analysis: 64x8 tile with 256 threads; 6 / 8 taps on request and 10 taps: 64x16 with 512 threads, one column per thread; 12 taps:
// 64x8 with 512 threads, no spills (64x16 spills 137 registers).  Complex128: 8 taps on 64x16 / 512 (the 256-thread tile spills 16
// registers; 256^3: 0.97 -> 0.58 ms per launch), 10 / 12 on 64x8 / 512 (12: 16 spilled registers; on rows of whole groups of 4 two of
// the 12 z-window slots in LDS: 2 spilled registers)
#define NDWT_LIST_F64_FWD(F)                                                                                              \
    F(double, 12, 5, true, 2, false, false, 2)                                                                            \
    NDWT_F2(F, double, 2, 0, 2) NDWT_F2(F, double, 4, 0, 2) NDWT_F2(F, double, 6, 0, 2) NDWT_F2(F, double, 8, 1, 2)       \
    NDWT_F2(F, double, 10, 5, 2) NDWT_F2(F, double, 12, 5, 2)                                                             \
    NDWT_F2(F, double, 6, 1, 1) NDWT_F2(F, double, 8, 1, 1)                                                               \
    NDWT_F2(F, double, 2, 0, 1) NDWT_F2(F, double, 4, 0, 1) NDWT_F2(F, double, 6, 0, 1) NDWT_F2(F, double, 8, 0, 1)       \
    NDWT_F2(F, double, 10, 1, 1) NDWT_F2(F, double, 12, 5, 1)
// double synthesis: the lane-shift kernel on a 64x16 tile with 512 threads; 10 / 12 taps (complex128: 10, 6 spilled registers): 64x8 tile,
// 512 threads, no spills (64x16: 32 / 71 spilled registers); the LDS kernel Inv3 (A/B runs, db4 only)
#define NDWT_LIST_F64_INV(S)                                                                                              \
    NDWT_S2(S, Inv3S, double, 2, 1, 2) NDWT_S2(S, Inv3S, double, 4, 1, 2) NDWT_S2(S, Inv3S, double, 6, 1, 2) NDWT_S2(S, Inv3S, double, 8, 1, 2) \
    NDWT_S2(S, Inv3S, double, 10, 5, 2)                                                                                   \
    NDWT_S2(S, Inv3, double, 8, 3, 1)                                                                                     \
    NDWT_S2(S, Inv3S, double, 2, 1, 1) NDWT_S2(S, Inv3S, double, 4, 1, 1) NDWT_S2(S, Inv3S, double, 6, 1, 1) NDWT_S2(S, Inv3S, double, 8, 1, 1) \
    NDWT_S2(S, Inv3S, double, 10, 5, 1) NDWT_S2(S, Inv3S, double, 12, 5, 1)
// double real, 14 and 16 taps (db7, db8): 64x8 tiles with 512 threads and the 256-register budget (no spills on rows of whole 4-element
// groups; 10 .. 31 spilled registers in the 16-tap analysis and on ragged rows); the 16-tap analysis on rows of whole groups of 4 with two
// of the 16 z-window slots in LDS: no spills (13 without)
#define NDWT_LIST_F64_LONG(F, S)                                                                                          \
    F(double, 16, 5, true, 1, false, false, 2) NDWT_F2(F, double, 14, 5, 1) NDWT_F2(F, double, 16, 5, 1)                  \
    NDWT_S2(S, Inv3S, double, 14, 5, 1) NDWT_S2(S, Inv3S, double, 16, 5, 1)

// One level of an image (Fwd2S / Inv2S): a list serves the analysis unit and the synthesis unit of its tap lengths (KIND = Fwd2S / Inv2S).
// The tap lengths of a kind are split over units because one unit with all of them is the long pole of the build.
// float up to 12 taps at 4 waves per SIMD: real data; up to 8 taps also with the x taps stepping over 2 scalars (interleaved complex64,
// a level dilated by 2) and over 4 (a level dilated by 4).  2 .. 6 taps: ndwt_fused2_f32.hip, ndwt_fused2_f32_inva.hip
#define NDWT_LIST_F32_2S_SHORT(W, KIND)                                                                                   \
    NDWT_W2(W, KIND, float, 2, 4, 4) NDWT_W2(W, KIND, float, 2, 4, 2) NDWT_W2(W, KIND, float, 2, 4, 1)                    \
    NDWT_W2(W, KIND, float, 4, 4, 4) NDWT_W2(W, KIND, float, 4, 4, 2) NDWT_W2(W, KIND, float, 4, 4, 1)                    \
    NDWT_W2(W, KIND, float, 6, 4, 4) NDWT_W2(W, KIND, float, 6, 4, 2) NDWT_W2(W, KIND, float, 6, 4, 1)
// ... 8 .. 12 taps: ndwt_fused2_f32_fwdb.hip, ndwt_fused2_f32_invb.hip
#define NDWT_LIST_F32_2S_MID(W, KIND)                                                                                     \
    NDWT_W2(W, KIND, float, 8, 4, 4) NDWT_W2(W, KIND, float, 8, 4, 2) NDWT_W2(W, KIND, float, 8, 4, 1)                    \
    NDWT_W2(W, KIND, float, 10, 4, 1) NDWT_W2(W, KIND, float, 12, 4, 1)
// float real, 14 .. 20 taps (db7 .. db10): the 256-register budget (2 waves per SIMD), no spills.  Analysis: ndwt_fused2_f32_fwdl.hip;
// synthesis: 14 / 16 in ndwt_fused2_f32_invl.hip, 18 / 20 in ndwt_fused2_f32_invm.hip
#define NDWT_LIST_F32_2S_14_16(W, KIND) NDWT_W2(W, KIND, float, 14, 2, 1) NDWT_W2(W, KIND, float, 16, 2, 1)
#define NDWT_LIST_F32_2S_18_20(W, KIND) NDWT_W2(W, KIND, float, 18, 2, 1) NDWT_W2(W, KIND, float, 20, 2, 1)
// interleaved complex64, 10 .. 16 taps (db5 .. db8): the x taps stepping over (re, im) pairs on the 256-register budget, no spills
// (ndwt_fused2_f32_fwdc.hip, ndwt_fused2_f32_invc.hip)
#define NDWT_LIST_C64_2S_LONG(W, KIND) \
    NDWT_W2(W, KIND, float, 10, 2, 2) NDWT_W2(W, KIND, float, 12, 2, 2) NDWT_W2(W, KIND, float, 14, 2, 2) NDWT_W2(W, KIND, float, 16, 2, 2)
// double on the 256-register budget: real up to 12 taps; complex128 / a level dilated by 2 up to 8 (ndwt_fused2_f64.hip, ndwt_fused2_f64_inv.hip)
#define NDWT_LIST_F64_2S(W, KIND)                                                                                         \
    NDWT_W2(W, KIND, double, 8, 2, 2) NDWT_W2(W, KIND, double, 8, 2, 1) NDWT_W2(W, KIND, double, 10, 2, 1) NDWT_W2(W, KIND, double, 12, 2, 1) \
    NDWT_W2(W, KIND, double, 2, 2, 2) NDWT_W2(W, KIND, double, 2, 2, 1) NDWT_W2(W, KIND, double, 4, 2, 2) NDWT_W2(W, KIND, double, 4, 2, 1) \
    NDWT_W2(W, KIND, double, 6, 2, 2) NDWT_W2(W, KIND, double, 6, 2, 1)
// double real, 14 and 16 taps (db7, db8), both directions in ndwt_fused2_f64_long.hip: the analysis fits the 256-register budget, the
// synthesis spills 22 .. 70 registers (still 3x the per-axis path)
#define NDWT_LIST_F64_2S_LONG(W, KIND) NDWT_W2(W, KIND, double, 14, 2, 1) NDWT_W2(W, KIND, double, 16, 2, 1)
// every list of one direction
#define NDWT_LIST_2S(W, KIND)                                                                                             \
    NDWT_LIST_F32_2S_MID(W, KIND) NDWT_LIST_F32_2S_SHORT(W, KIND) NDWT_LIST_F32_2S_14_16(W, KIND) NDWT_LIST_F32_2S_18_20(W, KIND) \
    NDWT_LIST_C64_2S_LONG(W, KIND) NDWT_LIST_F64_2S(W, KIND) NDWT_LIST_F64_2S_LONG(W, KIND)

// 2-D synthesis with rows of band loads in flight (Inv2P), real data in rows of whole groups of 4 scalars.  float: PD rows in flight per
// wave; packed FMAs on pairs of adjacent x outputs with the tap pairs pinned in SGPRs for 4 / 8 / 12 taps at depth 4.  double: up to 8
// taps fit the 256-register budget without spills (4 rows in flight with 4 taps, 2 otherwise)
#define NDWT_LIST_F32_INV2P(P)                                                                                            \
    P(float, 4, 4, true) P(float, 8, 4, true) P(float, 12, 4, true)                                                       \
    P(float, 2, 2, false) P(float, 4, 2, false) P(float, 4, 4, false) P(float, 6, 2, false) P(float, 8, 2, false) P(float, 8, 4, false) \
    P(float, 10, 2, false) P(float, 12, 2, false) P(float, 12, 4, false)
#define NDWT_LIST_F64_INV2P(P) P(double, 2, 2, false) P(double, 4, 4, false) P(double, 6, 2, false) P(double, 8, 2, false)

// The cascaded 2-D kernels (Fwd2C / Inv2C), rows of whole groups of 4 scalars: THE table of the instances that exist -- cascade2_levels
// (ndwt_select.h) answers from it and the launch units (ndwt_fused2_{f32,c64,f64}_{fwd,inv}cas.hip) expand it.  Every instance runs
// without scratch; WPE = 1 (one wave per SIMD, the 512-register budget) is where two waves per SIMD would spill (DESIGN.md 4.3 has the
// register counts).  NDWT_A23 / NDWT_R23: both level counts of a tap length.
#define NDWT_A23(A, T, EW, L, WPE) A(T, EW, L, 2, WPE) A(T, EW, L, 3, WPE)
#define NDWT_R23(R, T, EW, L, PD, WPE) R(T, EW, L, 2, PD, WPE) R(T, EW, L, 3, PD, WPE)
// float real: 2 .. 8 taps; analysis also 12 taps at two levels (three: 132 spilled registers); synthesis with one or two rows of band
// loads in flight per level
#define NDWT_LIST_F32_FWD2C(A) NDWT_A23(A, float, 1, 2, 2) NDWT_A23(A, float, 1, 4, 2) NDWT_A23(A, float, 1, 6, 2) NDWT_A23(A, float, 1, 8, 2) A(float, 1, 12, 2, 2)
#define NDWT_LIST_F32_INV2C(R)                                                                                            \
    NDWT_R23(R, float, 1, 2, 1, 2) NDWT_R23(R, float, 1, 4, 1, 2) NDWT_R23(R, float, 1, 6, 1, 2) NDWT_R23(R, float, 1, 8, 1, 2) \
    NDWT_R23(R, float, 1, 2, 2, 2) NDWT_R23(R, float, 1, 4, 2, 2) NDWT_R23(R, float, 1, 6, 2, 2) NDWT_R23(R, float, 1, 8, 2, 2)
// interleaved complex64: every tap length and level count at two waves per SIMD; two rows in flight except three levels of 8 taps
// (40 bytes of scratch at two waves per SIMD: that launch keeps one row)
#define NDWT_LIST_C64_FWD2C(A) NDWT_A23(A, float, 2, 2, 2) NDWT_A23(A, float, 2, 4, 2) NDWT_A23(A, float, 2, 6, 2) NDWT_A23(A, float, 2, 8, 2)
#define NDWT_LIST_C64_INV2C(R)                                                                                            \
    NDWT_R23(R, float, 2, 2, 1, 2) NDWT_R23(R, float, 2, 4, 1, 2) NDWT_R23(R, float, 2, 6, 1, 2) NDWT_R23(R, float, 2, 8, 1, 2) \
    NDWT_R23(R, float, 2, 2, 2, 2) NDWT_R23(R, float, 2, 4, 2, 2) NDWT_R23(R, float, 2, 6, 2, 2) R(float, 2, 8, 2, 2, 2)
// double real and complex128: the y windows / pending sums of every level are 8 registers per row, so from 6 taps x 3 levels (analysis)
// and 4 taps x 3 levels (synthesis) on a wave needs the budget of one wave per SIMD; one row of band loads in flight.  Not built: the
// complex128 synthesis of 8 taps x 3 levels (192 bytes of scratch even at one wave per SIMD) -- those three levels run as 2 + 1.
#define NDWT_LIST_F64_FWD2C(A)                                                                                            \
    NDWT_A23(A, double, 1, 2, 2) NDWT_A23(A, double, 1, 4, 2) A(double, 1, 6, 2, 2) A(double, 1, 6, 3, 1) NDWT_A23(A, double, 1, 8, 1)
#define NDWT_LIST_C128_FWD2C(A)                                                                                           \
    NDWT_A23(A, double, 2, 2, 2) NDWT_A23(A, double, 2, 4, 2) A(double, 2, 6, 2, 2) A(double, 2, 6, 3, 1) NDWT_A23(A, double, 2, 8, 1)
#define NDWT_LIST_F64_INV2C(R)                                                                                            \
    NDWT_R23(R, double, 1, 2, 1, 2) R(double, 1, 4, 2, 1, 2) R(double, 1, 4, 3, 1, 1) NDWT_R23(R, double, 1, 6, 1, 1) NDWT_R23(R, double, 1, 8, 1, 1)
#define NDWT_LIST_C128_INV2C(R)                                                                                           \
    NDWT_R23(R, double, 2, 2, 1, 2) R(double, 2, 4, 2, 1, 2) R(double, 2, 4, 3, 1, 1) NDWT_R23(R, double, 2, 6, 1, 1) R(double, 2, 8, 2, 1, 1)

// The cascaded 1-D kernels of a batched plan (Fwd1C / Inv1C, ndwt_device_1d.h), rows of whole groups of 4 scalars: THE table of the
// instances that exist -- cascade1_levels (ndwt_select.h) answers from it, the launch units (ndwt_cascade1_{f32,c64,f64,c128}.hip)
// expand it.  {float, double} x EW {1, 2} x 2 .. 8 taps x 2 .. 4 levels x both directions: 96 instances, a list per data kind serving
// both directions (KIND = Fwd1C / Inv1C).  A lane holds a handful of 4-vectors: every instance fits 4 waves per SIMD without scratch.
#define NDWT_C234(C, KIND, T, EW, L) C(KIND, T, EW, L, 2) C(KIND, T, EW, L, 3) C(KIND, T, EW, L, 4)
#define NDWT_C1_KIND(C, KIND, T, EW) NDWT_C234(C, KIND, T, EW, 2) NDWT_C234(C, KIND, T, EW, 4) NDWT_C234(C, KIND, T, EW, 6) NDWT_C234(C, KIND, T, EW, 8)
#define NDWT_LIST_F32_1C(C, KIND) NDWT_C1_KIND(C, KIND, float, 1)
#define NDWT_LIST_C64_1C(C, KIND) NDWT_C1_KIND(C, KIND, float, 2)
#define NDWT_LIST_F64_1C(C, KIND) NDWT_C1_KIND(C, KIND, double, 1)
#define NDWT_LIST_C128_1C(C, KIND) NDWT_C1_KIND(C, KIND, double, 2)
#define NDWT_LIST_1C(C, KIND) NDWT_LIST_F32_1C(C, KIND) NDWT_LIST_C64_1C(C, KIND) NDWT_LIST_F64_1C(C, KIND) NDWT_LIST_C128_1C(C, KIND)

// The one-launch denoise of a batched 1-D plan (Den1C, ndwt_device_1d.h), rows of whole groups of 4 scalars: THE table of the instances
// that exist -- denoise1_levels (ndwt_select.h) answers from it, the launch units (ndwt_denoise1_{f32,c64,f64,c128}.hip) expand it.
// {float, double} x EW {1, 2} x 2 .. 8 taps x 1 .. 4 levels, less the three that spill: 61 instances.  A lane holds 2 + NLEV 4-vectors:
// every listed instance builds for gfx950 without LDS, scratch or spilled registers at 4 waves per SIMD (tools/kernel_resources.sh;
// DESIGN.md 4.3d has the counts).  Left out, all complex128: 6 taps x 4 levels (20 spilled registers, 84 B of scratch), 8 taps x 3
// levels (15, 64 B) and 8 taps x 4 levels (51, 208 B) -- ndwt_denoise_bands takes the general route there.
#define NDWT_D1234(D, T, EW, L) D(T, EW, L, 1) D(T, EW, L, 2) D(T, EW, L, 3) D(T, EW, L, 4)
#define NDWT_D1_KIND(D, T, EW) NDWT_D1234(D, T, EW, 2) NDWT_D1234(D, T, EW, 4) NDWT_D1234(D, T, EW, 6) NDWT_D1234(D, T, EW, 8)
#define NDWT_LIST_F32_DEN1(D) NDWT_D1_KIND(D, float, 1)
#define NDWT_LIST_C64_DEN1(D) NDWT_D1_KIND(D, float, 2)
#define NDWT_LIST_F64_DEN1(D) NDWT_D1_KIND(D, double, 1)
#define NDWT_LIST_C128_DEN1(D)                                                                                            \
    NDWT_D1234(D, double, 2, 2) NDWT_D1234(D, double, 2, 4) D(double, 2, 6, 1) D(double, 2, 6, 2) D(double, 2, 6, 3)      \
    D(double, 2, 8, 1) D(double, 2, 8, 2)
#define NDWT_LIST_DEN1(D) NDWT_LIST_F32_DEN1(D) NDWT_LIST_C64_DEN1(D) NDWT_LIST_F64_DEN1(D) NDWT_LIST_C128_DEN1(D)
// ... and with a threshold row per signal (Den1C<.., ROWTHR = true>; ndwt_denoise_bands_items, launch units ndwt_denoise1r_*.hip): a table
// of its own, the same (T, EW, L, NLEV) less the same three complex128 instances -- the row's thresholds live in scalar registers, and
// every listed instance builds with the VGPRs of its uniform twin and no scratch.  An instance that spilled where its
// twin does not would leave THIS table only.
#define NDWT_LIST_F32_DEN1R(D) NDWT_D1_KIND(D, float, 1)
#define NDWT_LIST_C64_DEN1R(D) NDWT_D1_KIND(D, float, 2)
#define NDWT_LIST_F64_DEN1R(D) NDWT_D1_KIND(D, double, 1)
#define NDWT_LIST_C128_DEN1R(D)                                                                                           \
    NDWT_D1234(D, double, 2, 2) NDWT_D1234(D, double, 2, 4) D(double, 2, 6, 1) D(double, 2, 6, 2) D(double, 2, 6, 3)      \
    D(double, 2, 8, 1) D(double, 2, 8, 2)
#define NDWT_LIST_DEN1R(D) NDWT_LIST_F32_DEN1R(D) NDWT_LIST_C64_DEN1R(D) NDWT_LIST_F64_DEN1R(D) NDWT_LIST_C128_DEN1R(D)

// The cascaded march of one strided axis (FwdMC / InvMC, ndwt_device_axis.h): THE table of the instances that exist -- cascadem_levels
// (ndwt_select.h) answers from it, the launch units (ndwt_marchc_{f32,f64}.hip) expand it.  {float, double} x 2 .. 8 taps x 2 .. 4 levels
// x both directions, less the two that spill.  A lane keeps NLEV windows of L 4-vectors: 4 NLEV L registers in float, twice that in
// double.  Every listed instance builds for gfx950 without scratch and without spilled vector registers (tools/kernel_resources.sh);
// InvMC<double, 8, 3> (5 spilled registers, 24 B of scratch) and InvMC<double, 8, 4> (162, 644 B) do not and are left out: the double
// 8-tap synthesis cascades two levels at a time.
#define NDWT_M234(M, KIND, T, L) M(KIND, T, L, 2) M(KIND, T, L, 3) M(KIND, T, L, 4)
#define NDWT_LIST_F32_FWDMC(M) NDWT_M234(M, FwdMC, float, 2) NDWT_M234(M, FwdMC, float, 4) NDWT_M234(M, FwdMC, float, 6) NDWT_M234(M, FwdMC, float, 8)
#define NDWT_LIST_F32_INVMC(M) NDWT_M234(M, InvMC, float, 2) NDWT_M234(M, InvMC, float, 4) NDWT_M234(M, InvMC, float, 6) NDWT_M234(M, InvMC, float, 8)
#define NDWT_LIST_F64_FWDMC(M) NDWT_M234(M, FwdMC, double, 2) NDWT_M234(M, FwdMC, double, 4) NDWT_M234(M, FwdMC, double, 6) NDWT_M234(M, FwdMC, double, 8)
#define NDWT_LIST_F64_INVMC(M) NDWT_M234(M, InvMC, double, 2) NDWT_M234(M, InvMC, double, 4) NDWT_M234(M, InvMC, double, 6) M(InvMC, double, 8, 2)
#define NDWT_LIST_MC(M) NDWT_LIST_F32_FWDMC(M) NDWT_LIST_F32_INVMC(M) NDWT_LIST_F64_FWDMC(M) NDWT_LIST_F64_INVMC(M)

// The per-axis passes (AxisMarch, AxisX: ndwt_device.h): THE table of the instances that exist -- axis_select (ndwt_select.h) answers from
// it, the launch unit (ndwt_march.hip) expands it.  AxisMarch: {float, double} x 2 .. 20 taps x both directions, 40 instances (interleaved
// complex: the factor 2 in the inner block).  AxisX: {float, double} x 2 .. 12 taps x both directions x EW {1, 2} x rows in whole groups of
// 4 scalars or not, 96 instances.  Where neither has an instance a pass runs the element-wise kernels, which take any tap length.
#define NDWT_N2(N, T, L) N(T, L, false) N(T, L, true)
#define NDWT_AXIS_MARCH_T(N, T)                                                                                            \
    NDWT_N2(N, T, 2) NDWT_N2(N, T, 4) NDWT_N2(N, T, 6) NDWT_N2(N, T, 8) NDWT_N2(N, T, 10) NDWT_N2(N, T, 12) NDWT_N2(N, T, 14)   \
    NDWT_N2(N, T, 16) NDWT_N2(N, T, 18) NDWT_N2(N, T, 20)
#define NDWT_LIST_F32_AXIS_MARCH(N) NDWT_AXIS_MARCH_T(N, float)
#define NDWT_LIST_F64_AXIS_MARCH(N) NDWT_AXIS_MARCH_T(N, double)
#define NDWT_X4(X, T, L, SYN) X(T, L, SYN, 1, true) X(T, L, SYN, 1, false) X(T, L, SYN, 2, true) X(T, L, SYN, 2, false)
#define NDWT_X8(X, T, L) NDWT_X4(X, T, L, false) NDWT_X4(X, T, L, true)
#define NDWT_AXISX_T(X, T) NDWT_X8(X, T, 2) NDWT_X8(X, T, 4) NDWT_X8(X, T, 6) NDWT_X8(X, T, 8) NDWT_X8(X, T, 10) NDWT_X8(X, T, 12)
#define NDWT_LIST_F32_AXISX(X) NDWT_AXISX_T(X, float)
#define NDWT_LIST_F64_AXISX(X) NDWT_AXISX_T(X, double)

// ---- questions to the lists
#define NDWT_IS_F(T, L, V, VEC4, EW, PIN, TPRE, WLDS) if (k == fwd3_instance(sizeof(T) == 8, L, V, VEC4, EW, PIN, TPRE, WLDS)) return true;
#define NDWT_IS_S(KIND, T, L, V, VEC4, EW) if (k == inv3s_instance(k##KIND, sizeof(T) == 8, L, V, VEC4, EW)) return true;
#define NDWT_IS_Y(L, VEC4, EW, DEPTH, UNIYZ, XSC) if (k == inv3y_instance(L, VEC4, EW, DEPTH, UNIYZ, XSC)) return true;
#define NDWT_IS_P(T, L, PD, PK) if (k == Fused2PInstance{sizeof(T) == 8, L, PD, PK}) return true;
inline bool inv3y_instantiated(const Fused3Instance& k) {
    NDWT_LIST_F32_INVY(NDWT_IS_Y) NDWT_LIST_F32_INVYS(NDWT_IS_Y) NDWT_LIST_F32_INVYC(NDWT_IS_Y)
    return false;
}
inline bool fused3_instantiated(const Fused3Instance& k) {
    if (k.kernel == kInv3Y) return inv3y_instantiated(k);
    NDWT_LIST_F32_FWD(NDWT_IS_F) NDWT_LIST_F32_FWDP(NDWT_IS_F) NDWT_LIST_F32_DEN(NDWT_IS_F) NDWT_LIST_F32_LONG(NDWT_IS_F)
    NDWT_LIST_F32_LONGB(NDWT_IS_F) NDWT_LIST_F32_INV(NDWT_IS_S) NDWT_LIST_F32_INVE(NDWT_IS_S) NDWT_LIST_F32_LONGI(NDWT_IS_S)
    NDWT_LIST_F64_FWD(NDWT_IS_F) NDWT_LIST_F64_INV(NDWT_IS_S) NDWT_LIST_F64_LONG(NDWT_IS_F, NDWT_IS_S)
    return false;
}
#define NDWT_IS_A(T, EW, L, NLEV, WPE) if (k == Cascade2Instance{false, sizeof(T) == 8, EW, L, NLEV, 0}) return true;
#define NDWT_IS_R(T, EW, L, NLEV, PD, WPE) if (k == Cascade2Instance{true, sizeof(T) == 8, EW, L, NLEV, PD}) return true;
inline bool cascade2_instantiated(const Cascade2Instance& k) {
    NDWT_LIST_F32_FWD2C(NDWT_IS_A) NDWT_LIST_C64_FWD2C(NDWT_IS_A) NDWT_LIST_F64_FWD2C(NDWT_IS_A) NDWT_LIST_C128_FWD2C(NDWT_IS_A)
    NDWT_LIST_F32_INV2C(NDWT_IS_R) NDWT_LIST_C64_INV2C(NDWT_IS_R) NDWT_LIST_F64_INV2C(NDWT_IS_R) NDWT_LIST_C128_INV2C(NDWT_IS_R)
    return false;
}
// scalars of a row one wave of the instance stores: the lanes inside the halo of every level, in whole 128-byte lines (Fwd2C::WX, Inv2C::WX;
// the launch units check the geometry against the kernel's own)
constexpr int cascade2_tile_width(const Cascade2Instance& k) { return wave_row_width(k.inverse, k.Lp, k.ew, k.f64, k.nlev); }
enum Cascade1Kind { kFwd1C, kInv1C };
#define NDWT_IS_C(KIND, T, EW, L, NLEV) if (k == Cascade1Instance{k##KIND == kInv1C, sizeof(T) == 8, EW, L, NLEV}) return true;
inline bool cascade1_instantiated(const Cascade1Instance& k) {
    NDWT_LIST_1C(NDWT_IS_C, Fwd1C) NDWT_LIST_1C(NDWT_IS_C, Inv1C)
    return false;
}
// scalars of a row one wave of the instance stores (Fwd1C::WX, Inv1C::WX: the same rule as the 2-D cascade's)
constexpr int cascade1_tile_width(const Cascade1Instance& k) { return wave_row_width(k.inverse, k.Lp, k.ew, k.f64, k.nlev); }
#define NDWT_IS_D(T, EW, L, NLEV) if (k == Den1Instance{sizeof(T) == 8, EW, L, NLEV}) return true;
inline bool den1r_instantiated(const Den1Instance& k) {
    NDWT_LIST_DEN1R(NDWT_IS_D)
    return false;
}
inline bool den1_instantiated(const Den1Instance& k) {
    NDWT_LIST_DEN1(NDWT_IS_D)
    return false;
}
// scalars of a row one wave of the instance stores (Den1C::WX)
constexpr int den1_tile_width(const Den1Instance& k) { return den1_tile_width(k.Lp, k.ew, k.f64, k.nlev); }
enum CascadeMKind { kFwdMC, kInvMC };
#define NDWT_IS_M(KIND, T, L, NLEV) if (k == CascadeMInstance{k##KIND == kInvMC, sizeof(T) == 8, L, NLEV}) return true;
inline bool cascadem_instantiated(const CascadeMInstance& k) {
    NDWT_LIST_MC(NDWT_IS_M)
    return false;
}
#define NDWT_IS_N(T, L, SYN) if (k == AxisMarchInstance{sizeof(T) == 8, SYN, L}) return true;
inline bool axis_march_instantiated(const AxisMarchInstance& k) {
    NDWT_LIST_F32_AXIS_MARCH(NDWT_IS_N) NDWT_LIST_F64_AXIS_MARCH(NDWT_IS_N)
    return false;
}
#define NDWT_IS_X(T, L, SYN, EW, VEC4) if (k == AxisXInstance{sizeof(T) == 8, SYN, VEC4, L, EW}) return true;
inline bool axisx_instantiated(const AxisXInstance& k) {
    NDWT_LIST_F32_AXISX(NDWT_IS_X) NDWT_LIST_F64_AXISX(NDWT_IS_X)
    return false;
}
// scalars of a row one wave of the instance stores (AxisX::WX)
constexpr int axisx_tile_width(const AxisXInstance& k) { return wave_row_width(k.syn, k.L, k.ew, k.f64, 1); }
#define NDWT_IS_W(KIND, T, L, VEC4, WPE, EW) if (k == Fused2SInstance{k##KIND == kInv2S, sizeof(T) == 8, VEC4, L, EW, WPE}) return true;
inline bool fused2s_instantiated(const Fused2SInstance& k) {
    NDWT_LIST_2S(NDWT_IS_W, Fwd2S) NDWT_LIST_2S(NDWT_IS_W, Inv2S)
    return false;
}
// a level of tap length Lp with the x taps stepping over ew scalars can run both ways: analysis and synthesis, rows in whole groups of 4
// scalars or not, at the register budget of fused2s_wpe
inline bool fused2s_both_ways(bool f64, int Lp, int ew) {
    for (int i = 0; i < 4; ++i)
        if (!fused2s_instantiated({i / 2 != 0, f64, i % 2 != 0, Lp, ew, fused2s_wpe(f64, Lp, ew)})) return false;
    return true;
}
inline bool inv2p_instantiated(const Fused2PInstance& k) {
    NDWT_LIST_F32_INV2P(NDWT_IS_P) NDWT_LIST_F64_INV2P(NDWT_IS_P)
    return false;
}

}  // namespace ndwt
