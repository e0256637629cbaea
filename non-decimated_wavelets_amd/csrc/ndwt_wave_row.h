// ndwt_wave_row.h -- the filter stages of the wave-per-row kernels, once each (included by ndwt_device.h below the primitives it uses:
// VecT, static_for, PkF32, Taps3 / Taps3Y, NDWT_LANE_SHIFT, modn, stream_store).
//
// Fwd2S, Fwd2C, Inv2S, Inv2P, Inv2C and AxisX (ndwt_device.h) and Fwd1C, Inv1C (ndwt_device_1d.h) follow one scheme: a wave owns a segment
// of a row, a lane holds 4 consecutive scalars, neighbours arrive by DPP lane shifts, and the y direction, where there is one, is a
// rotating register window (analysis) or rotating partial sums (synthesis).  What those kernels have in common is written here; what
// differs between them -- which lanes store, which band goes where, when a level computes -- stays in the kernels.  That the cascades
// compute bit for bit what the per-level kernels compute follows from their running these same functions.
//
// How a stage names a neighbour's value: NDWT_LANE_SHIFT evaluates an expression on the lane's own State on the GPU and on the peer's
// State under the emulator, so a stage cannot take a reference to "the row".  It takes a stateless accessor instead, one per input row,
//     NDWT_ROW(s.raw[S][b])   =   [](const State& s) -> const v4& { return s.raw[S][b]; }
// and writes NDWT_LANE_SHIFT(ex, tid, D, row(s)[c]).  (Both macros read the names `State` and `st` of the function they stand in.)
//
// Everything is NDWT_DEV (force-inlined): the kernels compile to the code they had with the stages written out in each of them
// (tools/isa_diff.sh compares two builds kernel by kernel; profiles/isa_identity_wave_rows.txt).
#pragma once
#include "ndwt_fused_tile.h"

#define NDWT_ROW(expr_of_s) [](const State& s) __attribute__((always_inline)) -> decltype(auto) { return (expr_of_s); }

namespace ndwt {

// A sum written as explicit fused multiply-adds: `acc += tap * v` compiles to FMA chains in the short bodies, but in the longer ones of
// the 1-D cascade the SLP vectorizer splits some chains into a packed multiply and separate adds (two roundings instead of one).
NDWT_DEV float fma1(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
NDWT_DEV double fma1(double a, double b, double c) { return __builtin_fma(a, b, c); }

// The geometry of a wave: the filter reaches LH scalars to the left and RH to the right of an output (EW scalars per element: the taps of
// interleaved complex data step over the (re, im) pairs), which is GL / GR lanes of 4 scalars; XV scalars of the wave-local window reach
// one lane's outputs.  WX: scalars of a row a wave stores (wave_row_width, the rule the host lays its launches out by).
template <typename T, int L_, int EW_, bool SYN, int NLEV_ = 1> struct WaveRowGeom {
    static constexpr int L = L_, EW = EW_, NLEV = NLEV_;
    static constexpr int LH = SYN ? L / 2 : L / 2 - 1, RH = SYN ? L / 2 - 1 : L / 2;
    static constexpr int GL = (LH * EW + 3) / 4, GR = (RH * EW + 3) / 4;
    static constexpr int XV = 4 * (1 + GL + GR);
    static constexpr int LPL = 32 / (int)sizeof(T);      // lanes to a 128-byte line (a lane stores 4 scalars)
    static constexpr int WX = wave_row_width(SYN, L, EW, sizeof(T) == 8, NLEV);
};

// run-time rotation -> compile-time R: f(std::integral_constant<int, R>) for R == r, one of L specialisations of the step body
template <int L, int R = 0, class F> NDWT_DEV void rot_dispatch(int r, F&& f) {
    if constexpr (R < L) {
        if (r == R) f(std::integral_constant<int, R>{});
        else rot_dispatch<L, R + 1>(r, f);
    }
}

// ---- analysis ----
// y stage: the row `cur` enters the window (rotation R: the newest row sits in slot (R + L - 1) % L); (lo, hi) pairs of the lane's 4 x
template <int R, typename T, int L, class V4, class V2> NDWT_DEV void ystage_pairs(V4 (&win)[L], const V4& cur, const Taps3<T, L>& tp, V2 (&yz)[4]) {
    win[(R + L - 1) % L] = cur;
    V2 acc[4];
    acc[0] = acc[1] = acc[2] = acc[3] = (V2)(T(0));
    NDWT_SFOR(j, L)
        V4 w = win[(R + j) % L];
        V2 t = {tp.lo[1][j], tp.hi[1][j]};
        acc[0] += t * w[0]; acc[1] += t * w[1]; acc[2] += t * w[2]; acc[3] += t * w[3];
    NDWT_SEND
    yz[0] = acc[0]; yz[1] = acc[1]; yz[2] = acc[2]; yz[3] = acc[3];
}
// x stage: the pairs of the neighbouring lanes by lane shifts (every lane executes them) -> (lo2, hi2) pairs of the x low-pass / high-pass
// sums of the lane's 4 x.  The kernels turn them into the four band vectors themselves (band_vectors, or written out): Fwd2S, which
// stores from a subset of its lanes, behind that test; Fwd2C in front of it -- with the vectors built in a function the float Fwd2C
// instances come out scheduled differently (tools/isa_diff.sh)
template <class G, class Exec, class State, typename T, class Row, class V2>
NDWT_DEV void xstage_pairs(Exec& ex, State& st, int tid, const Taps3<T, G::L>& tp, Row yz, V2 (&xlo)[4], V2 (&xhi)[4]) {
    typedef V2 v2;
    NDWT_SFOR(e, 4)
        xlo[e] = (v2)(T(0));
        xhi[e] = (v2)(T(0));
    NDWT_SEND
    NDWT_SFOR(i, G::XV)
        constexpr int D = i / 4 - G::GL;
        constexpr int c = i % 4;
        {
            v2 v = {NDWT_LANE_SHIFT(ex, tid, D, yz(s)[c].x), NDWT_LANE_SHIFT(ex, tid, D, yz(s)[c].y)};
            NDWT_SFOR(e, 4)
                constexpr int dj = i - 4 * G::GL - e;                  // = (j - LH) * EW
                if constexpr (dj % G::EW == 0) {
                    constexpr int j = dj / G::EW + G::LH;
                    if constexpr (j >= 0 && j < G::L) {
                        xlo[e] += tp.lo[0][j] * v;
                        xhi[e] += tp.hi[0][j] * v;
                    }
                }
            NDWT_SEND
        }
    NDWT_SEND
}
template <class V2, class V4> NDWT_DEV void band_vectors(const V2 (&xlo)[4], const V2 (&xhi)[4], V4& o0, V4& o1, V4& o2, V4& o3) {
    o0 = V4{xlo[0].x, xlo[1].x, xlo[2].x, xlo[3].x}; o1 = V4{xhi[0].x, xhi[1].x, xhi[2].x, xhi[3].x};
    o2 = V4{xlo[0].y, xlo[1].y, xlo[2].y, xlo[3].y}; o3 = V4{xhi[0].y, xhi[1].y, xhi[2].y, xhi[3].y};
}

// ---- synthesis, scalar form ----
// x stage: the rows a0 / d0 (x-bit 0 / 1 of y-bit 0) and a1 / d1 (y-bit 1) -> p0 / p1, the (a, d) inputs of the y synthesis; scalars,
// not pairs: see Inv3S::xsyn (pairs would be built right behind the prefetch loads)
template <class G, class Exec, class State, class Taps, class RA0, class RD0, class RA1, class RD1, typename T>
NDWT_DEV void xsyn_rows(Exec& ex, State& st, int tid, const Taps& tp, RA0 a0, RD0 d0, RA1 a1, RD1 d1, T (&p0)[4], T (&p1)[4]) {
    NDWT_SFOR(e, 4)
        p0[e] = T(0);
        p1[e] = T(0);
    NDWT_SEND
    NDWT_SFOR(i, G::XV)
        constexpr int D = i / 4 - G::GL;
        constexpr int c = i % 4;
        {
            const T wa0 = NDWT_LANE_SHIFT(ex, tid, D, a0(s)[c]);   // x-bit 0, y-bit 0
            const T wd0 = NDWT_LANE_SHIFT(ex, tid, D, d0(s)[c]);   // x-bit 1, y-bit 0
            const T wa1 = NDWT_LANE_SHIFT(ex, tid, D, a1(s)[c]);   // x-bit 0, y-bit 1
            const T wd1 = NDWT_LANE_SHIFT(ex, tid, D, d1(s)[c]);   // x-bit 1, y-bit 1
            NDWT_SFOR(e, 4)
                constexpr int dj = i - 4 * G::GL - e;
                if constexpr (dj % G::EW == 0) {
                    constexpr int j = dj / G::EW + G::LH;
                    if constexpr (j >= 0 && j < G::L) {
                        p0[e] += tp.lo[0][j] * wa0;
                        p0[e] += tp.hi[0][j] * wd0;
                        p1[e] += tp.lo[0][j] * wa1;
                        p1[e] += tp.hi[0][j] * wd1;
                    }
                }
            NDWT_SEND
        }
    NDWT_SEND
}
// y stage in scatter form: the newest row adds to the partial sums of the L output rows it reaches (rotation R) and completes the row
// in slot ysyn_done_slot.  Inv2S / Inv2P store that row from a subset of their lanes and build the vector at the store, behind the test
// (with the vector built here, hipcc schedules their float instances differently: tools/isa_diff.sh); the cascade, where every lane
// hands the row to the next level, takes it from ysyn_scatter_row / ysyn_scatter_pk.
constexpr int ysyn_done_slot(int R, int L) { return ((R - L) % L + L) % L; }
template <int R, int L, typename T, class Taps> NDWT_DEV void ysyn_scatter(T (&yacc)[L][4], const Taps& tp, const T (&p0)[4], const T (&p1)[4]) {
    NDWT_SFOR(j, L)
        constexpr int slot = ((R - 1 - j) % L + L) % L;
        NDWT_SFOR(e, 4)
            const T c = tp.lo[1][j] * p0[e] + tp.hi[1][j] * p1[e];
            if constexpr (j == 0) yacc[slot][e] = c;
            else yacc[slot][e] += c;
        NDWT_SEND
    NDWT_SEND
}
// the same, returning the row it completes (the cascade, where the row is the next level's input)
template <int R, int L, typename T, class Taps> NDWT_DEV typename VecT<T>::v4 ysyn_scatter_row(T (&yacc)[L][4], const Taps& tp, const T (&p0)[4], const T (&p1)[4]) {
    ysyn_scatter<R>(yacc, tp, p0, p1);
    constexpr int done = ysyn_done_slot(R, L);
    return typename VecT<T>::v4{yacc[done][0], yacc[done][1], yacc[done][2], yacc[done][3]};
}

// ---- synthesis, packed form (float, real data): pairs of adjacent x outputs per v_pk_fma_f32, tap pairs pinned in SGPRs ----
// the pinned pairs a kernel's RegT holds: xl / xh[k] = (t[k], t[k-1]) of the x low-pass / high-pass taps (Taps3Y::xplo / xphi), k = 0 .. L
template <int L, class RegT, class Taps> NDWT_DEV void pin_x_pairs(RegT& rt, const Taps& tp) {
    typedef PkF32::v2 v2;
    NDWT_SFOR(k, L + 1)
        rt.xl[k] = PkF32::pinned(v2{tp.xplo[k][0], tp.xplo[k][1]});
        rt.xh[k] = PkF32::pinned(v2{tp.xphi[k][0], tp.xphi[k][1]});
    NDWT_SEND
}
// yl / yh[m] = (t[2m], t[2m+1]) of the y taps
template <int L, class RegT, class Taps> NDWT_DEV void pin_y_pairs(RegT& rt, const Taps& tp) {
    typedef PkF32::v2 v2;
    NDWT_SFOR(m, L / 2)
        rt.yl[m] = PkF32::pinned(v2{tp.lo[1][2 * m], tp.lo[1][2 * m + 1]});
        rt.yh[m] = PkF32::pinned(v2{tp.hi[1][2 * m], tp.hi[1][2 * m + 1]});
    NDWT_SEND
}
// x stage: (out[e], out[e+1]) += w * (t[k], t[k-1]) with the neighbour's sample w broadcast from one half of its register pair.
// P[y band][x outputs (0, 1) / (2, 3)]
template <class G, class Exec, class State, class RegT, class RA0, class RD0, class RA1, class RD1>
NDWT_DEV void xsyn_rows_pk(Exec& ex, State& st, int tid, const RegT& rt, RA0 a0, RD0 d0, RA1 a1, RD1 d1, PkF32::v2 (&P)[2][2]) {
    typedef PkF32::v2 v2;
    P[0][0] = P[0][1] = P[1][0] = P[1][1] = (v2)(0.0f);
    NDWT_SFOR(ii, G::XV / 2)
        constexpr int i0 = 2 * ii;
        constexpr int D = i0 / 4 - G::GL;
        constexpr int c = i0 % 4;                         // 0 or 2: the register pair (c, c + 1) of the lane D away
        v2 w[4];
        w[0] = v2{NDWT_LANE_SHIFT(ex, tid, D, a0(s)[c]), NDWT_LANE_SHIFT(ex, tid, D, a0(s)[c + 1])};
        w[1] = v2{NDWT_LANE_SHIFT(ex, tid, D, d0(s)[c]), NDWT_LANE_SHIFT(ex, tid, D, d0(s)[c + 1])};
        w[2] = v2{NDWT_LANE_SHIFT(ex, tid, D, a1(s)[c]), NDWT_LANE_SHIFT(ex, tid, D, a1(s)[c + 1])};
        w[3] = v2{NDWT_LANE_SHIFT(ex, tid, D, d1(s)[c]), NDWT_LANE_SHIFT(ex, tid, D, d1(s)[c + 1])};
        NDWT_SFOR(h, 2)
            constexpr int k0 = i0 + h - 4 * G::GL + G::LH;   // tap pair of the outputs (0, 1); (2, 3): two taps earlier
            NDWT_SFOR(q, 2)
                constexpr int k = k0 - 2 * q;
                if constexpr (k >= 0 && k <= G::L) {
                    PkF32::fma_bt<h, false, false, false>(P[0][q], w[0], rt.xl[k]);
                    PkF32::fma_bt<h, false, false, false>(P[0][q], w[1], rt.xh[k]);
                    PkF32::fma_bt<h, false, false, false>(P[1][q], w[2], rt.xl[k]);
                    PkF32::fma_bt<h, false, false, false>(P[1][q], w[3], rt.xh[k]);
                }
            NDWT_SEND
        NDWT_SEND
    NDWT_SEND
}
// y stage in scatter form, a tap broadcast from one half of an SGPR pair; returns the row it completes (Inv2P does not use it: see above)
template <int R, int L, class RegT> NDWT_DEV VecT<float>::v4 ysyn_scatter_pk(float (&yacc)[L][4], const RegT& rt, const PkF32::v2 (&P)[2][2]) {
    typedef PkF32::v2 v2;
    NDWT_SFOR(j, L)
        constexpr int slot = ((R - 1 - j) % L + L) % L;
        NDWT_SFOR(q, 2)
            v2 acc;
            if constexpr (j == 0) acc = (v2)(0.0f);
            else acc = v2{yacc[slot][2 * q], yacc[slot][2 * q + 1]};
            PkF32::fma_s<j % 2, false>(acc, P[0][q], rt.yl[j / 2]);
            PkF32::fma_s<j % 2, false>(acc, P[1][q], rt.yh[j / 2]);
            yacc[slot][2 * q] = acc.x;
            yacc[slot][2 * q + 1] = acc.y;
        NDWT_SEND
    NDWT_SEND
    constexpr int done = ysyn_done_slot(R, L);
    return VecT<float>::v4{yacc[done][0], yacc[done][1], yacc[done][2], yacc[done][3]};
}

// ---- a lane's row access where rows need not be whole groups of 4 scalars (Fwd2S, Inv2S) ----
// offsets of the lane's scalars xb .. from the row start, wrapped: one if rows are whole groups of 4 (VEC4), else each of the 4
template <int NE> NDWT_DEV void lane_offsets(int (&off)[NE], int xb, int n1) {
    NDWT_SFOR(e, NE)
        off[e] = modn(xb + e, n1);
    NDWT_SEND
}
// the lane's 4 scalars of NB rows, row b at row(b) (a function: where the kernel wrote the address out at each access, it still is): one
// aligned access each (VEC4), one access at element alignment if the 4 are contiguous (VecT::v4u), scalar by scalar for the lane that
// straddles the wrap
template <bool VEC4, int NB, int NE, class V4, class RowPtr> NDWT_DEV void load_lane_rows(V4* dst, RowPtr row, const int (&off)[NE]) {
    typedef std::remove_cv_t<std::remove_reference_t<decltype(row(0)[0])>> T;
    if constexpr (VEC4) {
        NDWT_SFOR(b, NB)
            dst[b] = *reinterpret_cast<const V4*>(row(b) + off[0]);
        NDWT_SEND
    } else if (off[NE - 1] == off[0] + 3) {
        NDWT_SFOR(b, NB)
            dst[b] = *reinterpret_cast<const typename VecT<T>::v4u*>(row(b) + off[0]);
        NDWT_SEND
    } else {
        NDWT_SFOR(b, NB)
            NDWT_SFOR(e, NE)
                dst[b][e] = row(b)[off[e]];
            NDWT_SEND
        NDWT_SEND
    }
}
// store of the lane's 4 scalars of NB rows at p[b] + off, the scalars gx .. of a row of n1: streaming (VEC4), one access at element
// alignment, or a predicated scalar tail
template <bool VEC4, int NB, typename T, class V4>
NDWT_DEV void store_lane_rows(T* const (&p)[NB], long long off, const V4 (&o)[NB], int gx, int n1, int nt) {
    if constexpr (VEC4) {
        NDWT_SFOR(b, NB)
            stream_store(reinterpret_cast<V4*>(p[b] + off), o[b], nt);
        NDWT_SEND
    } else if (gx + 3 < n1) {
        NDWT_SFOR(b, NB)
            *reinterpret_cast<typename VecT<T>::v4u*>(p[b] + off) = o[b];
        NDWT_SEND
    } else {
        NDWT_SFOR(e, 4)
            if (gx + e < n1) {
                NDWT_SFOR(b, NB)
                    p[b][off + e] = o[b][e];
                NDWT_SEND
            }
        NDWT_SEND
    }
}

// ---- the 1-D row filter over lane shifts (AxisX, Fwd1C, Inv1C): output e of the lane sums the taps over the wave-local window ----
// FMA1: the sums as explicit FMAs (the cascade: see fma1) or as `acc += tap * v` (AxisX, whose instances all compile that to the same
// FMA chains; with the explicit form the SLP vectorizer packs AxisX<float, 8, analysis> differently, so it keeps the form it had)
// analysis: one input row, the low-pass and the high-pass sum
template <class G, bool FMA1, class Exec, class State, typename T, class Row, class V4>
NDWT_DEV void row_filter_ana(Exec& ex, State& st, int tid, const T (&lo)[G::L], const T (&hi)[G::L], Row in, V4& o0, V4& o1) {
    o0 = (V4)(T(0));
    o1 = (V4)(T(0));
    NDWT_SFOR(e, 4)
        NDWT_SFOR(j, G::L)
            constexpr int idx = e + (j - G::LH) * G::EW + 4 * G::GL;      // scalar index in the wave-local window, >= 0
            constexpr int D = idx / 4 - G::GL;
            constexpr int c = idx % 4;
            const T v = NDWT_LANE_SHIFT(ex, tid, D, in(s)[c]);
            if constexpr (FMA1) {
                o0[e] = fma1(lo[j], v, o0[e]);
                o1[e] = fma1(hi[j], v, o1[e]);
            } else {
                o0[e] += lo[j] * v;
                o1[e] += hi[j] * v;
            }
        NDWT_SEND
    NDWT_SEND
}
// synthesis: the approximation and the detail row, one sum
template <class G, bool FMA1, class Exec, class State, typename T, class RowA, class RowD, class V4>
NDWT_DEV void row_filter_syn(Exec& ex, State& st, int tid, const T (&lo)[G::L], const T (&hi)[G::L], RowA in0, RowD in1, V4& o0) {
    o0 = (V4)(T(0));
    NDWT_SFOR(e, 4)
        NDWT_SFOR(j, G::L)
            constexpr int idx = e + (j - G::LH) * G::EW + 4 * G::GL;
            constexpr int D = idx / 4 - G::GL;
            constexpr int c = idx % 4;
            if constexpr (FMA1) {
                o0[e] = fma1(lo[j], NDWT_LANE_SHIFT(ex, tid, D, in0(s)[c]), o0[e]);
                o0[e] = fma1(hi[j], NDWT_LANE_SHIFT(ex, tid, D, in1(s)[c]), o0[e]);
            } else {
                o0[e] += lo[j] * NDWT_LANE_SHIFT(ex, tid, D, in0(s)[c]);
                o0[e] += hi[j] * NDWT_LANE_SHIFT(ex, tid, D, in1(s)[c]);
            }
        NDWT_SEND
    NDWT_SEND
}

}  // namespace ndwt
