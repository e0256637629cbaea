// ndwt_device_1d.h -- several levels of many 1-D signals in one launch (Fwd1C / Inv1C): AxisX (ndwt_device.h) grown by a level loop.
//
// At the reference's dilation every level applies the same filter pair to the approximation of the level before, so the 4 scalars of
// level l's approximation a lane holds ARE the input of level l + 1: they stay in the lane, and only the detail band of every level
// (analysis) or of every level's input (synthesis) goes through memory -- (NLEV + 2) signal volumes instead of 3 NLEV.  Rows are
// [outer][row] scalars, row = n * EW (EW = 2: interleaved complex, the taps step over the pairs) in whole groups of 4, periodic.
//
// One wave per (row, segment) item, as AxisX: lane l holds the 4 scalars at xg = seg0 + 4 (l - NLEV GL) of the row (wrapped), its
// neighbours come from the adjacent lanes by DPP wave shifts.  Every level costs GL lanes on the left and GR on the right, so level k
// (1 = first computed) is valid in lanes [k GL, 64 - k GR); a wave stores the lanes valid at every level, rounded down to whole
// 128-byte lines (the rule of Fwd2C), and every band from that same window.  A level is the row filter AxisX::compute runs
// (row_filter_ana / row_filter_syn, ndwt_wave_row.h), so the result equals NLEV launches of AxisX<T, L, SYN, EW, true> bit for bit.
//
// Written like the fused kernels: per-lane stages driven through an executor, so the same source runs under the host emulator.
#pragma once
#include "ndwt_device.h"
#include "ndwt_shrink.h"

namespace ndwt {

template <typename T> struct Fused1CArgs {
    const T* in[5];        // analysis: in[0] the signals; synthesis: [0] the approximation of the coarsest level, [1 + c] the detail band of
                           // cascade level c (0 = coarsest: the one synthesised first)
    T* out[5];             // analysis: [0] the approximation of the last level, [1 + l] the detail band of cascade level l (0 = first /
                           // finest); synthesis: out[0]
    long long row;         // scalars per row = n * EW, a multiple of 4
    long long outer;       // rows (signals)
    long long nseg;        // wave segments per row: ceil(row / WX)
};

// what both directions share: the geometry of a wave and the (row, segment) item of a lane
template <typename T, int L_, int NLEV_, int EW_, bool SYN> struct Cascade1Geom {
    typedef WaveRowGeom<T, L_, EW_, SYN, NLEV_> W;
    static constexpr int NLEV = NLEV_, NT = 256;
    static constexpr int LH = W::LH, RH = W::RH, GL = W::GL, GR = W::GR, WX = W::WX;   // WX: output scalars per wave segment
    static_assert(NLEV >= 2 && NLEV <= 4, "two to four levels per launch");
    static_assert(WX > 0, "no lane is valid at every level");
    // fills the lane's place in its row; returns the offset of its 4 scalars (wrapped) from the band pointers
    template <class State> static NDWT_DEV long long place(State& st, const Fused1CArgs<T>& a, int bid, int tid) {
        const long long item = (long long)bid * (NT / 64) + tid / 64;           // one wave per (row, segment)
        const long long nitems = a.outer * a.nseg;
        st.valid = item < nitems;
        const long long it = st.valid ? item : nitems - 1;
        const long long o = it / a.nseg, sg = it % a.nseg;
        st.base = o * a.row;
        st.xg = (int)(sg * WX) + 4 * (tid % 64 - NLEV * GL);
        return st.base + modn64(st.xg, a.row);            // (rows are whole groups of 4: a group never straddles the wrap)
    }
    // this lane stores: inside the window valid at every level, and inside the row (the last segment may reach past its end)
    template <class State> static NDWT_DEV bool stores(const State& st, const Fused1CArgs<T>& a, int tid) {
        const int lane = tid % 64;
        return st.valid && lane >= NLEV * GL && lane < NLEV * GL + WX / 4 && st.xg < a.row;
    }
};

template <typename T, int L_, int NLEV_, int EW_ = 1, int WPE_ = 4> struct Fwd1C {
    typedef Cascade1Geom<T, L_, NLEV_, EW_, false> G;
    static constexpr int L = L_, NLEV = NLEV_, EW = EW_, NT = G::NT, WPE = WPE_;
    static constexpr int LH = G::LH, RH = G::RH, GL = G::GL, GR = G::GR, WX = G::WX;
    typedef typename VecT<T>::v4 v4;
    typedef Taps3<T, L> Taps;                            // axis 0 is used
    typedef Fused1CArgs<T> Args;
    struct Shared { int unused; };
    struct State {
        v4 cur;            // this lane's 4 scalars of the level's input: the raw row, then the approximations
        v4 nxt;            // the approximation being computed (the neighbours still read cur)
        long long base;
        int xg;            // first scalar of this lane inside the row (outside [0, row) for halo lanes)
        int valid;
    };
    // one level: AxisX's row filter on st.cur; the detail band to memory, the approximation to st.nxt
    template <int LEV, class Exec> static NDWT_DEV void level(Exec& ex, State& st, const Args& a, const Taps& tp, int tid) {
        v4 o0, o1;
        row_filter_ana<typename G::W, true>(ex, st, tid, tp.lo[0], tp.hi[0], NDWT_ROW(s.cur), o0, o1);
        st.nxt = o0;
        if (!G::stores(st, a, tid)) return;
        const long long off = st.base + st.xg;
        *reinterpret_cast<v4*>(a.out[1 + LEV] + off) = o1;
        if constexpr (LEV == NLEV - 1) *reinterpret_cast<v4*>(a.out[0] + off) = o0;
    }
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared&, const Args& a, const Taps& tp, int bid) {
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            const long long off = G::place(st, a, bid, tid);
            st.cur = *reinterpret_cast<const v4*>(a.in[0] + off);
        });
        NDWT_SFOR(lev, NLEV)
            ex.each([&](int tid, State& st) __attribute__((always_inline)) { level<lev>(ex, st, a, tp, tid); });
            if constexpr (lev + 1 < NLEV) ex.each([&](int, State& st) __attribute__((always_inline)) { st.cur = st.nxt; });
        NDWT_SEND
    }
};

template <typename T, int L_, int NLEV_, int EW_ = 1, int WPE_ = 4> struct Inv1C {
    typedef Cascade1Geom<T, L_, NLEV_, EW_, true> G;
    static constexpr int L = L_, NLEV = NLEV_, EW = EW_, NT = G::NT, WPE = WPE_;
    static constexpr int LH = G::LH, RH = G::RH, GL = G::GL, GR = G::GR, WX = G::WX;
    typedef typename VecT<T>::v4 v4;
    typedef Taps3<T, L> Taps;                            // axis 0 is used
    typedef Fused1CArgs<T> Args;
    struct Shared { int unused; };
    struct State {
        v4 cur;            // the approximation entering the level: the coarsest one, then every level's output
        v4 nxt;
        v4 det[NLEV_];     // the detail band of every level, all loaded up front
        long long base;
        int xg;
        int valid;
    };
    // one level: AxisX's row filter (synthesis) on st.cur and st.det[LEV]; its output is the approximation of the next finer level
    template <int LEV, class Exec> static NDWT_DEV void level(Exec& ex, State& st, const Args& a, const Taps& tp, int tid) {
        v4 o0;
        row_filter_syn<typename G::W, true>(ex, st, tid, tp.lo[0], tp.hi[0], NDWT_ROW(s.cur), NDWT_ROW(s.det[LEV]), o0);
        st.nxt = o0;
        if constexpr (LEV == NLEV - 1) {
            if (G::stores(st, a, tid)) *reinterpret_cast<v4*>(a.out[0] + st.base + st.xg) = o0;
        }
    }
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared&, const Args& a, const Taps& tp, int bid) {
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            const long long off = G::place(st, a, bid, tid);
            st.cur = *reinterpret_cast<const v4*>(a.in[0] + off);
            NDWT_SFOR(lev, NLEV)
                st.det[lev] = *reinterpret_cast<const v4*>(a.in[1 + lev] + off);
            NDWT_SEND
        });
        NDWT_SFOR(lev, NLEV)
            ex.each([&](int tid, State& st) __attribute__((always_inline)) { level<lev>(ex, st, a, tp, tid); });
            if constexpr (lev + 1 < NLEV) ex.each([&](int, State& st) __attribute__((always_inline)) { st.cur = st.nxt; });
        NDWT_SEND
    }
};

// ---- dec -> threshold per band -> rec of the signals of a batched plan in ONE launch (Den1C): the analysis cascade above, the
// thresholding of shrink_kernel (shrink_group, ndwt_shrink.h) on the coefficients where they lie -- in the lane -- and the synthesis
// cascade, without a coefficient ever reaching memory: one read of the signals (with halo) and one write.
//
// Geometry: a lane holds the 4 scalars at xg = seg0 + 4 (lane - HL), HL = NLEV (GLa + GLs) (a / s: the halo lanes of the analysis / of the
// synthesis, WaveRowGeom).  Analysis level k is valid in lanes [k GLa, 64 - k GRa); the synthesis, coarsest level first, then costs GLs
// and GRs lanes per level, so the result is valid in [HL, 64 - HR), HR = NLEV (GRa + GRs), stored in whole 128-byte lines: WX =
// den1_tile_width.  What a lane outside its level's window computes (the wave shifts deliver 0 past the wave's ends) never reaches a
// storing lane.  A wave reads halo scalars that lie in another wave's output segment: the input and the output must not overlap.
template <typename T> struct Den1CArgs : Fused1CArgs<T> {   // in[0]: the signals; out[0]: the result
    T thr[5];              // [0] the approximation of the last level, [1 + l] the detail band of cascade level l (0 = finest); 0: the band is left alone
    int hard;
    const T* thr_rows = nullptr;   // Den1C<.., ROWTHR = true>: a device table [outer][5], row j the thr[] of signal j (ndwt_denoise_bands_items)
};
template <typename T, int L> struct Taps1D {              // both directions of a 1-D plan, as the host appends them (axis 0 is used)
    Taps3<T, L> ana, syn;
};

// ROWTHR: the thresholds of a wave are those of its signal, read from a.thr_rows (five loads per wave, the row number is the wave's);
// false: a.thr for every signal
template <typename T, int L_, int NLEV_, int EW_ = 1, int WPE_ = 4, bool ROWTHR_ = false> struct Den1C {
    typedef WaveRowGeom<T, L_, EW_, false> WA;
    typedef WaveRowGeom<T, L_, EW_, true> WS;
    static constexpr int L = L_, NLEV = NLEV_, EW = EW_, NT = 256, WPE = WPE_;
    static constexpr bool ROWTHR = ROWTHR_;
    static constexpr int HL = NLEV * (WA::GL + WS::GL), HR = NLEV * (WA::GR + WS::GR);
    static constexpr int WX = 4 * ((64 - HL - HR) / WA::LPL * WA::LPL);   // output scalars per wave segment
    static_assert(NLEV >= 1 && NLEV <= 4, "one to four levels per launch");
    static_assert(WX > 0, "no lane is valid at every level");
    typedef typename VecT<T>::v4 v4;
    typedef Taps1D<T, L> Taps;
    typedef Den1CArgs<T> Args;
    struct Shared { int unused; };
    struct State {
        v4 cur;            // the raw row, then the approximations on the way down, then every synthesis level's output on the way up
        v4 nxt;
        v4 det[NLEV_];     // the detail band of every level (0 = finest)
        long long base;
        int xg;            // first scalar of this lane inside the row (outside [0, row) for halo lanes)
        int valid;
    };
    // fills the lane's place in its row; returns the offset of its 4 scalars (wrapped) from the signals
    static NDWT_DEV long long place(State& st, const Args& a, int bid, int tid) {
        const long long item = (long long)bid * (NT / 64) + tid / 64;           // one wave per (row, segment)
        const long long nitems = a.outer * a.nseg;
        st.valid = item < nitems;
        const long long it = st.valid ? item : nitems - 1;
        const long long o = it / a.nseg, sg = it % a.nseg;
        st.base = o * a.row;
        st.xg = (int)(sg * WX) + 4 * (tid % 64 - HL);
        return st.base + modn64(st.xg, a.row);            // (rows are whole groups of 4: a group never straddles the wrap)
    }
    // a value every lane of the wave holds alike: in scalar registers on the device, so that what is loaded through it is a scalar load
    static NDWT_DEV long long wave_uniform(long long v) {
#ifndef NDWT_HOST_EMU
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
        return (long long)(((unsigned long long)hi << 32) | lo);
#else
        return v;
#endif
    }
    // this lane stores: inside the window valid after the last synthesis level, and inside the row
    static NDWT_DEV bool stores(const State& st, const Args& a, int tid) {
        const int lane = tid % 64;
        return st.valid && lane >= HL && lane < HL + WX / 4 && st.xg < a.row;
    }
    // shrink_kernel's arithmetic on the lane's 4 scalars (EW = 2: two (re, im) pairs)
    static NDWT_DEV void shrink4(v4& c, T thr, int hard) {
        T e[4] = {c[0], c[1], c[2], c[3]};
        NDWT_SFOR(k, 4 / EW)
            shrink_group<T, EW>(e + k * EW, thr, hard);
        NDWT_SEND
        c = v4{e[0], e[1], e[2], e[3]};
    }
    template <int LEV, class Exec> static NDWT_DEV void ana_level(Exec& ex, State& st, const Taps& tp, int tid) {
        v4 o0, o1;
        row_filter_ana<WA, true>(ex, st, tid, tp.ana.lo[0], tp.ana.hi[0], NDWT_ROW(s.cur), o0, o1);
        st.nxt = o0;
        st.det[LEV] = o1;
    }
    // synthesis of cascade level LEV (NLEV - 1 = coarsest, first): its output is the approximation of the next finer level, or the result
    template <int LEV, class Exec> static NDWT_DEV void syn_level(Exec& ex, State& st, const Args& a, const Taps& tp, int tid) {
        v4 o0;
        row_filter_syn<WS, true>(ex, st, tid, tp.syn.lo[0], tp.syn.hi[0], NDWT_ROW(s.cur), NDWT_ROW(s.det[LEV]), o0);
        st.nxt = o0;
        if constexpr (LEV == 0) {
            if (stores(st, a, tid)) *reinterpret_cast<v4*>(a.out[0] + st.base + st.xg) = o0;
        }
    }
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared&, const Args& a, const Taps& tp, int bid) {
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            const long long off = place(st, a, bid, tid);
            st.cur = *reinterpret_cast<const v4*>(a.in[0] + off);
        });
        NDWT_SFOR(lev, NLEV)
            ex.each([&](int tid, State& st) __attribute__((always_inline)) { ana_level<lev>(ex, st, tp, tid); });
            ex.each([&](int, State& st) __attribute__((always_inline)) { st.cur = st.nxt; });
        NDWT_SEND
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            if constexpr (ROWTHR) {
                // the row of place(): the wave's (row, segment) item, the waves past the last item clamped onto it -- inside the table
                const long long item = (long long)bid * (NT / 64) + tid / 64, nitems = a.outer * a.nseg;
                const T* const thr = a.thr_rows + 5 * wave_uniform((item < nitems ? item : nitems - 1) / a.nseg);
                if (thr[0] > T(0)) shrink4(st.cur, thr[0], a.hard);
                NDWT_SFOR(lev, NLEV)
                    if (thr[1 + lev] > T(0)) shrink4(st.det[lev], thr[1 + lev], a.hard);
                NDWT_SEND
            } else {
                if (a.thr[0] > T(0)) shrink4(st.cur, a.thr[0], a.hard);
                NDWT_SFOR(lev, NLEV)
                    if (a.thr[1 + lev] > T(0)) shrink4(st.det[lev], a.thr[1 + lev], a.hard);
                NDWT_SEND
            }
        });
        NDWT_SFOR(c, NLEV)
            ex.each([&](int tid, State& st) __attribute__((always_inline)) { syn_level<NLEV - 1 - c>(ex, st, a, tp, tid); });
            if constexpr (c + 1 < NLEV) ex.each([&](int, State& st) __attribute__((always_inline)) { st.cur = st.nxt; });
        NDWT_SEND
    }
};

}  // namespace ndwt
