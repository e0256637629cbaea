// ndwt_device_axis.h -- all levels of ONE strided axis inside one march (FwdMC / InvMC): AxisMarch (ndwt_device.h) with NLEV windows.
//
// For plans over interleaved samples (ndwt_plan_create_interleaved, ndim == 1, inner > 1) at the reference's dilation: the array is
// [outer][n][inner] scalars, the filtered axis has stride `inner`, every level applies the same taps at tap stride 1.  A thread owns 4
// consecutive scalars of the inner block (v4 loads and stores) and marches a chunk [zbeg, zend) of the axis, once, for NLEV levels:
//   analysis   level l + 1 takes the low output of level l the step it is produced; the details of every level and the approximation
//              of the last one are written for the positions of the chunk: 1 read -> NLEV + 1 writes, instead of NLEV x (1 -> 2)
//   synthesis  scatter form; the coarsest level's completed sum is the next level's approximation, taken with that level's detail plane
//              from memory: NLEV + 1 reads -> 1 write, instead of NLEV x (2 -> 1)
// A chunk reads NLEV (L - 1) planes of march-in on top of its own; every plane index goes through the periodic wrap of the item
// (modn64), whatever the ratio of march-in to axis length.
//
// All windows turn together: whichever level, the plane of step p sits in slot p % L, so one rot_dispatch<L> serves the NLEV windows
// (a rotation per level would be L^NLEV cases).  A level whose window is not full yet computes values nobody keeps: level l + 1 is
// full L - 1 steps after level l, and by then every slot it reads was written from a full level-l window.
// Per level, the FMAs are those of AxisMarch::step in the same order.
#pragma once
#include "ndwt_device.h"

namespace ndwt {

constexpr int kMarchCMaxLevels = 4;
template <typename T> struct MarchCArgs {
    const T* in[1 + kMarchCMaxLevels];   // analysis: in[0]; synthesis: in[0] = approximation of the coarsest level, in[1 + c] = detail of
                                         // cascade stage c (0 = coarsest)
    T* out[1 + kMarchCMaxLevels];        // analysis: out[0] = approximation of the last level, out[1 + l] = detail of cascade level l
                                         // (0 = finest); synthesis: out[0]
    long long inner;                     // scalars between two planes of the axis, a multiple of 4
    long long n;                         // length of the axis
    long long outer;                     // items: item o at o * n * inner
    int chunk, nchunks;                  // output planes per thread, chunks along the axis
    long long ngroups;                   // inner / 4
};

// what both directions share: bid -> (block of 256 (item, group) pairs, chunk), as AxisMarch lays them out
template <typename T, int L_, int NLEV_, bool SYN> struct MarchCBase {
    static constexpr int L = L_, NLEV = NLEV_, NT = 256, WPE = 4;
    static constexpr int LH = SYN ? L / 2 : L / 2 - 1, RH = SYN ? L / 2 - 1 : L / 2;
    static_assert(NLEV >= 2 && NLEV <= kMarchCMaxLevels && L >= 2 && L % 2 == 0, "FwdMC / InvMC: 2 .. 4 levels, even tap lengths");
    typedef typename VecT<T>::v4 v4;
    typedef MarchTaps<T, L> Taps;
    typedef MarchCArgs<T> Args;
    struct Shared { int unused; };
    struct State {
        v4 win[NLEV][L];               // analysis: the planes each level's filter sees; synthesis: partial sums of each level's pending outputs
        v4 nxt[SYN ? NLEV + 1 : 1];    // the planes of the next step, in flight
        long long base;
        int active;
    };
    template <class Exec, class Load> static NDWT_DEV void setup(Exec& ex, const Args& a, int bid, long long& zbeg, long long& zend, Load&& load) {
        const long long items = a.ngroups * a.outer;
        const long long iblocks = (items + NT - 1) / NT;
        const long long ib = bid % iblocks;
        zbeg = (long long)(bid / iblocks) * a.chunk;
        zend = zbeg + a.chunk < a.n ? zbeg + a.chunk : a.n;
        const long long q0 = zbeg - (long long)NLEV * LH;
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            const long long it = ib * NT + tid;
            st.active = it < items;
            const long long iv = st.active ? it : 0;     // (an idle thread marches item 0 and stores nothing)
            st.base = (iv / a.ngroups) * a.n * a.inner + (iv % a.ngroups) * 4;
            NDWT_SFOR(l, NLEV)
                NDWT_SFOR(j, L)
                    st.win[l][j] = (v4)(T(0));
                NDWT_SEND
            NDWT_SEND
            load(st, q0);
        });
    }
};

template <typename T, int L_, int NLEV_> struct FwdMC : MarchCBase<T, L_, NLEV_, false> {
    typedef MarchCBase<T, L_, NLEV_, false> B;
    using B::L; using B::NLEV; using B::NT; using B::LH; using B::RH;
    typedef typename B::v4 v4;
    typedef typename B::Taps Taps;
    typedef typename B::Args Args;
    typedef typename B::Shared Shared;
    typedef typename B::State State;
    static NDWT_DEV void load(State& st, const Args& a, long long q) {
        st.nxt[0] = *reinterpret_cast<const v4*>(a.in[0] + st.base + modn64(q, a.n) * a.inner);
    }
    // input plane q enters level 1; level l + 1 (l = 0 ..) then holds its output for position q - (l + 1) RH
    template <int R> static NDWT_DEV void step(State& st, const Args& a, const Taps& tp, long long zbeg, long long zend, long long q) {
        v4 cur = st.nxt[0];
        NDWT_SFOR(l, NLEV)
            st.win[l][(R + L - 1) % L] = cur;
            v4 lo = (v4)(T(0)), hi = (v4)(T(0));
            NDWT_SFOR(j, L)
                lo += tp.lo[j] * st.win[l][(R + j) % L];
                hi += tp.hi[j] * st.win[l][(R + j) % L];
            NDWT_SEND
            const long long z = q - (long long)(l + 1) * RH;   // inside the chunk only once this level's window is full
            if (st.active && z >= zbeg && z < zend) {
                const long long off = st.base + z * a.inner;
                *reinterpret_cast<v4*>(a.out[1 + l] + off) = hi;
                if constexpr (l == NLEV - 1) *reinterpret_cast<v4*>(a.out[0] + off) = lo;
            }
            cur = lo;
        NDWT_SEND
    }
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared&, const Args& a, const Taps& tp, int bid) {
        long long zbeg, zend;
        B::setup(ex, a, bid, zbeg, zend, [&](State& st, long long q) __attribute__((always_inline)) { load(st, a, q); });
        const long long q0 = zbeg - (long long)NLEV * LH;
        const int nplanes = (int)(zend - zbeg) + NLEV * (L - 1);
        for (int p = 0; p < nplanes; ++p) {
            ex.each([&](int, State& st) __attribute__((always_inline)) {
                rot_dispatch<L>((p + 1) % L, [&](auto R) __attribute__((always_inline)) { step<decltype(R)::value>(st, a, tp, zbeg, zend, q0 + p); });
                load(st, a, q0 + (p + 1 < nplanes ? p + 1 : p));
            });
        }
    }
};

template <typename T, int L_, int NLEV_> struct InvMC : MarchCBase<T, L_, NLEV_, true> {
    typedef MarchCBase<T, L_, NLEV_, true> B;
    using B::L; using B::NLEV; using B::NT; using B::LH; using B::RH;
    typedef typename B::v4 v4;
    typedef typename B::Taps Taps;
    typedef typename B::Args Args;
    typedef typename B::Shared Shared;
    typedef typename B::State State;
    // stage c takes its planes c RH positions behind stage 0: the approximation and the coarsest detail at q, the detail of stage c at q - c RH
    static NDWT_DEV void load(State& st, const Args& a, long long q) {
        st.nxt[0] = *reinterpret_cast<const v4*>(a.in[0] + st.base + modn64(q, a.n) * a.inner);
        NDWT_SFOR(c, NLEV)
            st.nxt[1 + c] = *reinterpret_cast<const v4*>(a.in[1 + c] + st.base + modn64(q - (long long)c * RH, a.n) * a.inner);
        NDWT_SEND
    }
    template <int R> static NDWT_DEV void step(State& st, const Args& a, const Taps& tp, long long zbeg, long long zend, long long q) {
        v4 ap = st.nxt[0];
        NDWT_SFOR(c, NLEV)
            const v4 d = st.nxt[1 + c];
            NDWT_SFOR(j, L)
                constexpr int slot = ((R - 1 - j) % L + L) % L;
                const v4 t = tp.lo[j] * ap + tp.hi[j] * d;
                if constexpr (j == 0) st.win[c][slot] = t;
                else st.win[c][slot] += t;
            NDWT_SEND
            ap = st.win[c][((R - L) % L + L) % L];            // the output this plane completes: the next stage's approximation
        NDWT_SEND
        const long long z = q - (long long)NLEV * RH;
        if (st.active && z >= zbeg && z < zend) *reinterpret_cast<v4*>(a.out[0] + st.base + z * a.inner) = ap;
    }
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared&, const Args& a, const Taps& tp, int bid) {
        long long zbeg, zend;
        B::setup(ex, a, bid, zbeg, zend, [&](State& st, long long q) __attribute__((always_inline)) { load(st, a, q); });
        const long long q0 = zbeg - (long long)NLEV * LH;
        const int nplanes = (int)(zend - zbeg) + NLEV * (L - 1);
        for (int p = 0; p < nplanes; ++p) {
            ex.each([&](int, State& st) __attribute__((always_inline)) {
                rot_dispatch<L>((p + 1) % L, [&](auto R) __attribute__((always_inline)) { step<decltype(R)::value>(st, a, tp, zbeg, zend, q0 + p); });
                load(st, a, q0 + (p + 1 < nplanes ? p + 1 : p));
            });
        }
    }
};

}  // namespace ndwt
