// ndwt_device_neigh.h -- the kernel of ndwt_shrink_neigh / ndwt_denoise_neigh: neighbourhood shrinkage, where the energy of a small
// periodic window around a coefficient, inside its own item of its own band, decides that coefficient (include/ndwt.h has the
// definition; NeighShrink, NeighBlock / NeighCoeff and the locally adaptive Wiener rule are this one primitive with other thresholds).
//
//   NeighShrink<T, COMP, ND, R>  a workgroup owns a tile of TX (x TY for ND = 3) positions of the leading filtered axes of one item of
//                one band and, for ND >= 2, marches along the last filtered axis over a chunk of it.  Per step it stores one haloed
//                line (ND <= 2) or plane tile (ND = 3) of the raw coefficients in LDS, (TX + 2R) (x (TY + 2R)) elements, every index
//                wrapped within the item; the loads of the next step are issued before this one's are used.
//                  A  the window sum along axis 0: dx ascending, re before im, a = fma((double)e, (double)e, a) from 0 -- straight from
//                     the raw tile (LDS holds the coefficients in T, not their squares: a float widens exactly, and a double's square
//                     added by an fma cannot be had from a rounded square).  ND = 3: for all TY + 2R rows, into a second LDS tile.
//                  B  ND = 3: the 2R + 1 rows of A, the first term first, plain double additions.
//                The last axis (ND >= 2) goes through a register ring of the 2R + 1 latest partial sums (A for ND = 2, B for ND = 3) of
//                every position the thread owns, summed anew from its 2R + 1 terms, the first term first, at every step: no running
//                sum, so a value does not depend on where the march began.  The centre coefficients wait R steps in registers.  A chunk
//                primes its ring from the R planes before its first output, wrapped, and runs R planes past its last.
//                ND = 1: one step, no ring; the items lie in the grid.
//
// Per position, S the window sum, tt = the band's (double)t * (double)t from the host (so that S - t * t is never contracted):
// S > tt in double: soft g = (T)((S - tt) / S), every part times g in T; hard: copied; else every part is stored as +0.  tt < 0 marks a
// band with t == 0: its tiles copy their positions and nothing else.
//
// The tile (neigh_tx / neigh_ty, ndwt_select.h) and what it costs, (TX + 2R)(TY + 2R) / (TX TY), are in DESIGN.md 4.3j.  A wave's loads
// and stores run along axis 0: a row of the tile is 64 or 256 consecutive elements.  No atomics, no hand-off between workgroups; the
// input is only read, the output only written, each position by the one thread that owns it.
//
// Written like the kernels of ndwt_device_joint.h: per-thread phases driven through an executor, so the same source runs under the host
// emulator.  What a thread keeps across a barrier lies in its State.
#pragma once
#include <initializer_list>
#include "ndwt_device_joint.h"

namespace ndwt {

template <typename T> struct NeighArgs {
    const T* y;                        // band 0 of the coefficient array
    T* out;                            // band 0 of the result: the layout of y
    long long band_pitch;              // scalars from one band to the next, in both
    long long n;                       // scalars of ONE item of a band; item j of band b starts at b * band_pitch + j * n
    const double* tt;                  // device, [bands of the table]: the squared thresholds; below 0: copy the band
    long long items;
    int n0, n1, n2;                    // elements along the filtered axes of one item, axis 0 the fastest (1 where there is none)
    int band0, nbands;                 // the bands of this launch
    int ntx, nty, chunk, nchunks;      // neigh_geometry: tiles along axis 0 and axis 1, planes of a chunk of the march, chunks
    int hard;
};

// An element as the kernel moves it: a scalar, or the two parts of a complex one as a vector at element alignment (a vector is a
// register value wherever it goes; a struct of two doubles is not: the compiler parks it in LDS or scratch).
template <typename T, int COMP> struct NeighElem {
    typedef T type;
    template <int K> static NDWT_DEV T part(const type& c) { return c; }
};
template <typename T> struct NeighElem<T, 2> {
    typedef typename VecT<T>::v2u type;
    template <int K> static NDWT_DEV T part(const type& c) { return c[K]; }
};

// Workgroup `bid` is (band, item, chunk, tile y, tile x), x fastest.  The host has checked: every filtered axis >= 2R + 1, a line
// (ND <= 2) or a plane (ND = 3) of one item below 2^31 scalars.
template <typename T, int COMP_, int ND_, int R_> struct NeighShrink {
    static constexpr int COMP = COMP_, ND = ND_, R = R_, NT = 256, WPE = 4;
    static constexpr int TX = neigh_tx(ND), TY = neigh_ty(ND, (int)sizeof(T) * COMP, R);
    static constexpr int D = ND == 1 ? 0 : R;                       // steps between a plane's load and its output
    static constexpr int RAWX = TX + 2 * R, RAWY = ND == 3 ? TY + 2 * R : 1, NRAW = RAWX * RAWY, NLOAD = (NRAW + NT - 1) / NT;
    static constexpr int ROWS = NT / TX, PER = TY / ROWS;           // rows of the tile in one pass of the threads; positions a thread owns
    static constexpr int PERA = ND == 3 ? (RAWY + ROWS - 1) / ROWS : 0;   // rows of A a thread computes
    static constexpr int NBUF = ND == 3 ? 1 : 2;                    // (ND <= 2: one barrier a step, so two lines)
    static_assert(NT % TX == 0 && TY % ROWS == 0 && PER >= 1, "the threads cover the tile in whole passes of whole rows");
    typedef NeighElem<T, COMP> E;
    typedef typename E::type item_t;
    static_assert(alignof(item_t) == alignof(T), "an element lies wherever a scalar may");
    typedef NeighArgs<T> Args;
    typedef SelectTaps Taps;
    struct Shared {
        item_t raw[NBUF][NRAW];        // the haloed tile of one step, [row][x]
        double A[ND == 3 ? RAWY * TX : 1];   // ND = 3: the window sums along axis 0 of every row, [row][x]
    };
    struct State {
        item_t pre[NLOAD];             // the thread's loads of the next step
        int off[NLOAD];                // where they come from: elements from the start of the line / plane
        double ring[2 * D + 1][PER];   // the partial sums of the 2D + 1 latest steps, oldest first
        item_t cen[D + 1][PER];        // the coefficients of the D + 1 latest steps, oldest first
    };
    static NDWT_DEV void load(State& st, const T* p) {
        NDWT_SFOR(k, NLOAD)
            st.pre[k] = reinterpret_cast<const item_t*>(p)[st.off[k]];
        NDWT_SEND
    }
    static NDWT_DEV double rowsum(const item_t* w) {
        double s = 0.0;
        NDWT_SFOR(dx, 2 * R + 1)
            const item_t c = w[dx];
            NDWT_SFOR(k, COMP)
                const double e = (double)E::template part<k>(c);
                s = __builtin_fma(e, e, s);                           // (as JointStep::add accumulates)
            NDWT_SEND
        NDWT_SEND
        return s;
    }
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        int q = bid;
        const int x0 = q % a.ntx * TX;
        q /= a.ntx;
        const int y0 = q % a.nty * TY;
        q /= a.nty;
        const int z0 = q % a.nchunks * a.chunk;
        q /= a.nchunks;
        const long long item = q % a.items;
        const int band = a.band0 + (int)(q / a.items);
        const int nm = ND == 1 ? 1 : ND == 2 ? a.n1 : a.n2;         // the marched axis
        const int z1 = z0 + a.chunk < nm ? z0 + a.chunk : nm;
        const long long plane = ND == 1 ? 0 : (ND == 2 ? (long long)a.n0 : (long long)a.n0 * a.n1) * COMP;   // scalars from a step to the next
        const long long base = band * a.band_pitch + item * a.n;
        const T* const src = a.y + base;
        T* const dst = a.out + base;
        const double tt = a.tt[band];
        // position k of thread tid: inside the item?  and its element in the line / plane
        const auto own = [&](int tid, int k, int* at) __attribute__((always_inline)) {
            const int gx = x0 + tid % TX, gy = y0 + tid / TX + k * ROWS;
            const bool in = gx < a.n0 && (ND != 3 || gy < a.n1);
            *at = !in ? 0 : ND == 3 ? gy * a.n0 + gx : gx;
            return in;
        };
        if (tt < 0.0) {
            ex.each([&](int tid, State&) __attribute__((always_inline)) {
                for (int z = z0; z < z1; ++z)
                    NDWT_SFOR(k, PER)
                        int at;
                        if (own(tid, k, &at)) reinterpret_cast<item_t*>(dst + z * plane)[at] = reinterpret_cast<const item_t*>(src + z * plane)[at];
                    NDWT_SEND
            });
            return;
        }
        const int nsteps = z1 - z0 + 2 * D;
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            NDWT_SFOR(k, NLOAD)
                const int idx = tid + k * NT;
                st.off[k] = 0;                                    // (beyond the tile: a load nobody uses)
                if (idx < NRAW) {
                    st.off[k] = modn(x0 - R + idx % RAWX, a.n0);
                    if constexpr (ND == 3) st.off[k] += modn(y0 - R + idx / RAWX, a.n1) * a.n0;
                }
            NDWT_SEND
            load(st, src + modn(z0 - D, nm) * plane);
        });
        _Pragma("clang loop unroll(disable)")
        for (int s = 0; s < nsteps; ++s) {
            const int buf = NBUF == 2 ? s & 1 : 0;
            ex.each([&](int tid, State& st) __attribute__((always_inline)) {
                NDWT_SFOR(k, NLOAD)
                    if (tid + k * NT < NRAW) sh.raw[buf][tid + k * NT] = st.pre[k];
                NDWT_SEND
                if (s + 1 < nsteps) load(st, src + modn(z0 - D + s + 1, nm) * plane);
            });
            ex.barrier();
            if constexpr (ND == 3) {
                ex.each([&](int tid, State& st) __attribute__((always_inline)) {
                    const int x = tid % TX, row = tid / TX;
                    NDWT_SFOR(k, PERA)
                        if (row + k * ROWS < RAWY) sh.A[(row + k * ROWS) * TX + x] = rowsum(&sh.raw[0][(row + k * ROWS) * RAWX + x]);
                    NDWT_SEND
                    NDWT_SFOR(k, PER)
                        st.cen[D][k] = sh.raw[0][(row + k * ROWS + R) * RAWX + x + R];
                    NDWT_SEND
                });
                ex.barrier();
            }
            ex.each([&](int tid, State& st) __attribute__((always_inline)) {
                const int x = tid % TX, row = tid / TX;
                NDWT_SFOR(k, PER)
                    NDWT_SFOR(j, 2 * D)
                        st.ring[j][k] = st.ring[j + 1][k];
                    NDWT_SEND
                    if constexpr (ND == 3) {
                        double b = sh.A[(row + k * ROWS) * TX + x];
                        NDWT_SFOR(dy, 2 * R)
                            b += sh.A[(row + k * ROWS + dy + 1) * TX + x];
                        NDWT_SEND
                        st.ring[2 * D][k] = b;
                    } else {
                        st.ring[2 * D][k] = rowsum(&sh.raw[buf][x]);
                        st.cen[D][k] = sh.raw[buf][x + R];
                    }
                NDWT_SEND
                if (s >= 2 * D) {
                    const long long zo = (long long)(z0 + s - 2 * D) * plane;
                    NDWT_SFOR(k, PER)
                        double sum = st.ring[0][k];
                        NDWT_SFOR(j, 2 * D)
                            sum += st.ring[j + 1][k];
                        NDWT_SEND
                        item_t c = st.cen[0][k];
                        if (sum > tt) {
                            if (!a.hard) c = c * (T)((sum - tt) / sum);
                        } else {
                            c = item_t{};                             // an explicit +0 in every part
                        }
                        int at;
                        if (own(tid, k, &at)) reinterpret_cast<item_t*>(dst + zo)[at] = c;
                    NDWT_SEND
                }
                NDWT_SFOR(k, PER)
                    NDWT_SFOR(j, D)
                        st.cen[j][k] = st.cen[j + 1][k];
                    NDWT_SEND
                NDWT_SEND
            });
        }
    }
};

// What a launch checks before any workgroup runs (the emulator too): the geometry is that of the instance's own tile over the whole
// item and covers the march exactly, no axis is shorter than the window, a line / plane stays below 2^31 scalars, the bands do not
// overlap and the grid can be numbered.  *blocks: the workgroups.
template <typename T> inline bool neigh_launch_ok(const NeighArgs<T>& a, int comp, int nd, int r, long long* blocks) {
    if ((comp != 1 && comp != 2) || nd < 1 || nd > 3 || r < 1 || r > 3) return false;
    const int tx = neigh_tx(nd), ty = neigh_ty(nd, (int)sizeof(T) * comp, r), w = 2 * r + 1;
    const long long nm = nd == 1 ? 1 : nd == 2 ? a.n1 : a.n2;
    if (a.n0 < w || a.n1 < (nd >= 2 ? w : 1) || a.n2 < (nd == 3 ? w : 1) || (nd < 2 && a.n1 != 1) || (nd < 3 && a.n2 != 1)) return false;
    if ((long long)a.n0 * (nd == 3 ? a.n1 : 1) * comp > 0x7fffffffLL || (long long)a.n0 * a.n1 * a.n2 * comp != a.n) return false;
    if (a.ntx != (a.n0 + tx - 1) / tx || a.nty != (nd == 3 ? (a.n1 + ty - 1) / ty : 1)) return false;
    if (a.chunk < 1 || a.nchunks < 1 || (long long)a.nchunks * a.chunk < nm || (long long)(a.nchunks - 1) * a.chunk >= nm) return false;
    if (a.nbands < 1 || a.band0 < 0 || a.items < 1 || a.band_pitch / a.items < a.n || !a.y || !a.out || !a.tt) return false;
    long long b = a.nbands;
    for (const long long f : {a.items, (long long)a.nchunks, (long long)a.nty, (long long)a.ntx}) {
        if (b > 0x7fffffffLL / f) return false;
        b *= f;
    }
    *blocks = b;
    return true;
}

#ifndef NDWT_HOST_EMU
// The launches (ndwt_neigh_f32.hip / ndwt_neigh_f64.hip): NeighShrink<T, comp, nd, r> on nbands * items * nchunks * nty * ntx workgroups.
// buf_dev: a device buffer of the plan (what the kernel gets for a tap table: it reads none).  -1: no such instance, -2: a geometry that
// is not the instance's tile, an axis shorter than the window, a plane past 2^31 scalars or a grid the launch cannot express.
int launch_neigh_shrink(const NeighArgs<float>& a, int comp, int nd, int r, const void* buf_dev, hipStream_t s);
int launch_neigh_shrink(const NeighArgs<double>& a, int comp, int nd, int r, const void* buf_dev, hipStream_t s);
#endif

}  // namespace ndwt
