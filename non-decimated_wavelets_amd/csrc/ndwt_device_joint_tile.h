// ndwt_device_joint_tile.h -- the tile form of the joint shrinkage and the group norms (ndwt_device_joint.h has the semantics and the
// chunk form): for plans of MANY SHORT items, where a band has too few steps to give every thread of the chunk form a position.
//
//   JointTile       a workgroup takes a strip of SW consecutive steps of one band.  Sweep 1: all 256 threads load -- thread tid is
//                   (row tid / SW, column tid % SW), a pass moves step `column` of 256 / SW items, P = J * SW / 256 passes fill an LDS
//                   tile of J items x SW steps -- and the SW * NPOS threads that own a position of the strip add the tile's J items to
//                   their s in ascending j, re before im, with the fma of JointStep::add; s stays in a register over all tiles.  The
//                   loads of tile t + 1 are issued before tile t is summed.  Sweep 2: the gain of every position once, through LDS, then
//                   all 256 threads read their (item, step) again, scale and store -- two batches of P loads in flight, no order to keep.
//   GroupNormsTile  sweep 1 alone; the owners feed the accumulators of GroupNorms, then the combine of BandNorms.  With more than one
//                   strip per band the partials go to NormsFinish (one item), as the chunks of GroupNorms do.
//
// The order of s is that of JointShrink / GroupNorms, so every stored scalar, every group's s and m, nnz and max are the same bits; l1
// and l2sq add the positions in another fixed order (the owners of a strip through the tree, the strips through NormsFinish): no
// floating-point atomics, two calls on one device give the same bits.
//
// Rows beyond the last item and columns beyond the band's last step load and store nothing; a band with threshold 0 returns before
// any access.  LDS: the tile, J * SW steps (16 KB float, 32 KB double in the 4-scalar form), plus the gains or the combine's 8 KB.
//
// Written like the kernels of ndwt_device_joint.h: per-thread phases driven through an executor, so the same source runs under the host
// emulator.  What a thread keeps across a barrier lies in its State.
#pragma once
#include "ndwt_device_joint.h"

namespace ndwt {

// the shapes both kernels share, and sweep 1
template <typename T, int COMP, bool VEC> struct JointTileSum {
    typedef JointStep<T, COMP, VEC> S;
    typedef typename S::item_t item_t;
    static constexpr int NT = 256, SW = kJointTileSW, J = kJointTileJ, ROWS = NT / SW, P = J / ROWS, OWN = SW * S::NPOS;
    static_assert(NT % SW == 0 && J % ROWS == 0 && P >= 1 && OWN <= NT, "a pass is whole rows of the strip, a tile whole passes");
    struct Tile { alignas(32) T v[J * SW * S::W]; };   // [item][step][scalar]: pass p of thread tid lies at step-sized slot p * NT + tid
    struct State {
        item_t c[P];                   // the thread's loads of the next tile (sweep 2: of the next batch)
        double s;                      // an owner's sum of squares
    };
    // the loads of thread tid for the tile that starts at item j0: nothing beyond item K - 1 or step `steps` - 1
    static NDWT_DEV void load(int tid, State& st, const T* d, long long n, long long K, long long steps, int strip, long long j0) {
        const int row = tid / SW, col = tid % SW;
        const long long i = (long long)strip * SW + col;
        NDWT_SFOR(p, P)
            const long long j = j0 + p * ROWS + row;
            st.c[p] = item_t{};
            if (i < steps && j < K) st.c[p] = reinterpret_cast<const item_t*>(d + j * n)[i];
        NDWT_SEND
    }
    // Afterwards st.s of thread tid < OWN is the s of position tid of the strip (step tid / NPOS, position tid % NPOS of it); a
    // position beyond the band's last step has s = +0.  Ends behind a barrier: the tile is free.
    template <class Exec> static NDWT_DEV void sweep(Exec& ex, Tile& tile, const T* d, long long n, long long K, long long steps, int strip) {
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            st.s = 0.0;
            load(tid, st, d, n, K, steps, strip, 0);
        });
        for (long long j0 = 0; j0 < K; j0 += J) {
            ex.each([&](int tid, State& st) __attribute__((always_inline)) {
                item_t* const t = reinterpret_cast<item_t*>(tile.v);
                NDWT_SFOR(p, P)
                    t[p * NT + tid] = st.c[p];
                NDWT_SEND
                if (j0 + J < K) load(tid, st, d, n, K, steps, strip, j0 + J);
            });
            ex.barrier();
            ex.each([&](int tid, State& st) __attribute__((always_inline)) {
                if (tid >= OWN) return;
                const int jn = K - j0 < J ? (int)(K - j0) : J;
                const T* const q = tile.v + tid * COMP;           // item j of this position: q[j * SW * W + part]
                double s = st.s;
                const auto add = [&](int j) __attribute__((always_inline)) {
                    NDWT_SFOR(k, COMP)
                        const double e = (double)q[j * (SW * S::W) + k];
                        s = __builtin_fma(e, e, s);
                    NDWT_SEND
                };
                if (jn == J) {
                    _Pragma("unroll 16")                          // (16 LDS reads ahead of the chain of fmas)
                    for (int j = 0; j < J; ++j) add(j);
                } else {
                    for (int j = 0; j < jn; ++j) add(j);
                }
                st.s = s;
            });
            ex.barrier();
        }
    }
};

// Workgroup `bid` is (band, strip), strip fastest; a.chunks is the strips per band, joint_tile_strips (the launch checks it).  VEC: y,
// band_pitch and n are multiples of 4 scalars (the rule of ShrinkItems).
template <typename T, int COMP_, bool VEC_> struct JointTile {
    typedef JointTileSum<T, COMP_, VEC_> G;
    static constexpr int COMP = COMP_, NT = G::NT, WPE = 4, SW = G::SW, J = G::J;
    static constexpr bool VEC = VEC_;
    typedef typename G::S S;
    typedef typename S::item_t item_t;
    typedef JointShrinkArgs<T> Args;
    typedef SelectTaps Taps;
    typedef typename G::State State;
    struct Shared {
        typename G::Tile tile;
        T g[G::OWN];                   // the gain of every position of the strip (0 where the group goes to zero)
        int keep[G::OWN];
    };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        const int strip = bid % a.chunks, band = bid / a.chunks;
        const T thr = a.table[band];
        if (thr == T(0)) return;
        T* const d = a.y + band * a.band_pitch;
        const long long steps = VEC ? a.n / 4 : a.n / COMP, K = a.items;
        G::sweep(ex, sh.tile, d, a.n, K, steps, strip);
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            if (tid >= G::OWN) return;
            T g = T(0);
            const bool keep = S::gain(st.s, thr, a.hard, &g);
            sh.g[tid] = keep ? g : T(0);
            sh.keep[tid] = keep;
        });
        ex.barrier();
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            const int row = tid / SW, col = tid % SW;
            const long long i = (long long)strip * SW + col;
            if (i >= steps) return;
            T g[S::NPOS];
            bool keep[S::NPOS];
            NDWT_SFOR(k, S::NPOS)
                g[k] = sh.g[col * S::NPOS + k];
                keep[k] = sh.keep[col * S::NPOS + k] != 0;
            NDWT_SEND
            const auto at = [&](long long j) __attribute__((always_inline)) { return reinterpret_cast<item_t*>(d + j * a.n) + i; };
            const auto load = [&](long long j0) __attribute__((always_inline)) {
                NDWT_SFOR(p, G::P)
                    st.c[p] = j0 + p * G::ROWS < K ? *at(j0 + p * G::ROWS) : item_t{};
                NDWT_SEND
            };
            load(row);
            for (long long j0 = row; j0 < K; j0 += J) {
                item_t c[G::P];
                NDWT_SFOR(p, G::P)
                    c[p] = st.c[p];
                NDWT_SEND
                load(j0 + J);
                NDWT_SFOR(p, G::P)
                    if (j0 + p * G::ROWS < K) *at(j0 + p * G::ROWS) = S::scaled(c[p], keep, g);
                NDWT_SEND
            }
        });
    }
};

// Workgroup `bid` is (band, strip), strip fastest; a.chunks is the strips per band.  a.out: chunks == 1: the results [nb][4]; else the
// partials [band][strip][4] (NormsFinish's, one item).
template <typename T, int COMP_, bool VEC_> struct GroupNormsTile {
    typedef JointTileSum<T, COMP_, VEC_> G;
    static constexpr int COMP = COMP_, NT = G::NT, WPE = 4, SW = G::SW, J = G::J;
    static constexpr bool VEC = VEC_;
    typedef GroupNormsArgs<T> Args;
    typedef SelectTaps Taps;
    typedef typename G::State State;
    struct Shared {
        typename G::Tile tile;
        NormsShared<NT> n;
    };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        const int strip = bid % a.chunks, band = bid / a.chunks;
        const T* const d = a.y + band * a.band_pitch;
        G::sweep(ex, sh.tile, d, a.n, a.items, VEC ? a.n / 4 : a.n / COMP, strip);
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            NormsAcc acc = {0.0, 0.0, 0.0, 0ULL};                 // (a thread that owns no position adds nothing)
            if (tid < G::OWN) {
                const double m = (double)(T)sqrt((T)st.s);
                acc.l1 += m;
                acc.l2 += st.s;
                acc.mx = norms_max(acc.mx, m);
                acc.nz += st.s != 0.0;
            }
            sh.n.l1[tid] = acc.l1;
            sh.n.l2[tid] = acc.l2;
            sh.n.mx[tid] = acc.mx;
            sh.n.nz[tid] = acc.nz;
        });
        norms_tree<NT, State>(ex, sh.n);
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            if (tid != 0) return;
            norms_write<NT>(sh.n, a.chunks == 1 ? a.out + (long long)band * 4 : a.out + ((long long)band * a.chunks + strip) * 4);
        });
    }
};

#ifndef NDWT_HOST_EMU
// The launches (ndwt_joint_tile_f32.hip / ndwt_joint_tile_f64.hip): JointTile<T, comp, vec> and GroupNormsTile<T, comp, vec> on
// nb * chunks workgroups.  buf_dev: a device buffer of the plan (what the kernels get for a tap table: they read none).  -1: no such
// instance, -2: a grid the launch cannot express, or chunks that are not the strips of the band.
int launch_joint_tile(const JointShrinkArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
int launch_joint_tile(const JointShrinkArgs<double>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
int launch_group_norms_tile(const GroupNormsArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
int launch_group_norms_tile(const GroupNormsArgs<double>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
#endif

}  // namespace ndwt
