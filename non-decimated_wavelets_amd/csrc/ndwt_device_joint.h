// ndwt_device_joint.h -- the kernels of ndwt_shrink_joint / ndwt_denoise_joint / ndwt_group_norms*: joint shrinkage across the items of
// a batched, stack or interleaved plan (the prox of the l2,1 norm: group soft thresholding) and the norms of the groups, each in one
// launch.  The group at position p of band b is the K = items coefficients y[b][j][p], j = 0 .. K - 1: the same position of every item.
//
//   JointShrink  every workgroup takes a chunk of the positions of one band; per position the sum of squares over the items, one
//                magnitude, one gain, and every item's coefficient scaled by it (or stored as zero).  REG: the K coefficients of a step
//                stay in registers -- one read, one write; else two sweeps over the items, the second reads them again.
//   GroupNorms   the first sweep alone with the accumulators and the combine of BandNorms (ndwt_device_norms.h); NormsFinish adds the
//                chunks of a band.
//
// Per group, T the plan's scalar type: s = the sum over j ascending of re_j^2 (+ im_j^2, re before im) in double, every square added
// with an explicit fma on the widened parts, from 0 (as norms_add accumulates l2); m = sqrt((T)s) in T; m > t: every part of every c_j
// times g = hard ? 1 : (m - t) / m in T; else every part is stored as +0 -- an explicit zero, so a group that holds a NaN (m > t is
// false) becomes zeros, as the real form of shrink_group does.  The norms: l1 = the sum of m (widened), l2sq = the sum of s, max = the
// largest m (a NaN sticks: norms_max), nnz = the count of groups with s != 0 (a NaN counts; a group of -0 does not).
//
// Item j of a step lies j * n scalars further on, so a wave's load is one contiguous KiB in the 4-scalar form whatever K.  No
// floating-point atomics; the order of every sum is that of BandNorms: a fixed function of the shape and the launch geometry.
//
// Written like the kernels of ndwt_device_items.h: per-thread phases driven through an executor, so the same source runs under the host
// emulator.
#pragma once
#include "ndwt_device_norms.h"

namespace ndwt {

// what a thread moves in one step: 4 scalars (VEC), else one element
template <typename T, int COMP, bool VEC> struct JointStep {
    typedef typename std::conditional<VEC, typename VecT<T>::v4, typename std::conditional<COMP == 2, NormsPair<T>, T>::type>::type item_t;
    static constexpr int W = VEC ? 4 : COMP, NPOS = W / COMP;       // scalars and positions (groups) of a step
    static NDWT_DEV void unpack(const item_t& c, T* e) {
        if constexpr (VEC) { e[0] = c[0]; e[1] = c[1]; e[2] = c[2]; e[3] = c[3]; }
        else if constexpr (COMP == 2) { e[0] = c.v[0]; e[1] = c.v[1]; }
        else e[0] = c;
    }
    static NDWT_DEV item_t pack(const T* e) {
        if constexpr (VEC) return item_t{e[0], e[1], e[2], e[3]};
        else if constexpr (COMP == 2) return item_t{{e[0], e[1]}};
        else return e[0];
    }
    // s[p] += the squares of item c's parts at every position p of the step
    static NDWT_DEV void add(double* s, const item_t& c) {
        T e[W];
        unpack(c, e);
        NDWT_SFOR(k, W)
            s[k / COMP] = __builtin_fma((double)e[k], (double)e[k], s[k / COMP]);
        NDWT_SEND
    }
    // the group's gain from its sum of squares; false: the group goes to zero
    static NDWT_DEV bool gain(double s, T thr, int hard, T* g) {
        const T m = sqrt((T)s);
        if (!(m > thr)) return false;
        *g = hard ? T(1) : (m - thr) / m;
        return true;
    }
    static NDWT_DEV item_t scaled(const item_t& c, const bool* keep, const T* g) {
        T e[W];
        unpack(c, e);
        NDWT_SFOR(k, W)
            e[k] = keep[k / COMP] ? e[k] * g[k / COMP] : T(0);
        NDWT_SEND
        return pack(e);
    }
};

template <typename T> struct JointShrinkArgs {
    T* y;                              // band 0 of the coefficient array
    long long band_pitch;              // scalars from one band to the next
    long long n;                       // scalars of ONE item of a band; item j of band b starts at b * band_pitch + j * n
    const T* table;                    // device, [nb]: the thresholds in the plan's scalar type; 0 = leave the band alone
    long long items;                   // K
    int nb;                            // bands of the table and of the launch
    int chunks;                        // workgroups per band
    int hard;
};

// Workgroup `bid` is (band, chunk), chunk fastest.  VEC: y, band_pitch and n are multiples of 4 scalars (the rule of ShrinkItems).
// REG (items <= kJointReg): the item loop is unrolled with a predicate on j < items, all loads of a step are issued before the first
// use and the group stays in registers.  !REG: DEPTH loads in flight in either sweep, as ItemSelect's ahead[].
template <typename T, int COMP_, bool VEC_, bool REG_> struct JointShrink {
    static constexpr int COMP = COMP_, NT = 256, WPE = 4, DEPTH = 4, KREG = kJointReg;
    static constexpr bool VEC = VEC_, REG = REG_;
    typedef JointStep<T, COMP, VEC> S;
    typedef typename S::item_t item_t;
    typedef JointShrinkArgs<T> Args;
    typedef SelectTaps Taps;
    struct Shared { int unused; };
    struct State { int unused; };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared&, const Args& a, const Taps&, int bid) {
        const int chunk = bid % a.chunks, band = bid / a.chunks;
        const T thr = a.table[band];
        if (thr == T(0)) return;
        T* const d = a.y + band * a.band_pitch;
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            const long long steps = VEC ? a.n / 4 : a.n / COMP, stride = (long long)a.chunks * NT, K = a.items;
            const auto at = [&](long long j, long long i) __attribute__((always_inline)) { return reinterpret_cast<item_t*>(d + j * a.n) + i; };
            for (long long i = (long long)chunk * NT + tid; i < steps; i += stride) {
                double s[S::NPOS];
                NDWT_SFOR(k, S::NPOS)
                    s[k] = 0.0;
                NDWT_SEND
                T g[S::NPOS];
                bool keep[S::NPOS];
                if constexpr (REG) {
                    item_t c[KREG];
                    NDWT_SFOR(j, KREG)
                        if (j < K) c[j] = *at(j, i);
                    NDWT_SEND
                    NDWT_SFOR(j, KREG)
                        if (j < K) S::add(s, c[j]);
                    NDWT_SEND
                    NDWT_SFOR(k, S::NPOS)
                        keep[k] = S::gain(s[k], thr, a.hard, &g[k]);
                    NDWT_SEND
                    NDWT_SFOR(j, KREG)
                        if (j < K) *at(j, i) = S::scaled(c[j], keep, g);
                    NDWT_SEND
                } else {
                    const auto load = [&](long long j) __attribute__((always_inline)) { return j < K ? *at(j, i) : item_t{}; };
                    item_t ahead[DEPTH - 1];
                    NDWT_SFOR(k, DEPTH - 1)
                        ahead[k] = load(k);
                    NDWT_SEND
                    for (long long j = 0; j < K; ++j) {
                        const item_t c = ahead[0];
                        NDWT_SFOR(k, DEPTH - 2)
                            ahead[k] = ahead[k + 1];
                        NDWT_SEND
                        ahead[DEPTH - 2] = load(j + DEPTH - 1);
                        S::add(s, c);
                    }
                    NDWT_SFOR(k, S::NPOS)
                        keep[k] = S::gain(s[k], thr, a.hard, &g[k]);
                    NDWT_SEND
                    NDWT_SFOR(k, DEPTH - 1)
                        ahead[k] = load(k);
                    NDWT_SEND
                    for (long long j = 0; j < K; ++j) {
                        const item_t c = ahead[0];
                        NDWT_SFOR(k, DEPTH - 2)
                            ahead[k] = ahead[k + 1];
                        NDWT_SEND
                        ahead[DEPTH - 2] = load(j + DEPTH - 1);
                        *at(j, i) = S::scaled(c, keep, g);
                    }
                }
            }
        });
    }
};

template <typename T> struct GroupNormsArgs {
    const T* y;                        // band 0 of the coefficient array
    long long band_pitch, n;           // as JointShrinkArgs
    double* out;                       // chunks == 1: the results [nb][4]; else the partials [band][chunk][4] (NormsFinish's, one item)
    long long items;                   // K
    int nb;
    int chunks;                        // workgroups per band
};

// Workgroup `bid` is (band, chunk), chunk fastest.  A thread walks its steps in ascending order and the items of a step in ascending
// order; the loads of that one sequence run DEPTH - 1 ahead, across the end of a step, so that a plan of one item has as many in flight
// as a plan of many.  A load past the thread's last step loads nothing.
template <typename T, int COMP_, bool VEC_> struct GroupNorms {
    static constexpr int COMP = COMP_, NT = 256, WPE = 8, DEPTH = 4;
    static constexpr bool VEC = VEC_;
    typedef JointStep<T, COMP, VEC> S;
    typedef typename S::item_t item_t;
    typedef GroupNormsArgs<T> Args;
    typedef SelectTaps Taps;
    typedef NormsShared<NT> Shared;
    struct State { int unused; };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        const int chunk = bid % a.chunks, band = bid / a.chunks;
        const T* const d = a.y + band * a.band_pitch;
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            const long long steps = VEC ? a.n / 4 : a.n / COMP, stride = (long long)a.chunks * NT, K = a.items;
            long long qi = (long long)chunk * NT + tid, qj = 0;   // the next load of the sequence: step qi, item qj
            const auto load = [&]() __attribute__((always_inline)) {
                const item_t c = qi < steps ? reinterpret_cast<const item_t*>(d + qj * a.n)[qi] : item_t{};
                if (++qj == K) { qj = 0; qi += stride; }
                return c;
            };
            NormsAcc acc = {0.0, 0.0, 0.0, 0ULL};
            item_t ahead[DEPTH - 1];
            NDWT_SFOR(k, DEPTH - 1)
                ahead[k] = load();
            NDWT_SEND
            for (long long i = (long long)chunk * NT + tid; i < steps; i += stride) {
                double s[S::NPOS];
                NDWT_SFOR(k, S::NPOS)
                    s[k] = 0.0;
                NDWT_SEND
                for (long long j = 0; j < K; ++j) {
                    const item_t c = ahead[0];
                    NDWT_SFOR(k, DEPTH - 2)
                        ahead[k] = ahead[k + 1];
                    NDWT_SEND
                    ahead[DEPTH - 2] = load();
                    S::add(s, c);
                }
                NDWT_SFOR(k, S::NPOS)
                    const double m = (double)(T)sqrt((T)s[k]);
                    acc.l1 += m;
                    acc.l2 += s[k];
                    acc.mx = norms_max(acc.mx, m);
                    acc.nz += s[k] != 0.0;
                NDWT_SEND
            }
            sh.l1[tid] = acc.l1;
            sh.l2[tid] = acc.l2;
            sh.mx[tid] = acc.mx;
            sh.nz[tid] = acc.nz;
        });
        norms_tree<NT, State>(ex, sh);
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            if (tid != 0) return;
            norms_write<NT>(sh, a.chunks == 1 ? a.out + (long long)band * 4 : a.out + ((long long)band * a.chunks + chunk) * 4);
        });
    }
};

#ifndef NDWT_HOST_EMU
// The launches (ndwt_joint_f32.hip / ndwt_joint_f64.hip): JointShrink<T, comp, vec, reg> and GroupNorms<T, comp, vec> on nb * chunks
// workgroups.  buf_dev: a device buffer of the plan (what the kernels get for a tap table: they read none).  -1: no such instance, -2: a
// grid the launch cannot express, or reg with more items than kJointReg.
int launch_joint_shrink(const JointShrinkArgs<float>& a, int comp, bool vec, bool reg, const void* buf_dev, hipStream_t s);
int launch_joint_shrink(const JointShrinkArgs<double>& a, int comp, bool vec, bool reg, const void* buf_dev, hipStream_t s);
int launch_group_norms(const GroupNormsArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
int launch_group_norms(const GroupNormsArgs<double>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
#endif

}  // namespace ndwt
