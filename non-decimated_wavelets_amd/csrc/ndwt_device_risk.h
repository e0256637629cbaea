// ndwt_device_risk.h -- the kernels of ndwt_band_risk / ndwt_band_risk_items: what Stein's unbiased risk estimate of a soft threshold
// needs of every (band, item) block of a coefficient array, at up to NDWT_RISK_MAX_CAND candidate thresholds in one read of the array.
//
//   BandRisk    every workgroup reads its chunk of one (band, item) block in the grid-stride loop of BandNorms, each thread with its
//               accumulators of every candidate in registers; the workgroup combines them in LDS, candidate after candidate, and one
//               thread writes the block's own values (chunks == 1) or the chunk's partials
//   RiskFinish  one small workgroup per (band, item) combines the partials of its chunks (chunks > 1 only), as NormsFinish does
//
// Per element and candidate t (NDWT_RISK_*, include/ndwt.h), with m the magnitude the shrink compares -- |c| of real data,
// norms_magnitude<T, VEC> of interleaved complex data -- and the comparison made in the scalar type, as the shrink makes it:
//   count    elements with !(m > t): those a shrink at t sets to zero (a NaN is one of them)
//   energy   c^2 (re^2 + im^2) of those elements, accumulated in double from the widened parts with an explicit fma, as norms_add
//            accumulates l2: at t = +inf the steps of a thread are those of NDWT_NORM_L2SQ
//   invsum   complex data only: 1.0 / (double)m of the elements with m > t
// The magnitude, the widened parts and the reciprocal are computed once per element; a candidate costs a comparison and its predicated
// accumulations.  The candidate loop is unrolled (NDWT_SFOR) under the uniform predicate i < nc: the accumulators are indexed by
// constants only and stay in registers.
//
// The thresholds of a block are a row of a device table in the scalar type, [item][band][nc]; a row whose first entry is negative skips
// its block: the workgroup writes zeros from one thread and returns before it loads anything of the array.
//
// No floating-point atomics: a thread adds its steps in ascending order, the workgroup's values go through the fixed halving tree of
// norms_tree (one candidate's three values at a time through one buffer), the chunks of a block are added in ascending order per lane
// of RiskFinish and go through the same tree.  Two calls on one device give the same bits, and the host emulator -- no wave intrinsics
// here -- reproduces the order exactly.
#pragma once
#include "ndwt_device_norms.h"

namespace ndwt {

constexpr int kRiskMaxCand = 8;        // NDWT_RISK_MAX_CAND
// the elements a thread of BandRisk sees at most: its steps of the grid-stride loop, each of 4 scalars or of one element
constexpr long long risk_thread_elements(long long item_scalars, int comp, bool vec, long long chunks) {
    return ((vec ? item_scalars / 4 : item_scalars / comp) / (256 * chunks) + 1) * (vec ? 4 / comp : 1);
}

// The combine of a workgroup of NT threads for ONE candidate: every thread's three values in LDS, then the halving tree of norms_tree.
// Afterwards entry 0 holds the workgroup's values (read them behind the last barrier).
template <int NT> struct RiskShared {
    double en[NT], inv[NT];
    unsigned long long cnt[NT];
};
template <int NT, int COMP, class State, class Exec> NDWT_DEV void risk_tree(Exec& ex, RiskShared<NT>& sh) {
    for (int half = NT / 2; half >= 1; half /= 2) {
        ex.barrier();
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            if (tid >= half) return;
            sh.cnt[tid] += sh.cnt[tid + half];
            sh.en[tid] += sh.en[tid + half];
            if constexpr (COMP == 2) sh.inv[tid] += sh.inv[tid + half];
        });
    }
    ex.barrier();
}

template <typename T> struct BandRiskArgs {
    const T* y;                        // band 0 of the coefficient array
    long long band_pitch;              // scalars from one band to the next
    long long n;                       // scalars of ONE item of a band; item j of band b starts at b * band_pitch + j * n
    const T* cand;                     // the thresholds [item][nb][nc]; a row that begins with a negative entry skips its block
    double* out;                       // chunks == 1: the results [item][nb][nc][3]; else the partials [band][item][chunk][nc][3]
    long long items;
    int nb;                            // bands of the coefficient array
    int band0, nbands;                 // the launch covers bands band0 .. band0 + nbands - 1
    int chunks;                        // workgroups per (band, item) block
    int nc;                            // candidates of every block, 1 .. kRiskMaxCand
};

// Workgroup `bid` is (band, item, chunk), chunk fastest; the loop, VEC and DEPTH are those of BandNorms.
template <typename T, int COMP_, bool VEC_> struct BandRisk {
    static constexpr int COMP = COMP_, NT = 256, WPE = 4, DEPTH = 4, NC = kRiskMaxCand;
    static constexpr bool VEC = VEC_;
    typedef BandRiskArgs<T> Args;
    typedef SelectTaps Taps;
    typedef RiskShared<NT> Shared;
    typedef typename VecT<T>::v4 v4;
    typedef typename std::conditional<VEC, v4, typename std::conditional<COMP == 2, NormsPair<T>, T>::type>::type item_t;
    // a thread's accumulators live across the phases of the combine.  Its counts are 32-bit (the workgroup's are not): the host refuses a
    // block of which a thread would see 2^32 elements (risk_thread_elements)
    struct State {
        double en[NC], inv[NC];
        unsigned int cnt[NC];
    };
    // one element: c[0 .. COMP) against the nc thresholds
    static NDWT_DEV void add(State& st, const T (&thr)[NC], int nc, const T* c) {
        T m;
        double w0 = (double)c[0], w1 = 0.0, r = 0.0;
        if constexpr (COMP == 1) {
            m = c[0] < T(0) ? -c[0] : c[0];
        } else {
            m = norms_magnitude<T, VEC>(c[0], c[1]);
            w1 = (double)c[1];
            r = 1.0 / (double)m;
        }
        NDWT_SFOR(i, NC)
            if (i < nc) {
                if (m > thr[i]) {
                    if constexpr (COMP == 2) st.inv[i] += r;
                } else {
                    st.cnt[i] += 1;
                    st.en[i] = __builtin_fma(w0, w0, st.en[i]);
                    if constexpr (COMP == 2) st.en[i] = __builtin_fma(w1, w1, st.en[i]);
                }
            }
        NDWT_SEND
    }
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        const int chunk = bid % a.chunks, nc = a.nc;
        const long long bi = bid / a.chunks, item = bi % a.items;
        const int band = a.band0 + (int)(bi / a.items);
        const T* const row = a.cand + (item * a.nb + band) * nc;
        double* const dst = a.chunks == 1 ? a.out + (item * a.nb + band) * nc * 3 : a.out + ((((long long)band * a.items + item) * a.chunks + chunk) * nc) * 3;
        if (row[0] < T(0)) {                              // a skipped block: zeros, and nothing of the array is read
            ex.each([&](int tid, State&) __attribute__((always_inline)) {
                if (tid != 0) return;
                for (int k = 0; k < nc * 3; ++k) dst[k] = 0.0;
            });
            return;
        }
        const T* const d = a.y + band * a.band_pitch + item * a.n;
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            T thr[NC];
            NDWT_SFOR(i, NC)
                thr[i] = i < nc ? row[i] : T(0);
                st.cnt[i] = 0u;
                st.en[i] = 0.0;
                st.inv[i] = 0.0;
            NDWT_SEND
            const long long steps = VEC ? a.n / 4 : a.n / COMP, stride = (long long)a.chunks * NT;
            const item_t* const src = reinterpret_cast<const item_t*>(d);
            const auto load = [&](long long i) __attribute__((always_inline)) { return i < steps ? src[i] : item_t{}; };
            const long long first = (long long)chunk * NT + tid;
            item_t ahead[DEPTH - 1];
            NDWT_SFOR(k, DEPTH - 1)
                ahead[k] = load(first + k * stride);
            NDWT_SEND
            for (long long i = first; i < steps; i += stride) {
                const item_t c = ahead[0];
                NDWT_SFOR(k, DEPTH - 2)
                    ahead[k] = ahead[k + 1];
                NDWT_SEND
                ahead[DEPTH - 2] = load(i + (DEPTH - 1) * stride);
                if constexpr (VEC) {
                    const T e[4] = {c[0], c[1], c[2], c[3]};
                    NDWT_SFOR(k, 4 / COMP)
                        add(st, thr, nc, e + k * COMP);
                    NDWT_SEND
                } else if constexpr (COMP == 2) {
                    add(st, thr, nc, c.v);
                } else {
                    add(st, thr, nc, &c);
                }
            }
        });
        NDWT_SFOR(i, NC)
            if (i < nc) {
                ex.each([&](int tid, State& st) __attribute__((always_inline)) {
                    sh.cnt[tid] = st.cnt[i];
                    sh.en[tid] = st.en[i];
                    if constexpr (COMP == 2) sh.inv[tid] = st.inv[i];
                });
                risk_tree<NT, COMP, State>(ex, sh);
                ex.each([&](int tid, State&) __attribute__((always_inline)) {
                    if (tid != 0) return;
                    dst[3 * i] = (double)sh.cnt[0];
                    dst[3 * i + 1] = sh.en[0];
                    dst[3 * i + 2] = COMP == 2 ? sh.inv[0] : 0.0;
                });
            }
        NDWT_SEND
    }
};

struct RiskFinishArgs {
    const double* part;                // the partials of BandRisk: [band][item][chunk][nc][3]
    double* out;                       // the results [item][nb][nc][3]
    long long items;
    int nb;
    int band0, nbands;                 // as BandRiskArgs
    int chunks;
    int nc;
};

// Workgroup `bid` is (band, item).  Candidate after candidate: partial c goes to lane c mod NT, a lane adds its partials in ascending c,
// the lanes go through the tree of BandRisk.  (The count is a whole number below 2^53 in every partial: it returns to the integer
// exactly.  The partials of a skipped block are zeros, and so is their sum.)
template <int NT_ = 64> struct RiskFinish {
    static constexpr int NT = NT_, WPE = 1;
    typedef RiskFinishArgs Args;
    typedef SelectTaps Taps;
    typedef RiskShared<NT> Shared;
    struct State { int unused; };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        const long long item = bid % a.items;
        const int band = a.band0 + (int)(bid / a.items);
        const double* const p = a.part + ((long long)band * a.items + item) * a.chunks * a.nc * 3;
        double* const dst = a.out + (item * a.nb + band) * a.nc * 3;
        for (int i = 0; i < a.nc; ++i) {
            ex.each([&](int tid, State&) __attribute__((always_inline)) {
                unsigned long long cnt = 0ULL;
                double en = 0.0, inv = 0.0;
                for (int c = tid; c < a.chunks; c += NT) {
                    const double* const q = p + ((long long)c * a.nc + i) * 3;
                    cnt += (unsigned long long)q[0];
                    en += q[1];
                    inv += q[2];
                }
                sh.cnt[tid] = cnt;
                sh.en[tid] = en;
                sh.inv[tid] = inv;
            });
            risk_tree<NT, 2, State>(ex, sh);
            ex.each([&](int tid, State&) __attribute__((always_inline)) {
                if (tid != 0) return;
                dst[3 * i] = (double)sh.cnt[0];
                dst[3 * i + 1] = sh.en[0];
                dst[3 * i + 2] = sh.inv[0];
            });
        }
    }
};

#ifndef NDWT_HOST_EMU
// The launches (ndwt_risk_f32.hip / ndwt_risk_f64.hip): BandRisk<T, comp, vec> on nbands * items * chunks workgroups, RiskFinish on
// nbands * items.  buf_dev: a device buffer of the plan (what the kernels get for a tap table: they read none).  -1: no such instance,
// -2: a grid or a candidate count the launch cannot express.
int launch_band_risk(const BandRiskArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
int launch_band_risk(const BandRiskArgs<double>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
int launch_risk_finish(const RiskFinishArgs& a, const void* buf_dev, hipStream_t s);
#endif

}  // namespace ndwt
