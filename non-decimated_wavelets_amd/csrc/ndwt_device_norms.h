// ndwt_device_norms.h -- the kernels of ndwt_band_norms / ndwt_band_norms_items / ndwt_band_norms_dev: four sums of every (band, item)
// block of a coefficient array in one read of it -- the l1 norm, the energy, the largest magnitude and the count of non-zeros.
//
//   BandNorms    every workgroup reads its chunk of one (band, item) block in a grid-stride loop, each thread with its four accumulators
//                in registers; the workgroup combines them in LDS and one thread writes the four values: the block's own (chunks == 1)
//                or the chunk's partials
//   NormsFinish  one small workgroup per (band, item) combines the partials of its chunks (chunks > 1 only): the reduce at the launch
//                boundary -- no counter, no hand-off between workgroups inside a launch
//
// Per element (NDWT_NORM_*, include/ndwt.h): real data |c|, c^2, |c| and c != 0; interleaved complex data m = sqrt(re^2 + im^2) in the
// scalar type, the magnitude the shrink compares and the select orders (norms_magnitude, below), re^2 + im^2 from the widened parts, m,
// and re != 0 || im != 0.  Everything is accumulated in double, the squares with an explicit fma (the host build and the device build then agree whatever the
// compiler contracts), the count in a 64-bit integer that becomes a double when it is written.  A NaN makes l1, l2sq and max of its
// block NaN (the comparison of norms_max is written so that a NaN sticks: the hardware's max would drop it) and counts as non-zero; -0
// is zero.
//
// No floating-point atomics: a thread adds its steps in ascending order, the workgroup's 256 x 4 values go through a fixed halving tree
// in LDS (thread t takes t + 128, then t + 64, ...), the chunks of a block are added in ascending order per lane of NormsFinish and go
// through the same tree.  The order of every sum is a fixed function of the shape and the launch geometry: two calls on one device give
// the same bits, and the host emulator -- no wave intrinsics here -- reproduces the order exactly.
//
// Written like the kernels of ndwt_device_items.h: per-thread phases driven through an executor, so the same source runs under the host
// emulator.
#pragma once
#include "ndwt_device_select.h"

namespace ndwt {

// max with a NaN that sticks: a NaN on either side gives a NaN
NDWT_DEV double norms_max(double acc, double m) { return (m > acc || m != m) ? m : acc; }

// the four accumulators of a thread
struct NormsAcc {
    double l1, l2, mx;
    unsigned long long nz;
};
// The magnitude of an interleaved complex element, bit for bit the one the select kernels order (BandHist / ItemSelect; NDWT_NORM_MAX is
// their last order statistic).  Their source, shrink_magnitude, leaves the rounding of re^2 + im^2 to the compiler, which fuses re^2
// into the sum -- fma(re, re, im * im) -- everywhere but in the element-wise float form, where both products are rounded (a packed
// multiply).  Here the two forms are written out, so that they stay what they are; tests/test_gpu_norms.py holds them to the select.
template <typename T, bool VEC> NDWT_DEV T norms_magnitude(T re, T im) {
    if constexpr (sizeof(T) == 4 && !VEC) {
#pragma clang fp contract(off)
        const T a = re * re, b = im * im;
        return sqrt(a + b);
    } else if constexpr (sizeof(T) == 4) {
        return sqrt(__builtin_fmaf(re, re, im * im));
    } else {
        return sqrt(__builtin_fma(re, re, im * im));
    }
}

template <typename T, int COMP, bool VEC> NDWT_DEV void norms_add(NormsAcc& s, const T* c) {
    if constexpr (COMP == 1) {
        const T m = c[0] < T(0) ? -c[0] : c[0];
        s.l1 += (double)m;
        s.l2 = __builtin_fma((double)c[0], (double)c[0], s.l2);
        s.mx = norms_max(s.mx, (double)m);
        s.nz += c[0] != T(0);
    } else {
        const T m = norms_magnitude<T, VEC>(c[0], c[1]);
        s.l1 += (double)m;
        s.l2 = __builtin_fma((double)c[0], (double)c[0], s.l2);
        s.l2 = __builtin_fma((double)c[1], (double)c[1], s.l2);
        s.mx = norms_max(s.mx, (double)m);
        s.nz += (c[0] != T(0)) | (c[1] != T(0));
    }
}

// The combine of a workgroup of NT threads: every thread's four values in LDS, then the halving tree, a barrier after every level.
// Afterwards entry 0 holds the workgroup's values (read them behind the last barrier).
template <int NT> struct NormsShared {
    double l1[NT], l2[NT], mx[NT];
    unsigned long long nz[NT];
};
template <int NT, class State, class Exec> NDWT_DEV void norms_tree(Exec& ex, NormsShared<NT>& sh) {
    for (int half = NT / 2; half >= 1; half /= 2) {
        ex.barrier();
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            if (tid >= half) return;
            sh.l1[tid] += sh.l1[tid + half];
            sh.l2[tid] += sh.l2[tid + half];
            sh.mx[tid] = norms_max(sh.mx[tid], sh.mx[tid + half]);
            sh.nz[tid] += sh.nz[tid + half];
        });
    }
    ex.barrier();
}
// the four values of entry 0 to dst[0 .. 4): two 16-byte vector stores (dst is 8-byte aligned)
template <int NT> NDWT_DEV void norms_write(const NormsShared<NT>& sh, double* dst) {
    typedef typename VecT<double>::v2u d2;
    *reinterpret_cast<d2*>(dst) = d2{sh.l1[0], sh.l2[0]};
    *reinterpret_cast<d2*>(dst + 2) = d2{sh.mx[0], (double)sh.nz[0]};
}

// one interleaved complex element, aligned as its scalars are (the element-wise form reads blocks at any scalar offset)
template <typename T> struct NormsPair { T v[2]; };

template <typename T> struct BandNormsArgs {
    const T* y;                        // band 0 of the coefficient array
    long long band_pitch;              // scalars from one band to the next
    long long n;                       // scalars of ONE item of a band; item j of band b starts at b * band_pitch + j * n
    double* out;                       // chunks == 1: the results [item][nb][4]; else the partials [band][item][chunk][4]
    long long items;
    int nb;                            // bands of the coefficient array
    int band0, nbands;                 // the launch covers bands band0 .. band0 + nbands - 1
    int chunks;                        // workgroups per (band, item) block
};

// Workgroup `bid` is (band, item, chunk), chunk fastest.  VEC: 4 scalars per thread and step through one 16- / 32-byte load -- y,
// band_pitch and n are multiples of 4 scalars, so every block is; else one element per step (the rule of ShrinkItems, for every block at
// once).  DEPTH steps of a thread have their loads in flight together, as in BandHist; a step past the block's end loads nothing and
// adds zeros, which change none of the four values.
template <typename T, int COMP_, bool VEC_> struct BandNorms {
    static constexpr int COMP = COMP_, NT = 256, WPE = 8, DEPTH = 4;
    static constexpr bool VEC = VEC_;
    typedef BandNormsArgs<T> Args;
    typedef SelectTaps Taps;
    typedef NormsShared<NT> Shared;
    typedef typename VecT<T>::v4 v4;
    typedef typename std::conditional<VEC, v4, typename std::conditional<COMP == 2, NormsPair<T>, T>::type>::type item_t;
    struct State { int unused; };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        const int chunk = bid % a.chunks;
        const long long bi = bid / a.chunks, item = bi % a.items;
        const int band = a.band0 + (int)(bi / a.items);
        const T* const d = a.y + band * a.band_pitch + item * a.n;
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            const long long steps = VEC ? a.n / 4 : a.n / COMP, stride = (long long)a.chunks * NT;
            const item_t* const src = reinterpret_cast<const item_t*>(d);
            const auto load = [&](long long i) __attribute__((always_inline)) { return i < steps ? src[i] : item_t{}; };
            NormsAcc s = {0.0, 0.0, 0.0, 0ULL};
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
                        norms_add<T, COMP, true>(s, e + k * COMP);
                    NDWT_SEND
                } else if constexpr (COMP == 2) {
                    norms_add<T, 2, false>(s, c.v);
                } else {
                    norms_add<T, 1, false>(s, &c);
                }
            }
            sh.l1[tid] = s.l1;
            sh.l2[tid] = s.l2;
            sh.mx[tid] = s.mx;
            sh.nz[tid] = s.nz;
        });
        norms_tree<NT, State>(ex, sh);
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            if (tid != 0) return;
            norms_write<NT>(sh, a.chunks == 1 ? a.out + (item * a.nb + band) * 4 : a.out + (((long long)band * a.items + item) * a.chunks + chunk) * 4);
        });
    }
};

struct NormsFinishArgs {
    const double* part;                // the partials of BandNorms: [band][item][chunk][4]
    double* out;                       // the results [item][nb][4]
    long long items;
    int nb;
    int band0, nbands;                 // as BandNormsArgs
    int chunks;
};

// Workgroup `bid` is (band, item).  Partial c goes to lane c mod NT, a lane adds its partials in ascending c, the lanes go through the
// tree of BandNorms.  (The count is a whole number below 2^53 in every partial: it returns to the integer exactly.)
template <int NT_ = 64> struct NormsFinish {
    static constexpr int NT = NT_, WPE = 1;
    typedef NormsFinishArgs Args;
    typedef SelectTaps Taps;
    typedef NormsShared<NT> Shared;
    struct State { int unused; };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        const long long item = bid % a.items;
        const int band = a.band0 + (int)(bid / a.items);
        const double* const p = a.part + ((long long)band * a.items + item) * a.chunks * 4;
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            NormsAcc s = {0.0, 0.0, 0.0, 0ULL};
            for (int c = tid; c < a.chunks; c += NT) {
                s.l1 += p[4 * c];
                s.l2 += p[4 * c + 1];
                s.mx = norms_max(s.mx, p[4 * c + 2]);
                s.nz += (unsigned long long)p[4 * c + 3];
            }
            sh.l1[tid] = s.l1;
            sh.l2[tid] = s.l2;
            sh.mx[tid] = s.mx;
            sh.nz[tid] = s.nz;
        });
        norms_tree<NT, State>(ex, sh);
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            if (tid != 0) return;
            norms_write<NT>(sh, a.out + (item * a.nb + band) * 4);
        });
    }
};

#ifndef NDWT_HOST_EMU
// The launches (ndwt_norms_f32.hip / ndwt_norms_f64.hip): BandNorms<T, comp, vec> on nbands * items * chunks workgroups, NormsFinish on
// nbands * items.  buf_dev: a device buffer of the plan (what the kernels get for a tap table: they read none).  -1: no such instance,
// -2: a grid the launch cannot express.
int launch_band_norms(const BandNormsArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
int launch_band_norms(const BandNormsArgs<double>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
int launch_norms_finish(const NormsFinishArgs& a, const void* buf_dev, hipStream_t s);
#endif

}  // namespace ndwt
