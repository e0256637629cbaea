// ndwt_device_items.h -- the kernels of the per-item calls (ndwt_band_select_items, ndwt_shrink_bands_items, ndwt_denoise_bands_items): one
// launch serves every item of a batched plan -- the signals of ndwt_plan_create_many, the images / volumes of a stack, the blocks of
// interleaved samples.  An item's part of a band is one contiguous run of item_vol() scalars, item j at j * item_vol().
//
//   ItemSelect   the whole radix select of ONE item in one workgroup, all items in one launch: the passes of BandHist / BandPick
//                (ndwt_device_select.h) with the histogram, the state and the pick in the workgroup's LDS.  No global histogram, no
//                global atomic, nothing kept between launches; integer counting only, so the keys are those of the band-wide passes run
//                on the item's sub-range, bit for bit.
//   ShrinkItems  shrink_group (ndwt_shrink.h) on every (band, item) block with that block's own threshold, read from a device table
//                [item][band]: all bands and all items in one launch.
//
// Written like the kernels of ndwt_device_select.h: per-thread phases driven through an executor, so the same source runs under the host
// emulator.
#pragma once
#include "ndwt_device_select.h"

namespace ndwt {

template <typename T> struct ItemSelectArgs {
    const T* y;                        // item 0's part of the band
    long long n;                       // scalars of ONE item (interleaved complex: 2 per element); item j starts at j * n
    unsigned long long* keys;          // [items][kSelectMaxRanks]: slot r of item j, one 64-bit word for either key width
    unsigned k[kSelectMaxRanks];       // the ranks asked for, the same for every item
    int nk;
};

// COMP, VEC, AGG: as BandHist's (VEC: every item's address and length are multiples of 4 scalars).  Workgroup `bid` is item `bid`.
// Shared is the histogram of BandHist (32 KB) plus the scratch of the pick (4 KB) and the state: 36 KB, four workgroups to the CU.
template <typename T, int COMP_, bool VEC_, int AGG_ = 2> struct ItemSelect {
    typedef BandHist<T, COMP_, VEC_, AGG_> H;             // its keys, its steps, its depth of loads in flight
    static constexpr int COMP = COMP_, AGG = AGG_, NT = kPickThreads, WPE = 4, DEPTH = H::DEPTH, NKEY = H::NKEY;
    static constexpr bool VEC = VEC_, F64 = sizeof(T) == 8;
    typedef typename H::key_t key_t;
    typedef typename H::item_t item_t;
    typedef ItemSelectArgs<T> Args;
    typedef SelectTaps Taps;
    struct Shared {
        unsigned h[kSelectMaxRanks][kSelectBins];
        PickScratch pick;
        SelectState st;
    };
    struct State {
        key_t pf[kSelectMaxRanks];     // the prefix of every slot
        unsigned owns;                 // bit r: slot r is an owner
        int own[kSelectMaxRanks];      // (pick_scan's)
    };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            if (tid < kSelectMaxRanks) { sh.st.prefix[tid] = 0; sh.st.rank[tid] = 0; sh.st.owner[tid] = 0; }
        });
        ex.barrier();
        for (int pass = 0; pass < select_passes(F64); ++pass) {
            const int shift = select_digit_shift(F64, pass), bits = select_digit_bits(F64, pass), top = shift + bits;
            ex.each([&](int tid, State& st) __attribute__((always_inline)) {
                st.owns = 0;
                for (int r = 0; r < kSelectMaxRanks; ++r) {
                    const unsigned long long pf = r < a.nk ? sh.st.prefix[r] : 0;
                    if constexpr (F64) st.pf[r] = ((key_t)select_uniform((unsigned)(pf >> 32)) << 32) | select_uniform((unsigned)pf);
                    else st.pf[r] = select_uniform((unsigned)pf);
                    if (r < a.nk && sh.st.owner[r] == r) st.owns |= 1u << r;
                }
                st.owns = select_uniform(st.owns);
                for (int r = 0; r < kSelectMaxRanks; ++r)
                    if ((st.owns >> r) & 1)
                        for (int i = tid; i < kSelectBins; i += NT) sh.h[r][i] = 0;
            });
            ex.barrier();
            ex.each([&](int tid, State& st) __attribute__((always_inline)) {
                const long long steps = VEC ? a.n / 4 : a.n / COMP;
                const key_t himask = top >= select_key_bits(F64) ? (key_t)0 : (key_t)(~(key_t)0 << top), dmask = (key_t)((1u << bits) - 1u);
                const item_t* const src = reinterpret_cast<const item_t*>(a.y + (long long)bid * a.n);
                const auto load = [&](long long i) __attribute__((always_inline)) { return i < steps ? src[i] : item_t(0); };
                item_t ahead[DEPTH - 1];
                NDWT_SFOR(d, DEPTH - 1)
                    ahead[d] = load((long long)tid + d * NT);
                NDWT_SEND
                // (the bound is the workgroup's, not the thread's: every lane of a wave makes every turn, as count_digit needs it)
                for (long long base = 0; base < steps; base += NT) {
                    const long long i = base + tid;
                    const bool in = i < steps;
                    const item_t c = ahead[0];
                    NDWT_SFOR(d, DEPTH - 2)
                        ahead[d] = ahead[d + 1];
                    NDWT_SEND
                    ahead[DEPTH - 2] = load(i + (long long)(DEPTH - 1) * NT);
                    key_t key[NKEY];
                    if constexpr (VEC) {
                        const T e[4] = {c[0], c[1], c[2], c[3]};
                        NDWT_SFOR(k, NKEY)
                            key[k] = H::key_of(e + k * COMP);
                        NDWT_SEND
                    } else if constexpr (COMP == 2) {
                        const T e[2] = {c[0], c[1]};
                        key[0] = H::key_of(e);
                    } else {
                        key[0] = H::key_of(&c);
                    }
                    NDWT_SFOR(r, kSelectMaxRanks)
                        if ((st.owns >> r) & 1) {
                            NDWT_SFOR(k, NKEY)
                                count_digit<AGG>(sh.h[r], (unsigned)((key[k] >> shift) & dmask), in && (key[k] & himask) == st.pf[r]);
                            NDWT_SEND
                        }
                    NDWT_SEND
                }
            });
            ex.barrier();
            pick_scan<false, State>(ex, sh.pick, &sh.h[0][0], &sh.st,
                                    [&](int r) __attribute__((always_inline)) { return pass == 0 ? a.k[r] : sh.st.rank[r]; }, a.nk, shift);
            ex.barrier();
        }
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            if (tid < a.nk) a.keys[(long long)bid * kSelectMaxRanks + tid] = sh.st.prefix[tid];
        });
    }
};

template <typename T> struct ShrinkItemsArgs {
    T* y;                              // band 0 of the coefficient array
    long long band_pitch;              // scalars from one band to the next
    long long n;                       // scalars of ONE item of a band; item j of band b starts at b * band_pitch + j * n
    const T* table;                    // device, [items][nb]: the thresholds in the plan's scalar type; 0 = leave the block alone
    long long items;
    int nb;                            // bands of the table (and of the launch, counted from band0)
    int band0, nbands;                 // the launch covers bands band0 .. band0 + nbands - 1
    int chunks;                        // workgroups per (band, item) block
    int hard;
};

// Workgroup `bid` is (band, item, chunk), chunk fastest.  VEC: 4 scalars per thread and step -- y, band_pitch and n are multiples of 4
// scalars, so every block is; else one element (the rule of shrink_run, for every block at once).  Per element the arithmetic and the
// order are shrink_kernel's: the values are those of shrink_kernel run on each block with its threshold.
template <typename T, int COMP_, bool VEC_> struct ShrinkItems {
    static constexpr int COMP = COMP_, NT = 256, WPE = 8;
    static constexpr bool VEC = VEC_;
    typedef ShrinkItemsArgs<T> Args;
    typedef SelectTaps Taps;
    struct Shared { int unused; };
    struct State { int unused; };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared&, const Args& a, const Taps&, int bid) {
        const int chunk = bid % a.chunks;
        const long long bi = bid / a.chunks, item = bi % a.items;
        const int band = a.band0 + (int)(bi / a.items);
        const T thr = a.table[item * a.nb + band];
        if (thr == T(0)) return;
        T* const d = a.y + band * a.band_pitch + item * a.n;
        ex.each([&](int tid, State&) __attribute__((always_inline)) {
            const long long t0 = (long long)chunk * NT + tid, stride = (long long)a.chunks * NT;
            if constexpr (VEC) {
                typedef typename VecT<T>::v4 v4;
                v4* const dv = reinterpret_cast<v4*>(d);
                for (long long i = t0; i < a.n / 4; i += stride) {
                    const v4 c = dv[i];
                    T e[4] = {c[0], c[1], c[2], c[3]};
                    NDWT_UNROLL
                    for (int k = 0; k < 4; k += COMP) shrink_group<T, COMP>(e + k, thr, a.hard);
                    dv[i] = v4{e[0], e[1], e[2], e[3]};
                }
            } else {
                for (long long i = t0; i < a.n / COMP; i += stride) shrink_group<T, COMP>(d + i * COMP, thr, a.hard);
            }
        });
    }
};

#ifndef NDWT_HOST_EMU
// The launches (ndwt_select_items_f32.hip / _f64.hip): ItemSelect<T, comp, vec> on `items` workgroups, ShrinkItems<T, comp, vec> on
// nbands * items * chunks.  buf_dev: a device buffer of the plan (what the kernels get for a tap table: they read none).  -1: no such
// instance.
int launch_item_select(const ItemSelectArgs<float>& a, int comp, bool vec, int items, const void* buf_dev, hipStream_t s);
int launch_item_select(const ItemSelectArgs<double>& a, int comp, bool vec, int items, const void* buf_dev, hipStream_t s);
int launch_shrink_items(const ShrinkItemsArgs<float>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
int launch_shrink_items(const ShrinkItemsArgs<double>& a, int comp, bool vec, const void* buf_dev, hipStream_t s);
#endif

}  // namespace ndwt
