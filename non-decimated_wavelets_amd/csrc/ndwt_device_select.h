// ndwt_device_select.h -- exact order statistics of a band's |c| on the device (ndwt_band_select): a radix select on the bit pattern
// of |c|, most significant digit first, in read-only passes over the band.  No sort, no copy, integer counting only: deterministic.
//
// The key of a coefficient is the bit pattern of |c| with the sign cleared (interleaved complex: of the magnitude the shrink compares,
// shrink_magnitude of ndwt_shrink.h), as an unsigned integer of the scalar's width: non-negative IEEE values order as their bit
// patterns, -0 and +0 are one key, and a NaN orders after every number (as numpy sorts it).
//
// A pass is two launches (digit layout: ndwt_select.h, select_digit_shift / select_digit_bits):
//   BandHist  every workgroup reads its share of the band in a grid-stride loop, keeps the keys whose higher digits equal the prefix
//             found so far, counts their current digit into a histogram in LDS (integer LDS atomics) and adds what it counted to the
//             plan's global histogram (no-return integer atomics)
//   BandPick  one workgroup scans the global histogram for the digit whose cumulative count crosses the wanted rank, writes the
//             extended prefix and the rank that remains inside that digit into the device-side state, and zeroes the histogram
// The next pass reads the state; nothing returns to the host in between.  After the last digit the prefix is the complete key.
//
// Up to kSelectMaxRanks ranks are served by the same passes.  Each rank has its slot of the state; a slot whose prefix equals that of
// a lower slot (the two middle ranks of an even count nearly always agree on every digit but the last) is an alias of it: `owner`
// names the lowest slot with the same prefix, only owners are counted, and BandPick reads the owner's histogram for every alias.
//
// Same-bin contention: the first digit of a float key is the exponent and two mantissa bits, so a band of coefficients of similar
// scale puts most lanes of a wave on a handful of counters, and LDS atomics on one address serialise.  count_digit therefore combines
// equal digits across the wave first: for AGG rounds the digit of the first lane still to be counted is broadcast, the lanes that hold
// the same digit are counted with one ballot, and one lane adds their number; what is left after the rounds goes lane by lane.
// Measured: two rounds keep a pass within 154 .. 182 us on a 512^3 float band whatever it holds, none ranges from
// 144 us (benign coefficients) to 468 us (one value).
//
// Written like the fused kernels: per-thread phases driven through an executor (ex.each), separated by barriers, so the same source
// runs under the host emulator, where the atomics are plain adds (count_add).
#pragma once
#include <stddef.h>

#include "ndwt_device.h"
#include "ndwt_select.h"
#include "ndwt_shrink.h"

namespace ndwt {

// the device-side state of a selection, in the plan's select buffer in front of the global histogram; all zero before the first pass
struct SelectState {
    unsigned long long prefix[kSelectMaxRanks];   // the digits found so far, in place (the complete key after the last pass)
    unsigned rank[kSelectMaxRanks];               // the rank that remains among the keys that carry the prefix
    int owner[kSelectMaxRanks];                   // the lowest slot with the same prefix: the one whose histogram counts
};
struct SelectTaps { int unused; };                // (the kernels take no taps; the launch passes the select buffer)
constexpr size_t kSelectHistBytes = sizeof(unsigned) * kSelectMaxRanks * kSelectBins;
constexpr size_t kSelectBufBytes = sizeof(SelectState) + kSelectHistBytes;   // state, then the global histogram [slot][bin]

// The one place a counter is added to.  LDS: a workgroup's histogram, else the global one; the result is not used, so the device
// forms are the no-return integer atomics.  Under the emulator the threads run in turn: a plain add.
template <bool LDS> NDWT_DEV void count_add(unsigned* p, unsigned v) {
#ifdef NDWT_HOST_EMU
    *p += v;
#else
    if (LDS) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// a value every lane of the wave holds alike (read from the state): in a scalar register on the device, so that what depends on it
// is a scalar branch and not a masked one
NDWT_DEV unsigned select_uniform(unsigned v) {
#ifdef NDWT_HOST_EMU
    return v;
#else
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
#endif
}

// hist[digit] += 1 for every lane with `active`, equal digits combined across the wave for AGG rounds first.  Every lane of the wave
// calls it together (the callers' loops run the same number of turns in every lane).
template <int AGG> NDWT_DEV void count_digit(unsigned* hist, unsigned digit, bool active) {
#ifndef NDWT_HOST_EMU
    if constexpr (AGG > 0) {
        unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
        const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        for (int r = 0; r < AGG && todo; ++r) {
            const int leader = __builtin_ctzll(todo);
            const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
            const unsigned long long same = __builtin_amdgcn_ballot_w64(digit == d) & todo;
            if (lane == leader) count_add<true>(hist + d, (unsigned)__builtin_popcountll(same));
            todo &= ~same;
        }
        active = (todo >> lane) & 1;
    }
#endif
    if (active) count_add<true>(hist + digit, 1u);
}

template <typename T> struct SelectKey;
template <> struct SelectKey<float> { typedef unsigned type; };
template <> struct SelectKey<double> { typedef unsigned long long type; };
// the key of |v|: its bits without the sign
template <typename T> NDWT_DEV typename SelectKey<T>::type select_key(T v) {
    typename SelectKey<T>::type k;
    __builtin_memcpy(&k, &v, sizeof k);
    return k & (~(typename SelectKey<T>::type)0 >> 1);
}

template <typename T> struct BandHistArgs {
    const T* y;                        // the band
    long long n;                       // its scalars (interleaved complex: 2 per element)
    const SelectState* st;
    unsigned* ghist;                   // [kSelectMaxRanks][kSelectBins]
    unsigned long long himask;         // the key's bits above the current digit: the prefix lives there
    int shift, bits;                   // the current digit is bits [shift, shift + bits) of the key
    int nk;                            // ranks of the call
    int nblocks;                       // workgroups of the launch
};

// COMP: scalars per element; VEC: 4 scalars per thread and step (the band's address and length are multiples of 4 scalars), else one
// element; AGG: rounds of count_digit
template <typename T, int COMP_, bool VEC_, int AGG_ = 2> struct BandHist {
    static constexpr int COMP = COMP_, AGG = AGG_, NT = 256, WPE = 5;   // (5 workgroups of 32 KB of LDS per CU)
    static constexpr int DEPTH = 4;                       // steps of a thread whose loads are in flight together
    static constexpr bool VEC = VEC_;
    static constexpr int NKEY = VEC ? 4 / COMP : 1;       // keys of one step of a thread
    typedef typename SelectKey<T>::type key_t;
    typedef typename VecT<T>::v4 v4;
    typedef BandHistArgs<T> Args;
    typedef SelectTaps Taps;
    struct Shared { unsigned h[kSelectMaxRanks][kSelectBins]; };
    typedef typename std::conditional<VEC, v4, typename std::conditional<COMP == 2, typename VecT<T>::v2u, T>::type>::type item_t;
    struct State {
        key_t pf[kSelectMaxRanks];     // the prefix of every slot
        unsigned owns;                 // bit r: slot r is an owner
    };
    static NDWT_DEV key_t key_of(const T* c) {
        if constexpr (COMP == 1) return select_key<T>(c[0]);
        else return select_key<T>(shrink_magnitude(c[0], c[1]));
    }
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int bid) {
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            st.owns = 0;
            for (int r = 0; r < kSelectMaxRanks; ++r) {
                const unsigned long long pf = r < a.nk ? a.st->prefix[r] : 0;
                if constexpr (sizeof(key_t) == 8) st.pf[r] = ((key_t)select_uniform((unsigned)(pf >> 32)) << 32) | select_uniform((unsigned)pf);
                else st.pf[r] = select_uniform((unsigned)pf);
                if (r < a.nk && a.st->owner[r] == r) st.owns |= 1u << r;
            }
            st.owns = select_uniform(st.owns);
            for (int r = 0; r < kSelectMaxRanks; ++r)
                if ((st.owns >> r) & 1)
                    for (int i = tid; i < kSelectBins; i += NT) sh.h[r][i] = 0;
        });
        ex.barrier();
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            const long long items = VEC ? a.n / 4 : a.n / COMP;
            const long long step = (long long)a.nblocks * NT;
            const key_t himask = (key_t)a.himask, dmask = (key_t)((1u << a.bits) - 1u);
            const item_t* const src = reinterpret_cast<const item_t*>(a.y);
            const auto load = [&](long long i) __attribute__((always_inline)) { return i < items ? src[i] : item_t(0); };
            // the next DEPTH - 1 steps of the thread are loaded before this one is counted: a workgroup's LDS keeps the CU at 5 waves
            // per SIMD, too few to cover the memory latency with one load each
            const long long first = (long long)bid * NT + tid;
            item_t ahead[DEPTH - 1];
            NDWT_SFOR(d, DEPTH - 1)
                ahead[d] = load(first + d * step);
            NDWT_SEND
            // (the bound is the workgroup's, not the thread's: every lane of a wave makes every turn, as count_digit needs it)
            for (long long base = (long long)bid * NT; base < items; base += step) {
                const long long i = base + tid;
                const bool in = i < items;
                const item_t c = ahead[0];
                NDWT_SFOR(d, DEPTH - 2)
                    ahead[d] = ahead[d + 1];
                NDWT_SEND
                ahead[DEPTH - 2] = load(i + (DEPTH - 1) * step);
                key_t key[NKEY];
                if constexpr (VEC) {
                    const T e[4] = {c[0], c[1], c[2], c[3]};
                    NDWT_SFOR(k, NKEY)
                        key[k] = key_of(e + k * COMP);
                    NDWT_SEND
                } else if constexpr (COMP == 2) {
                    const T e[2] = {c[0], c[1]};
                    key[0] = key_of(e);
                } else {
                    key[0] = key_of(&c);
                }
                NDWT_SFOR(r, kSelectMaxRanks)
                    if ((st.owns >> r) & 1) {
                        NDWT_SFOR(k, NKEY)
                            count_digit<AGG>(sh.h[r], (unsigned)((key[k] >> a.shift) & dmask), in && (key[k] & himask) == st.pf[r]);
                        NDWT_SEND
                    }
                NDWT_SEND
            }
        });
        ex.barrier();
        ex.each([&](int tid, State& st) __attribute__((always_inline)) {
            for (int r = 0; r < kSelectMaxRanks; ++r)
                if ((st.owns >> r) & 1)
                    for (int i = tid; i < kSelectBins; i += NT) {
                        const unsigned v = sh.h[r][i];
                        if (v) count_add<false>(a.ghist + r * kSelectBins + i, v);
                    }
        });
    }
};

struct BandPickArgs {
    SelectState* st;
    unsigned* ghist;
    unsigned k[kSelectMaxRanks];       // the ranks asked for (read in pass 0; afterwards the state's)
    int nk, pass, shift;
};

// The pick of one pass, once: BandPick runs it on the plan's global histogram and state, ItemSelect (ndwt_device_items.h) on its
// workgroup's own in LDS.  Per slot, the digit at which the cumulative count of its owner's histogram passes the slot's rank; the
// extended prefix, the rank that remains inside that digit and the new owner go to `state`.  kPickThreads threads, three phases with
// the executor's barrier between them; the caller's State carries own[kSelectMaxRanks] across them.  rank_of(r): the rank slot r looks
// for in this pass (the first pass: the one asked for; afterwards the state's).  ZERO: the histogram of every slot that was counted is
// zero again for the next pass.
constexpr int kPickThreads = 256, kPickPer = kSelectBins / kPickThreads;
struct PickScratch {
    unsigned part[kSelectMaxRanks][kPickThreads];
    unsigned long long newp[kSelectMaxRanks];
    unsigned newr[kSelectMaxRanks];
};
template <bool ZERO, class State, class Exec, class RankOf>
NDWT_DEV void pick_scan(Exec& ex, PickScratch& sh, unsigned* hist, SelectState* state, RankOf&& rank_of, int nk, int shift) {
    constexpr int NT = kPickThreads, PER = kPickPer;
    ex.each([&](int tid, State& st) __attribute__((always_inline)) {
        for (int r = 0; r < kSelectMaxRanks; ++r) {
            st.own[r] = r < nk ? state->owner[r] : -1;
            if (r >= nk) continue;
            unsigned sum = 0;
            for (int j = 0; j < PER; ++j) sum += hist[st.own[r] * kSelectBins + tid * PER + j];
            sh.part[r][tid] = sum;
        }
    });
    ex.barrier();
    ex.each([&](int tid, State& st) __attribute__((always_inline)) {
        if (tid >= nk) return;
        const int r = tid;
        const unsigned want = rank_of(r);
        unsigned cum = 0;
        int c = 0;
        for (; c < NT - 1; ++c) {                         // (the rank lies below the total by construction: the last chunk takes what is left)
            if (cum + sh.part[r][c] > want) break;
            cum += sh.part[r][c];
        }
        int bin = c * PER;
        for (int j = 0; j < PER - 1; ++j, ++bin) {
            const unsigned v = hist[st.own[r] * kSelectBins + bin];
            if (cum + v > want) break;
            cum += v;
        }
        sh.newp[r] = state->prefix[r] | ((unsigned long long)bin << shift);
        sh.newr[r] = want - cum;
    });
    ex.barrier();
    ex.each([&](int tid, State& st) __attribute__((always_inline)) {
        if (ZERO)
            for (int r = 0; r < kSelectMaxRanks; ++r)
                if (r < nk && st.own[r] == r)
                    for (int j = 0; j < PER; ++j) hist[r * kSelectBins + tid * PER + j] = 0;
        if (tid >= nk) return;
        int o = tid;
        for (int r = tid - 1; r >= 0; --r)
            if (sh.newp[r] == sh.newp[tid]) o = r;
        state->prefix[tid] = sh.newp[tid];
        state->rank[tid] = sh.newr[tid];
        state->owner[tid] = o;
    });
}

// one workgroup: pick_scan on the plan's select buffer
template <typename T> struct BandPick {
    static constexpr int NT = kPickThreads, WPE = 1, PER = kPickPer;
    typedef BandPickArgs Args;
    typedef SelectTaps Taps;
    typedef PickScratch Shared;
    struct State { int own[kSelectMaxRanks]; };
    template <class Exec> static NDWT_DEV void block(Exec& ex, Shared& sh, const Args& a, const Taps&, int) {
        pick_scan<true, State>(ex, sh, a.ghist, a.st,
                               [&](int r) __attribute__((always_inline)) { return a.pass == 0 ? a.k[r] : a.st->rank[r]; }, a.nk, a.shift);
    }
};

#ifndef NDWT_HOST_EMU
// The launches (ndwt_select_f32.hip / ndwt_select_f64.hip): BandHist<T, comp, vec, agg> on a.nblocks workgroups, BandPick<T> on one.
// buf_dev: the plan's select buffer (what the kernels get for a tap table: they read none).  -1: no such instance.
int launch_band_hist(const BandHistArgs<float>& a, int comp, bool vec, int agg, const void* buf_dev, hipStream_t s);
int launch_band_hist(const BandHistArgs<double>& a, int comp, bool vec, int agg, const void* buf_dev, hipStream_t s);
int launch_band_pick(bool f64, const BandPickArgs& a, const void* buf_dev, hipStream_t s);
#endif

}  // namespace ndwt
