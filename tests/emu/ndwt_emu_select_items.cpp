// Host emulation of the per-item kernels (ItemSelect / ShrinkItems, csrc/ndwt_device_items.h) -- TEST INFRASTRUCTURE.
// Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports three entry points for the four kinds: float
// real, complex64 (float, COMP = 2), double real, complex128.
//   ndwt_emu_select_items   ItemSelect: one workgroup per item, the keys in a heap block of exactly items x kSelectMaxRanks words
//   ndwt_emu_band_pick      BandPick alone on a histogram and a state the caller supplies (what the refactoring of its scan into
//                           pick_scan must leave as it was)
//   ndwt_emu_shrink_items   ShrinkItems on every (band, item, chunk) workgroup
// tests/test_emulated_select_items.py builds it as a plain shared object; with ndwt_emu_select_items_main.cpp the same code is a program
// for AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_items.h"

namespace {

template <typename T, int COMP, bool VEC> int run_items(const T* y, long long n, long long items, int nk, const long long* k, double* values) {
    typedef ndwt::ItemSelect<T, COMP, VEC> K;
    std::unique_ptr<unsigned long long[]> keys(new unsigned long long[(size_t)items * ndwt::kSelectMaxRanks]);
    for (size_t i = 0; i < (size_t)items * ndwt::kSelectMaxRanks; ++i) keys[i] = ~0ULL;
    ndwt::ItemSelectArgs<T> a = {y, n, keys.get(), {0, 0, 0, 0}, nk};
    for (int i = 0; i < nk; ++i) a.k[i] = (unsigned)k[i];
    const ndwt::SelectTaps tp = {0};
    for (long long b = 0; b < items; ++b) {
        std::unique_ptr<typename K::Shared> sh(new typename K::Shared);
        std::memset(sh.get(), 0xA5, sizeof(typename K::Shared));   // (LDS holds anything when a workgroup starts)
        EmuExec<typename K::State, K::NT> ex;
        K::block(ex, *sh, a, tp, (int)b);
    }
    for (long long j = 0; j < items; ++j) {
        for (int i = 0; i < ndwt::kSelectMaxRanks; ++i) {
            const unsigned long long w = keys[(size_t)j * ndwt::kSelectMaxRanks + i];
            if (i >= nk) {
                if (w != ~0ULL) return -4;                           // a slot that was not asked for is not written
                continue;
            }
            const typename ndwt::SelectKey<T>::type key = (typename ndwt::SelectKey<T>::type)w;
            if ((unsigned long long)key != w) return -5;             // one 64-bit word per rank, the key in its low bits
            T v;
            std::memcpy(&v, &key, sizeof v);
            values[j * nk + i] = (double)v;
        }
    }
    return 0;
}

template <typename T> int items_kind(int comp, bool vec, const T* y, long long n, long long items, int nk, const long long* k, double* values) {
    return comp == 2 ? (vec ? run_items<T, 2, true>(y, n, items, nk, k, values) : run_items<T, 2, false>(y, n, items, nk, k, values))
                     : (vec ? run_items<T, 1, true>(y, n, items, nk, k, values) : run_items<T, 1, false>(y, n, items, nk, k, values));
}

template <typename T, int COMP, bool VEC> void run_shrink(const ndwt::ShrinkItemsArgs<T>& a) {
    typedef ndwt::ShrinkItems<T, COMP, VEC> K;
    const ndwt::SelectTaps tp = {0};
    for (long long b = 0; b < (long long)a.nbands * a.items * a.chunks; ++b) {
        typename K::Shared sh = {0};
        EmuExec<typename K::State, K::NT> ex;
        K::block(ex, sh, a, tp, (int)b);
    }
}

template <typename T> int shrink_kind(int comp, T* y, long long pitch, long long n, const double* thr, long long items, int nb, int chunks, int hard) {
    std::unique_ptr<T[]> table(new T[(size_t)items * nb]);         // (exactly items x nb scalars)
    for (size_t i = 0; i < (size_t)items * nb; ++i) table[i] = (T)thr[i];
    const bool vec = (uintptr_t)y % (4 * sizeof(T)) == 0 && pitch % 4 == 0 && n % 4 == 0;
    const ndwt::ShrinkItemsArgs<T> a = {y, pitch, n, table.get(), items, nb, 0, nb, chunks, hard};
    if (comp == 2) { if (vec) run_shrink<T, 2, true>(a); else run_shrink<T, 2, false>(a); }
    else { if (vec) run_shrink<T, 1, true>(a); else run_shrink<T, 1, false>(a); }
    return vec ? 1 : 0;
}

}  // namespace

// y: items x n_scalars scalars of the kind, item j at j * n_scalars (complex: 2 per element); k: nk ranks in [0, elements of one item);
// vec: 1 the 4-scalar form (y aligned to 4 scalars and n_scalars a multiple of 4, else -1), 0 one element at a time, -1 what select_vec
// decides.  values: items x nk doubles.  -1: not served (as the library refuses it), -4 / -5: the keys array was written wrongly.
extern "C" int ndwt_emu_select_items(int f64, int comp, int vec, const void* y, long long n_scalars, long long items, int nk, const long long* k,
                                     double* values) {
    if ((comp != 1 && comp != 2) || nk < 1 || nk > ndwt::kSelectMaxRanks || n_scalars < comp || n_scalars % comp != 0 || items < 1) return -1;
    const long long N = n_scalars / comp;
    if (!ndwt::select_fits(N)) return -1;
    for (int i = 0; i < nk; ++i)
        if (k[i] < 0 || k[i] >= N) return -1;
    const bool can_vec = ndwt::select_vec((unsigned long long)(uintptr_t)y, n_scalars, f64 ? 8 : 4);
    if (vec == 1 && !can_vec) return -1;
    const bool v = vec == -1 ? can_vec : vec == 1;
    if (f64) return items_kind<double>(comp, v, (const double*)y, n_scalars, items, nk, k, values);
    return items_kind<float>(comp, v, (const float*)y, n_scalars, items, nk, k, values);
}

// One BandPick step.  state: prefix[4] (64-bit), then rank[4], then owner[4] (32-bit) -- SelectState; hist: [4][2048] counters.  Both are
// updated in place, as the kernel leaves them.
extern "C" int ndwt_emu_band_pick(int f64, void* state, unsigned* hist, const unsigned* k, int nk, int pass, int shift) {
    static_assert(sizeof(ndwt::SelectState) == 64, "the layout the test writes");
    ndwt::BandPickArgs pa = {(ndwt::SelectState*)state, hist, {k[0], k[1], k[2], k[3]}, nk, pass, shift};
    const ndwt::SelectTaps tp = {0};
    if (f64) {
        typedef ndwt::BandPick<double> P;
        std::unique_ptr<P::Shared> sh(new P::Shared);
        EmuExec<P::State, P::NT> ex;
        P::block(ex, *sh, pa, tp, 0);
    } else {
        typedef ndwt::BandPick<float> P;
        std::unique_ptr<P::Shared> sh(new P::Shared);
        EmuExec<P::State, P::NT> ex;
        P::block(ex, *sh, pa, tp, 0);
    }
    return 0;
}

// y: nb bands at `pitch` scalars, each items x n_scalars; thr: [items][nb] doubles (converted as the library converts them).  Returns 1 if
// the 4-scalar form ran, 0 for the element-wise one.
extern "C" int ndwt_emu_shrink_items(int f64, int comp, void* y, long long pitch, long long n_scalars, const double* thr, long long items, int nb,
                                     int chunks, int hard) {
    if ((comp != 1 && comp != 2) || n_scalars % comp != 0 || items < 1 || nb < 1 || chunks < 1 || pitch < items * n_scalars) return -1;
    if (f64) return shrink_kind<double>(comp, (double*)y, pitch, n_scalars, thr, items, nb, chunks, hard);
    return shrink_kind<float>(comp, (float*)y, pitch, n_scalars, thr, items, nb, chunks, hard);
}
