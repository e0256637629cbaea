// Host emulation of the order statistics of a band (BandHist / BandPick, csrc/ndwt_device_select.h) -- TEST INFRASTRUCTURE.
// Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports one entry point for the four kinds: float
// real, complex64 (float, COMP = 2), double real, complex128.  The pass loop is the library's (select_impl, ndwt_api.hip), with the
// digits of csrc/ndwt_select.h; the state and the global histogram are one heap block of exactly kSelectBufBytes.
// tests/test_emulated_select.py builds it as a plain shared object; with ndwt_emu_select_main.cpp the same code is a program for
// AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_select.h"

namespace {

template <typename T, int COMP, bool VEC> int run_select(const T* y, long long n, int nk, const long long* k, int nblocks, unsigned long long* keys) {
    typedef ndwt::BandHist<T, COMP, VEC, 2> H;
    typedef ndwt::BandPick<T> P;
    constexpr bool f64 = sizeof(T) == 8;
    std::unique_ptr<char[]> buf(new char[ndwt::kSelectBufBytes]);
    std::memset(buf.get(), 0, ndwt::kSelectBufBytes);
    ndwt::SelectState* st = reinterpret_cast<ndwt::SelectState*>(buf.get());
    unsigned* ghist = reinterpret_cast<unsigned*>(buf.get() + sizeof(ndwt::SelectState));
    const ndwt::SelectTaps tp = {0};
    for (int pass = 0; pass < ndwt::select_passes(f64); ++pass) {
        const int shift = ndwt::select_digit_shift(f64, pass), bits = ndwt::select_digit_bits(f64, pass), top = shift + bits;
        const unsigned long long himask = top >= ndwt::select_key_bits(f64) ? 0ULL : ((~0ULL << top) & (f64 ? ~0ULL : 0xffffffffULL));
        const ndwt::BandHistArgs<T> a = {y, n, st, ghist, himask, shift, bits, nk, nblocks};
        for (int b = 0; b < nblocks; ++b) {
            std::unique_ptr<typename H::Shared> sh(new typename H::Shared);
            EmuExec<typename H::State, H::NT> ex;
            H::block(ex, *sh, a, tp, b);
        }
        ndwt::BandPickArgs pa = {st, ghist, {0, 0, 0, 0}, nk, pass, shift};
        for (int i = 0; i < nk; ++i) pa.k[i] = (unsigned)k[i];
        std::unique_ptr<typename P::Shared> sh(new typename P::Shared);
        EmuExec<typename P::State, P::NT> ex;
        P::block(ex, *sh, pa, tp, 0);
    }
    for (unsigned i = 0; i < ndwt::kSelectHistBytes / sizeof(unsigned); ++i)
        if (ghist[i]) return -3;                                  // the pick leaves the histogram zero
    for (int i = 0; i < nk; ++i) keys[i] = st->prefix[i];
    return 0;
}

template <typename T> int kind(int comp, bool vec, const T* y, long long n, int nk, const long long* k, int nblocks, double* values) {
    unsigned long long keys[ndwt::kSelectMaxRanks] = {};
    const int rc = comp == 2 ? (vec ? run_select<T, 2, true>(y, n, nk, k, nblocks, keys) : run_select<T, 2, false>(y, n, nk, k, nblocks, keys))
                             : (vec ? run_select<T, 1, true>(y, n, nk, k, nblocks, keys) : run_select<T, 1, false>(y, n, nk, k, nblocks, keys));
    if (rc) return rc;
    for (int i = 0; i < nk; ++i) {
        const typename ndwt::SelectKey<T>::type key = (typename ndwt::SelectKey<T>::type)keys[i];
        T v;
        std::memcpy(&v, &key, sizeof v);
        values[i] = (double)v;
    }
    return 0;
}

}  // namespace

// y: n_scalars scalars of the kind (complex: 2 per element); k: nk ranks in [0, elements); vec: 1 the 4-scalar form (y aligned to 4
// scalars and n_scalars a multiple of 4, else -1), 0 one element at a time, -1 what select_vec decides; nblocks: workgroups, 0 = what
// select_grid gives for 256 CUs.  values: nk doubles.  -1: not served (as the library refuses it), -3: the histogram was left dirty.
extern "C" int ndwt_emu_select(int f64, int comp, int vec, const void* y, long long n_scalars, int nk, const long long* k, int nblocks, double* values) {
    if ((comp != 1 && comp != 2) || nk < 1 || nk > ndwt::kSelectMaxRanks || n_scalars < comp || n_scalars % comp != 0) return -1;
    const long long N = n_scalars / comp;
    if (!ndwt::select_fits(N)) return -1;
    for (int i = 0; i < nk; ++i)
        if (k[i] < 0 || k[i] >= N) return -1;
    const bool can_vec = ndwt::select_vec((unsigned long long)(uintptr_t)y, n_scalars, f64 ? 8 : 4);
    if (vec == 1 && !can_vec) return -1;
    const bool v = vec == -1 ? can_vec : vec == 1;
    if (nblocks <= 0) nblocks = (int)ndwt::select_grid(n_scalars, comp, v, 256, 0);
    if (f64) return kind<double>(comp, v, (const double*)y, n_scalars, nk, k, nblocks, values);
    return kind<float>(comp, v, (const float*)y, n_scalars, nk, k, nblocks, values);
}
