// Host emulation of the one-launch denoise of a batched 1-D plan (Den1C, csrc/ndwt_device_1d.h) -- TEST INFRASTRUCTURE.
// Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports one entry point for the four kinds: float
// real (EW = 1), complex64 (float, EW = 2), double real, complex128.  tests/test_emulated_den1c.py builds it as a plain shared
// object; with ndwt_emu_den1c_main.cpp the same code is a program for AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_1d.h"

namespace {

// taps: [4][kMaxTaps] -- analysis lo, analysis hi, synthesis lo, synthesis hi in kernel form, the first L of each read
template <class K, typename T> int run_den1(ndwt::Den1CArgs<T>& a, const double* taps) {
    a.nseg = (a.row + K::WX - 1) / K::WX;
    std::vector<T> table;                                     // Taps1D<T, L> as the library uploads it: both directions, axis 0 filled
    ndwt::append_taps3(table, emu_taps_d(taps, taps + ndwt::kMaxTaps, K::L, 1), false);
    ndwt::append_taps3(table, emu_taps_d(taps + 2 * ndwt::kMaxTaps, taps + 3 * ndwt::kMaxTaps, K::L, 1), false);
    typename K::Taps tp;
    emu_load_taps(tp, table);
    const long long nblocks = (a.outer * a.nseg + K::NT / 64 - 1) / (K::NT / 64);
    for (long long b = 0; b < nblocks; ++b) {
        typename K::Shared sh;
        EmuExec<typename K::State, K::NT> ex;
        K::block(ex, sh, a, tp, (int)b);
    }
    return 0;
}

template <typename T, int EW> int kind(int L, int nlev, ndwt::Den1CArgs<T>& a, const double* taps) {
#define CASE1(LL, NL) \
    if (L == LL && nlev == NL) return run_den1<ndwt::Den1C<T, LL, NL, EW>, T>(a, taps);
#define CASE1L(LL) CASE1(LL, 1) CASE1(LL, 2) CASE1(LL, 3) CASE1(LL, 4)
    CASE1L(2) CASE1L(4) CASE1L(6) CASE1L(8)
#undef CASE1L
#undef CASE1
    return -1;
}

}  // namespace

// one translation unit per kind (EMU_D1_PART 1 .. 4; 0: the entry point), so that the test builds them in parallel
#ifndef EMU_D1_PART
#define EMU_D1_IN(part) 1
#else
#define EMU_D1_IN(part) (EMU_D1_PART == part)
#endif
int emu_d1_f32(int L, int nlev, ndwt::Den1CArgs<float>& a, const double* taps);
int emu_d1_c64(int L, int nlev, ndwt::Den1CArgs<float>& a, const double* taps);
int emu_d1_f64(int L, int nlev, ndwt::Den1CArgs<double>& a, const double* taps);
int emu_d1_c128(int L, int nlev, ndwt::Den1CArgs<double>& a, const double* taps);
#if EMU_D1_IN(1)
int emu_d1_f32(int L, int nlev, ndwt::Den1CArgs<float>& a, const double* taps) { return kind<float, 1>(L, nlev, a, taps); }
#endif
#if EMU_D1_IN(2)
int emu_d1_c64(int L, int nlev, ndwt::Den1CArgs<float>& a, const double* taps) { return kind<float, 2>(L, nlev, a, taps); }
#endif
#if EMU_D1_IN(3)
int emu_d1_f64(int L, int nlev, ndwt::Den1CArgs<double>& a, const double* taps) { return kind<double, 1>(L, nlev, a, taps); }
#endif
#if EMU_D1_IN(4)
int emu_d1_c128(int L, int nlev, ndwt::Den1CArgs<double>& a, const double* taps) { return kind<double, 2>(L, nlev, a, taps); }
#endif

#if EMU_D1_IN(0)
namespace {
template <typename T> int den1_kind(int ew, int L, int nlev, const T* in, T* out, long long row, long long outer, const double* taps,
                                    const double* thr, int hard) {
    if (nlev < 1 || nlev > 4 || row < 4 || row % 4 != 0 || outer < 1) return -1;
    ndwt::Den1CArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.row = row; a.outer = outer;
    a.in[0] = in;
    a.out[0] = out;
    a.thr[0] = (T)thr[0];
    for (int l = 0; l < nlev; ++l) a.thr[1 + l] = (T)thr[nlev - l];   // cascade level l (0 = finest) is transform level l + 1: band nlev - l
    a.hard = hard;
    if constexpr (sizeof(T) == 4) return ew == 2 ? emu_d1_c64(L, nlev, a, taps) : emu_d1_f32(L, nlev, a, taps);
    else return ew == 2 ? emu_d1_c128(L, nlev, a, taps) : emu_d1_f64(L, nlev, a, taps);
}
}  // namespace

// in / out: `outer` rows of `row` scalars (complex: 2 per element), two buffers that do not overlap; taps: [4][20] analysis lo / hi,
// synthesis lo / hi in kernel form; thr: 1 + nlev thresholds in the band order of the coefficient array (band 0 the approximation)
extern "C" int ndwt_emu1_denoise(int f64, int ew, int L, int nlev, const void* in, void* out, long long row, long long outer, const double* taps,
                                 const double* thr, int hard) {
    if (ew != 1 && ew != 2) return -1;
    if (f64) return den1_kind<double>(ew, L, nlev, (const double*)in, (double*)out, row, outer, taps, thr, hard);
    return den1_kind<float>(ew, L, nlev, (const float*)in, (float*)out, row, outer, taps, thr, hard);
}
#endif
