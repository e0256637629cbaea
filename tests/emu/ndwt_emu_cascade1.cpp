// Host emulation of the cascaded 1-D kernels of a batched plan (Fwd1C / Inv1C, csrc/ndwt_device_1d.h) -- TEST INFRASTRUCTURE.
// Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports one entry point for the four kinds: float
// real (EW = 1), complex64 (float, EW = 2), double real, complex128.  tests/test_emulated_cascade1.py builds it as a plain shared
// object; with ndwt_emu_cascade1_main.cpp the same code is a program for AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_1d.h"

namespace {

template <class K, typename T> int run_cascade1(ndwt::Fused1CArgs<T>& a, const double* lo, const double* hi) {
    a.nseg = (a.row + K::WX - 1) / K::WX;
    const typename K::Taps tp = emu_taps3<K, T>(lo, hi, 1);   // the table of a 1-D plan: axis 0, the other axes zero
    const long long nblocks = (a.outer * a.nseg + K::NT / 64 - 1) / (K::NT / 64);
    for (long long b = 0; b < nblocks; ++b) {
        typename K::Shared sh;
        EmuExec<typename K::State, K::NT> ex;
        K::block(ex, sh, a, tp, (int)b);
    }
    return 0;
}

template <typename T, int EW> int kind(int inverse, int L, int nlev, ndwt::Fused1CArgs<T>& a, const double* lo, const double* hi) {
#define CASE1(LL, NL)                                                                                 \
    if (L == LL && nlev == NL)                                                                        \
        return inverse ? run_cascade1<ndwt::Inv1C<T, LL, NL, EW>, T>(a, lo, hi) : run_cascade1<ndwt::Fwd1C<T, LL, NL, EW>, T>(a, lo, hi);
#define CASE1L(LL) CASE1(LL, 2) CASE1(LL, 3) CASE1(LL, 4)
    CASE1L(2) CASE1L(4) CASE1L(6) CASE1L(8)
#undef CASE1L
#undef CASE1
    return -1;
}

}  // namespace

// one translation unit per kind (EMU_C1_PART 1 .. 4; 0: the entry point), so that the test builds them in parallel
#ifndef EMU_C1_PART
#define EMU_C1_IN(part) 1
#else
#define EMU_C1_IN(part) (EMU_C1_PART == part)
#endif
int emu_c1_f32(int inverse, int L, int nlev, ndwt::Fused1CArgs<float>& a, const double* lo, const double* hi);
int emu_c1_c64(int inverse, int L, int nlev, ndwt::Fused1CArgs<float>& a, const double* lo, const double* hi);
int emu_c1_f64(int inverse, int L, int nlev, ndwt::Fused1CArgs<double>& a, const double* lo, const double* hi);
int emu_c1_c128(int inverse, int L, int nlev, ndwt::Fused1CArgs<double>& a, const double* lo, const double* hi);
#if EMU_C1_IN(1)
int emu_c1_f32(int inverse, int L, int nlev, ndwt::Fused1CArgs<float>& a, const double* lo, const double* hi) { return kind<float, 1>(inverse, L, nlev, a, lo, hi); }
#endif
#if EMU_C1_IN(2)
int emu_c1_c64(int inverse, int L, int nlev, ndwt::Fused1CArgs<float>& a, const double* lo, const double* hi) { return kind<float, 2>(inverse, L, nlev, a, lo, hi); }
#endif
#if EMU_C1_IN(3)
int emu_c1_f64(int inverse, int L, int nlev, ndwt::Fused1CArgs<double>& a, const double* lo, const double* hi) { return kind<double, 1>(inverse, L, nlev, a, lo, hi); }
#endif
#if EMU_C1_IN(4)
int emu_c1_c128(int inverse, int L, int nlev, ndwt::Fused1CArgs<double>& a, const double* lo, const double* hi) { return kind<double, 2>(inverse, L, nlev, a, lo, hi); }
#endif

#if EMU_C1_IN(0)
namespace {
template <typename T> int cascade1_kind(int inverse, int ew, int L, int nlev, const T* in, T* out, long long row, long long outer, const double* lo,
                                        const double* hi) {
    if (nlev < 2 || nlev > 4 || row < 4 || row % 4 != 0 || outer < 1) return -1;
    const long long band = row * outer;
    ndwt::Fused1CArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.row = row; a.outer = outer;
    if (!inverse) {                                       // cascade level l (0 = finest) is transform level l + 1: band 1 + (nlev - (l + 1))
        a.in[0] = in;
        a.out[0] = out;
        for (int l = 0; l < nlev; ++l) a.out[1 + l] = out + (long long)(nlev - l) * band;
    } else {                                              // cascade level c (0 = coarsest) is transform level nlev - c: band 1 + c
        for (int b = 0; b < 1 + nlev; ++b) a.in[b] = in + (long long)b * band;
        a.out[0] = out;
    }
    if constexpr (sizeof(T) == 4) return ew == 2 ? emu_c1_c64(inverse, L, nlev, a, lo, hi) : emu_c1_f32(inverse, L, nlev, a, lo, hi);
    else return ew == 2 ? emu_c1_c128(inverse, L, nlev, a, lo, hi) : emu_c1_f64(inverse, L, nlev, a, lo, hi);
}
}  // namespace

// in / out: `outer` rows of `row` scalars (complex: 2 per element) per band, 1 + nlev bands in the reference's order on the coefficient
// side; lo / hi: the L taps of the direction in kernel form
extern "C" int ndwt_emu1_cascade(int inverse, int f64, int ew, int L, int nlev, const void* in, void* out, long long row, long long outer,
                                 const double* lo, const double* hi) {
    if (ew != 1 && ew != 2) return -1;
    if (f64) return cascade1_kind<double>(inverse, ew, L, nlev, (const double*)in, (double*)out, row, outer, lo, hi);
    return cascade1_kind<float>(inverse, ew, L, nlev, (const float*)in, (float*)out, row, outer, lo, hi);
}
#endif
