// Host emulation of the cascaded 2-D kernels (Fwd2C / Inv2C) on double and interleaved complex data -- TEST INFRASTRUCTURE.
// Takes EmuExec and the tap helpers from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports one entry point for the
// three kinds: complex64 (float, EW = 2), double real (EW = 1), complex128 (double, EW = 2).  tests/test_emulated_cascade2_kinds.py builds
// it as a plain shared object; with ndwt_emu_cascade2_kinds_main.cpp the same code is a program for AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"

namespace {

template <class K, class A> int run_cascade(A& a, const double* lo, const double* hi, int ychunk) {
    typedef typename std::remove_reference<decltype(typename K::Taps().lo[0][0])>::type T;
    a.ntx = (a.n1 + K::WX - 1) / K::WX;
    a.ychunk = ychunk > 0 ? (ychunk < a.n2 ? ychunk : a.n2) : a.n2;
    a.nyc = (a.n2 + a.ychunk - 1) / a.ychunk;
    const typename K::Taps tp = emu_taps3<K, T>(lo, hi);
    for (int b = 0; b < a.ntx * a.nyc; ++b) {
        typename K::Shared sh;
        EmuExec<typename K::State, K::NT> ex;
        K::block(ex, sh, a, tp, b);
    }
    return 0;
}

#undef EMU_IN
// one translation unit per kind and direction (EMU_KINDS_PART 1 .. 6; 0: the entry point), so that the test builds them in parallel
#ifndef EMU_KINDS_PART
#define EMU_IN(part) 1
#else
#define EMU_IN(part) (EMU_KINDS_PART == part)
#endif

template <typename T, int EW> int fwd_kind(int Lp, int nlev, ndwt::Fused2CArgs<T>& a, const double* lo, const double* hi, int ychunk) {
#define CASEC(LL) case LL: return nlev == 3 ? run_cascade<ndwt::Fwd2C<T, LL, 3, 2, EW>>(a, lo, hi, ychunk) : run_cascade<ndwt::Fwd2C<T, LL, 2, 2, EW>>(a, lo, hi, ychunk);
    switch (Lp) {
        CASEC(2) CASEC(4) CASEC(6) CASEC(8)
        default: return -1;
    }
#undef CASEC
}
template <typename T, int EW> int inv_kind(int Lp, int nlev, int depth, ndwt::Fused2CIArgs<T>& a, const double* lo, const double* hi, int ychunk) {
#define CASEC(LL)                                                                                                        \
    case LL:                                                                                                             \
        if constexpr (sizeof(T) == 4) {   /* two rows of band loads in flight: complex64 only */                         \
            if (depth == 2) return nlev == 3 ? run_cascade<ndwt::Inv2C<T, LL, 3, 2, 2, EW>>(a, lo, hi, ychunk)           \
                                             : run_cascade<ndwt::Inv2C<T, LL, 2, 2, 2, EW>>(a, lo, hi, ychunk);          \
        }                                                                                                                \
        if (depth != 1) return -1;                                                                                       \
        return nlev == 3 ? run_cascade<ndwt::Inv2C<T, LL, 3, 1, 2, EW>>(a, lo, hi, ychunk) : run_cascade<ndwt::Inv2C<T, LL, 2, 1, 2, EW>>(a, lo, hi, ychunk);
    switch (Lp) {
        CASEC(2) CASEC(4) CASEC(6) CASEC(8)
        default: return -1;
    }
#undef CASEC
}

}  // namespace

int emu_kinds_fwd_c64(int Lp, int nlev, ndwt::Fused2CArgs<float>& a, const double* lo, const double* hi, int ychunk);
int emu_kinds_fwd_f64(int Lp, int nlev, ndwt::Fused2CArgs<double>& a, const double* lo, const double* hi, int ychunk);
int emu_kinds_fwd_c128(int Lp, int nlev, ndwt::Fused2CArgs<double>& a, const double* lo, const double* hi, int ychunk);
int emu_kinds_inv_c64(int Lp, int nlev, int depth, ndwt::Fused2CIArgs<float>& a, const double* lo, const double* hi, int ychunk);
int emu_kinds_inv_f64(int Lp, int nlev, int depth, ndwt::Fused2CIArgs<double>& a, const double* lo, const double* hi, int ychunk);
int emu_kinds_inv_c128(int Lp, int nlev, int depth, ndwt::Fused2CIArgs<double>& a, const double* lo, const double* hi, int ychunk);
#if EMU_IN(1)
int emu_kinds_fwd_c64(int Lp, int nlev, ndwt::Fused2CArgs<float>& a, const double* lo, const double* hi, int ychunk) { return fwd_kind<float, 2>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(2)
int emu_kinds_fwd_f64(int Lp, int nlev, ndwt::Fused2CArgs<double>& a, const double* lo, const double* hi, int ychunk) { return fwd_kind<double, 1>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(3)
int emu_kinds_fwd_c128(int Lp, int nlev, ndwt::Fused2CArgs<double>& a, const double* lo, const double* hi, int ychunk) { return fwd_kind<double, 2>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(4)
int emu_kinds_inv_c64(int Lp, int nlev, int depth, ndwt::Fused2CIArgs<float>& a, const double* lo, const double* hi, int ychunk) { return inv_kind<float, 2>(Lp, nlev, depth, a, lo, hi, ychunk); }
#endif
#if EMU_IN(5)
int emu_kinds_inv_f64(int Lp, int nlev, int depth, ndwt::Fused2CIArgs<double>& a, const double* lo, const double* hi, int ychunk) { return inv_kind<double, 1>(Lp, nlev, depth, a, lo, hi, ychunk); }
#endif
#if EMU_IN(6)
int emu_kinds_inv_c128(int Lp, int nlev, int depth, ndwt::Fused2CIArgs<double>& a, const double* lo, const double* hi, int ychunk) { return inv_kind<double, 2>(Lp, nlev, depth, a, lo, hi, ychunk); }
#endif

#if EMU_IN(0)
namespace {
template <typename T> int cascade_kind(int inverse, int ew, int Lp, int nlev, int depth, const T* in, T* out, int n1, int n2, int ychunk, const double* lo,
                                       const double* hi, double shrink_thr, int shrink_hard) {
    if (nlev != 2 && nlev != 3) return -1;
    const long long band = (long long)n1 * n2;
    if (!inverse) {
        ndwt::Fused2CArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        a.in = in; a.n1 = n1; a.n2 = n2; a.rs = n1;
        for (int b = 0; b < 1 + 3 * nlev; ++b) a.out[b] = out + b * band;
        if constexpr (sizeof(T) == 4) return emu_kinds_fwd_c64(Lp, nlev, a, lo, hi, ychunk);
        else return ew == 2 ? emu_kinds_fwd_c128(Lp, nlev, a, lo, hi, ychunk) : emu_kinds_fwd_f64(Lp, nlev, a, lo, hi, ychunk);
    } else {
        ndwt::Fused2CIArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        a.out = out; a.n1 = n1; a.n2 = n2; a.rs = n1;
        for (int b = 0; b < 1 + 3 * nlev; ++b) a.in[b] = in + b * band;
        if (shrink_thr > 0) { a.shrink_on = 1; a.shrink_thr = (T)shrink_thr; a.shrink_hard = shrink_hard; }
        if constexpr (sizeof(T) == 4) return emu_kinds_inv_c64(Lp, nlev, depth, a, lo, hi, ychunk);
        else return ew == 2 ? emu_kinds_inv_c128(Lp, nlev, depth, a, lo, hi, ychunk) : emu_kinds_inv_f64(Lp, nlev, depth, a, lo, hi, ychunk);
    }
}
}  // namespace

// in / out: n1 scalars per row (complex: 2 per element), n2 rows, 1 + 3 nlev bands in the reference's order on the coefficient side.
// f64 = 0 takes interleaved complex64 only (float real data has ndwt_emu2_cascade_f32 / _inv_f32 in ndwt_emu.cpp).
extern "C" int ndwt_emu2_cascade_kinds(int inverse, int f64, int ew, int Lp, int nlev, int depth, const void* in, void* out, int n1, int n2, int ychunk,
                                       const double* lo, const double* hi, double shrink_thr, int shrink_hard) {
    if (f64) return cascade_kind<double>(inverse, ew, Lp, nlev, depth, (const double*)in, (double*)out, n1, n2, ychunk, lo, hi, shrink_thr, shrink_hard);
    if (ew != 2) return -1;
    return cascade_kind<float>(inverse, ew, Lp, nlev, depth, (const float*)in, (float*)out, n1, n2, ychunk, lo, hi, shrink_thr, shrink_hard);
}
#endif
