// Host emulation of the cascaded 2-D kernels (Fwd2C / Inv2C) on a STACK of images -- TEST INFRASTRUCTURE.
// The kernels take the item from the block id and add its offset to their base pointers; here every wave of every item runs in turn,
// as the launch of cascade2_launch lays them out: ntx * nyc * nbatch blocks, the item the slowest part of the block id.
// Takes EmuExec and the tap helpers from ndwt_emu.cpp (an EMU_PART that selects none of its parts).  Four kinds (float, complex64,
// double, complex128) x both directions, the instances the test asks for: 8 taps x 3 levels, 4 taps x 2 levels, 2 taps x 3 levels.
// tests/test_emulated_stack2.py builds it as a plain shared object; with ndwt_emu_stack2_main.cpp the same code is a program for
// AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"

namespace {

template <class K, class A> int run_stack(A& a, const double* lo, const double* hi, int ychunk) {
    typedef typename std::remove_reference<decltype(typename K::Taps().lo[0][0])>::type T;
    a.ntx = (a.n1 + K::WX - 1) / K::WX;
    a.ychunk = ychunk > 0 ? (ychunk < a.n2 ? ychunk : a.n2) : a.n2;
    a.nyc = (a.n2 + a.ychunk - 1) / a.ychunk;
    const typename K::Taps tp = emu_taps3<K, T>(lo, hi);
    const int nblocks = a.ntx * a.nyc * (a.nbatch > 1 ? a.nbatch : 1);
    for (int b = 0; b < nblocks; ++b) {
        typename K::Shared sh;
        EmuExec<typename K::State, K::NT> ex;
        K::block(ex, sh, a, tp, b);
    }
    return 0;
}

template <typename T, int EW> int fwd_stack(int Lp, int nlev, ndwt::Fused2CArgs<T>& a, const double* lo, const double* hi, int ychunk) {
    if (Lp == 8 && nlev == 3) return run_stack<ndwt::Fwd2C<T, 8, 3, 2, EW>>(a, lo, hi, ychunk);
    if (Lp == 4 && nlev == 2) return run_stack<ndwt::Fwd2C<T, 4, 2, 2, EW>>(a, lo, hi, ychunk);
    if (Lp == 2 && nlev == 3) return run_stack<ndwt::Fwd2C<T, 2, 3, 2, EW>>(a, lo, hi, ychunk);
    return -1;
}
template <typename T, int EW> int inv_stack(int Lp, int nlev, ndwt::Fused2CIArgs<T>& a, const double* lo, const double* hi, int ychunk) {
    if (Lp == 8 && nlev == 3) return run_stack<ndwt::Inv2C<T, 8, 3, 1, 2, EW>>(a, lo, hi, ychunk);
    if (Lp == 4 && nlev == 2) return run_stack<ndwt::Inv2C<T, 4, 2, 1, 2, EW>>(a, lo, hi, ychunk);
    if (Lp == 2 && nlev == 3) return run_stack<ndwt::Inv2C<T, 2, 3, 1, 2, EW>>(a, lo, hi, ychunk);
    return -1;
}
template <typename T, int EW> int wx_of(int inverse, int Lp, int nlev) {
    if (Lp == 8 && nlev == 3) return inverse ? ndwt::Inv2C<T, 8, 3, 1, 2, EW>::WX : ndwt::Fwd2C<T, 8, 3, 2, EW>::WX;
    if (Lp == 4 && nlev == 2) return inverse ? ndwt::Inv2C<T, 4, 2, 1, 2, EW>::WX : ndwt::Fwd2C<T, 4, 2, 2, EW>::WX;
    if (Lp == 2 && nlev == 3) return inverse ? ndwt::Inv2C<T, 2, 3, 1, 2, EW>::WX : ndwt::Fwd2C<T, 2, 3, 2, EW>::WX;
    return -1;
}

}  // namespace

// one translation unit per kind and direction (EMU_STACK_PART 1 .. 8; 0: the entry points), so that the test builds them in parallel
#undef EMU_IN
#ifndef EMU_STACK_PART
#define EMU_IN(part) 1
#else
#define EMU_IN(part) (EMU_STACK_PART == part)
#endif

#define STACK_KIND(NAME, T, EW, PF, PI)                                                                                              \
    int emu_stack_fwd_##NAME(int Lp, int nlev, ndwt::Fused2CArgs<T>& a, const double* lo, const double* hi, int ychunk);              \
    int emu_stack_inv_##NAME(int Lp, int nlev, ndwt::Fused2CIArgs<T>& a, const double* lo, const double* hi, int ychunk);
STACK_KIND(f32, float, 1, 1, 2)
STACK_KIND(c64, float, 2, 3, 4)
STACK_KIND(f64, double, 1, 5, 6)
STACK_KIND(c128, double, 2, 7, 8)
#undef STACK_KIND
#if EMU_IN(1)
int emu_stack_fwd_f32(int Lp, int nlev, ndwt::Fused2CArgs<float>& a, const double* lo, const double* hi, int ychunk) { return fwd_stack<float, 1>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(2)
int emu_stack_inv_f32(int Lp, int nlev, ndwt::Fused2CIArgs<float>& a, const double* lo, const double* hi, int ychunk) { return inv_stack<float, 1>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(3)
int emu_stack_fwd_c64(int Lp, int nlev, ndwt::Fused2CArgs<float>& a, const double* lo, const double* hi, int ychunk) { return fwd_stack<float, 2>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(4)
int emu_stack_inv_c64(int Lp, int nlev, ndwt::Fused2CIArgs<float>& a, const double* lo, const double* hi, int ychunk) { return inv_stack<float, 2>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(5)
int emu_stack_fwd_f64(int Lp, int nlev, ndwt::Fused2CArgs<double>& a, const double* lo, const double* hi, int ychunk) { return fwd_stack<double, 1>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(6)
int emu_stack_inv_f64(int Lp, int nlev, ndwt::Fused2CIArgs<double>& a, const double* lo, const double* hi, int ychunk) { return inv_stack<double, 1>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(7)
int emu_stack_fwd_c128(int Lp, int nlev, ndwt::Fused2CArgs<double>& a, const double* lo, const double* hi, int ychunk) { return fwd_stack<double, 2>(Lp, nlev, a, lo, hi, ychunk); }
#endif
#if EMU_IN(8)
int emu_stack_inv_c128(int Lp, int nlev, ndwt::Fused2CIArgs<double>& a, const double* lo, const double* hi, int ychunk) { return inv_stack<double, 2>(Lp, nlev, a, lo, hi, ychunk); }
#endif

#if EMU_IN(0)
namespace {
template <typename T> int stack_kind(int inverse, int ew, int Lp, int nlev, const T* in, T* out, int n1, int n2, int nbatch, int ychunk, const double* lo,
                                     const double* hi) {
    if (nbatch < 0 || (ew != 1 && ew != 2)) return -1;
    // every band a whole array: its items back to back.  nbatch = 0: one image, the batch fields left as memset left them -- what every
    // caller that knows nothing of stacks passes
    const long long item = (long long)n1 * n2, band = item * (nbatch > 0 ? nbatch : 1), bstride = nbatch > 0 ? item : 0;
    if (!inverse) {
        ndwt::Fused2CArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        a.in = in; a.n1 = n1; a.n2 = n2; a.rs = n1; a.nbatch = nbatch; a.bstride = bstride;
        for (int b = 0; b < 1 + 3 * nlev; ++b) a.out[b] = out + b * band;
        if constexpr (sizeof(T) == 4) return ew == 2 ? emu_stack_fwd_c64(Lp, nlev, a, lo, hi, ychunk) : emu_stack_fwd_f32(Lp, nlev, a, lo, hi, ychunk);
        else return ew == 2 ? emu_stack_fwd_c128(Lp, nlev, a, lo, hi, ychunk) : emu_stack_fwd_f64(Lp, nlev, a, lo, hi, ychunk);
    } else {
        ndwt::Fused2CIArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        a.out = out; a.n1 = n1; a.n2 = n2; a.rs = n1; a.nbatch = nbatch; a.bstride = bstride;
        for (int b = 0; b < 1 + 3 * nlev; ++b) a.in[b] = in + b * band;
        if constexpr (sizeof(T) == 4) return ew == 2 ? emu_stack_inv_c64(Lp, nlev, a, lo, hi, ychunk) : emu_stack_inv_f32(Lp, nlev, a, lo, hi, ychunk);
        else return ew == 2 ? emu_stack_inv_c128(Lp, nlev, a, lo, hi, ychunk) : emu_stack_inv_f64(Lp, nlev, a, lo, hi, ychunk);
    }
}
}  // namespace

// in / out in kernel order: [nbatch][n2][n1 scalars] (complex: 2 scalars per element), on the coefficient side 1 + 3 nlev such arrays in
// the reference's band order.  ychunk: rows per wave, 0 = one chunk per item.
extern "C" int ndwt_emu2_stack(int inverse, int f64, int ew, int Lp, int nlev, const void* in, void* out, int n1, int n2, int nbatch, int ychunk,
                               const double* lo, const double* hi) {
    if (f64) return stack_kind<double>(inverse, ew, Lp, nlev, (const double*)in, (double*)out, n1, n2, nbatch, ychunk, lo, hi);
    return stack_kind<float>(inverse, ew, Lp, nlev, (const float*)in, (float*)out, n1, n2, nbatch, ychunk, lo, hi);
}
// scalars of a row one wave of the instance stores (the kernel's own WX), -1: not one of the instances here
extern "C" int ndwt_emu2_stack_wx(int inverse, int f64, int ew, int Lp, int nlev) {
    if (f64) return ew == 2 ? wx_of<double, 2>(inverse, Lp, nlev) : wx_of<double, 1>(inverse, Lp, nlev);
    return ew == 2 ? wx_of<float, 2>(inverse, Lp, nlev) : wx_of<float, 1>(inverse, Lp, nlev);
}
#endif
