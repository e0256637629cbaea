// Host emulation of the cascaded march of one strided axis (FwdMC / InvMC, csrc/ndwt_device_axis.h) -- TEST INFRASTRUCTURE.
// Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports one entry point for float and double;
// interleaved complex data is the factor 2 in `inner`.  tests/test_emulated_marchc.py builds it as a plain shared object; with
// ndwt_emu_marchc_main.cpp the same code is a program for AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_axis.h"
#include "ndwt_fused_list.h"

namespace {

template <class K, typename T> int run_marchc(const ndwt::MarchCArgs<T>& a, const double* lo, const double* hi) {
    typename K::Taps tp;
    for (int j = 0; j < K::L; ++j) { tp.lo[j] = (T)lo[j]; tp.hi[j] = (T)hi[j]; }
    const long long nblocks = (a.ngroups * a.outer + K::NT - 1) / K::NT * a.nchunks;     // the grid of launch_cascadem_k
    for (long long b = 0; b < nblocks; ++b) {
        typename K::Shared sh;
        EmuExec<typename K::State, K::NT> ex;
        K::block(ex, sh, a, tp, (int)b);
    }
    return 0;
}

template <typename T> int kind(int inverse, int L, int nlev, const ndwt::MarchCArgs<T>& a, const double* lo, const double* hi) {
#define CASEM(LL, NL)                                                                                 \
    if (L == LL && nlev == NL) return inverse ? run_marchc<ndwt::InvMC<T, LL, NL>, T>(a, lo, hi) : run_marchc<ndwt::FwdMC<T, LL, NL>, T>(a, lo, hi);
#define CASEML(LL) CASEM(LL, 2) CASEM(LL, 3) CASEM(LL, 4)
    CASEML(2) CASEML(4) CASEML(6) CASEML(8)
#undef CASEML
#undef CASEM
    return -1;
}

// in / out: bands of [outer][n][inner] scalars; the coefficient side holds 1 + nlev of them in the reference's order
template <typename T> int marchc_kind(int inverse, int L, int nlev, const T* in, T* out, long long inner, long long n, long long outer, int chunk,
                                      const double* lo, const double* hi) {
    if (!ndwt::cascadem_instantiated({inverse != 0, sizeof(T) == 8, L, nlev})) return -1;   // the library's own table
    if (inner < 4 || inner % 4 != 0 || n < 1 || outer < 1 || chunk < 0) return -1;
    const long long band = inner * n * outer;
    ndwt::MarchCArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.inner = inner; a.n = n; a.outer = outer; a.ngroups = inner / 4;
    a.chunk = (int)(chunk > 0 && chunk < n ? chunk : n);     // 0: one chunk per item
    a.nchunks = (int)((n + a.chunk - 1) / a.chunk);
    if (!inverse) {                                           // cascade level l (0 = finest) is transform level l + 1: band 1 + (nlev - (l + 1))
        a.in[0] = in;
        a.out[0] = out;
        for (int l = 0; l < nlev; ++l) a.out[1 + l] = out + (long long)(nlev - l) * band;
    } else {                                                  // cascade stage c (0 = coarsest) is transform level nlev - c: band 1 + c
        for (int b = 0; b < 1 + nlev; ++b) a.in[b] = in + (long long)b * band;
        a.out[0] = out;
    }
    return kind<T>(inverse, L, nlev, a, lo, hi);
}

}  // namespace

// lo / hi: the L taps of the direction in kernel form; chunk: planes of the axis per thread, 0 = the whole axis
extern "C" int ndwt_emu_marchc(int inverse, int f64, int L, int nlev, const void* in, void* out, long long inner, long long n, long long outer,
                               int chunk, const double* lo, const double* hi) {
    if (f64) return marchc_kind<double>(inverse, L, nlev, (const double*)in, (double*)out, inner, n, outer, chunk, lo, hi);
    return marchc_kind<float>(inverse, L, nlev, (const float*)in, (float*)out, inner, n, outer, chunk, lo, hi);
}
