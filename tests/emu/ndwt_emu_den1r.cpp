// Host emulation of the one-launch denoise of a batched 1-D plan with a threshold row per signal (Den1C<.., ROWTHR = true>,
// csrc/ndwt_device_1d.h) beside its uniform twin -- TEST INFRASTRUCTURE.  Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none
// of its parts) and exports one entry point for the four instances of tests/test_emulated_den1r.py: float db4 at 4 levels, float db1 at
// 1, complex64 db2 at 3, double db3 at 2.  The table of a ROWTHR run is a heap block of exactly outer x 5 scalars, so a wave that indexes
// past its last row is a sanitizer report.  With ndwt_emu_den1r_main.cpp the same code is a program for AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_1d.h"

namespace {

template <class K, typename T> void run_den1(ndwt::Den1CArgs<T>& a, const double* taps) {
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
}

// thr: rowthr ? [outer][1 + NLEV] : [1 + NLEV], in the band order of the coefficient array (band 0 the approximation)
template <typename T, int L, int NLEV, int EW> int den1r(const void* in, void* out, long long row, long long outer, const double* taps, const double* thr,
                                                       int hard, int rowthr) {
    if (row < 4 || row % 4 != 0 || outer < 1) return -1;
    ndwt::Den1CArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.row = row; a.outer = outer;
    a.in[0] = (const T*)in;
    a.out[0] = (T*)out;
    a.hard = hard;
    const auto order = [&](const double* t, T* dst) {         // cascade level l (0 = finest) is transform level l + 1: band NLEV - l
        dst[0] = (T)t[0];
        for (int l = 0; l < NLEV; ++l) dst[1 + l] = (T)t[NLEV - l];
        for (int l = NLEV; l < 4; ++l) dst[1 + l] = T(0);
    };
    if (!rowthr) {
        order(thr, a.thr);
        run_den1<ndwt::Den1C<T, L, NLEV, EW>, T>(a, taps);
        return 0;
    }
    std::unique_ptr<T[]> rows(new T[(size_t)outer * 5]);        // exactly outer x 5 scalars
    for (long long j = 0; j < outer; ++j) order(thr + j * (1 + NLEV), rows.get() + 5 * j);
    a.thr_rows = rows.get();
    for (int i = 0; i < 5; ++i) a.thr[i] = T(1e30);             // (a ROWTHR kernel that read a.thr would zero everything)
    run_den1<ndwt::Den1C<T, L, NLEV, EW, 4, true>, T>(a, taps);
    return (int)((outer * a.nseg) % 4);                         // waves of the last workgroup past the last item: 4 - this, if not 0
}

}  // namespace

// which: 0 float db4 (8 taps) 4 levels, 1 float db1 1 level, 2 complex64 db2 3 levels, 3 double db3 2 levels.  in / out: `outer` rows of
// `row` scalars, two buffers that do not overlap; taps: [4][20] analysis lo / hi, synthesis lo / hi in kernel form.  Returns < 0: refused;
// else (rowthr) the (row, segment) items in the last workgroup modulo 4.
extern "C" int ndwt_emu1r_denoise(int which, const void* in, void* out, long long row, long long outer, const double* taps, const double* thr, int hard,
                                  int rowthr) {
    switch (which) {
        case 0: return den1r<float, 8, 4, 1>(in, out, row, outer, taps, thr, hard, rowthr);
        case 1: return den1r<float, 2, 1, 1>(in, out, row, outer, taps, thr, hard, rowthr);
        case 2: return den1r<float, 4, 3, 2>(in, out, row, outer, taps, thr, hard, rowthr);
        case 3: return den1r<double, 6, 2, 1>(in, out, row, outer, taps, thr, hard, rowthr);
    }
    return -1;
}
