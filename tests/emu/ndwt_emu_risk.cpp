// Host emulation of the SURE-statistics kernels (BandRisk / RiskFinish, csrc/ndwt_device_risk.h) -- TEST INFRASTRUCTURE.
// Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports one entry point for the four kinds: float
// real, complex64 (float, COMP = 2), double real, complex128.
//   ndwt_emu_band_risk   BandRisk on every (band, item, chunk) workgroup; with chunks > 1 the partials go to a heap block of exactly
//                        nb x items x chunks x nc x 3 doubles and RiskFinish combines them, one workgroup per (band, item).  The
//                        candidates go to a heap block of exactly items x nb x nc scalars, converted as the library converts them
// tests/test_emulated_risk.py builds it as a plain shared object; with ndwt_emu_risk_main.cpp the same code is a program for
// AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_risk.h"

namespace {

template <class K> void run_blocks(const typename K::Args& a, long long nblocks) {
    const ndwt::SelectTaps tp = {0};
    for (long long b = 0; b < nblocks; ++b) {
        std::unique_ptr<typename K::Shared> sh(new typename K::Shared);
        std::memset(sh.get(), 0xA5, sizeof(typename K::Shared));   // (LDS holds anything when a workgroup starts)
        EmuExec<typename K::State, K::NT> ex;
        K::block(ex, *sh, a, tp, (int)b);
    }
}

template <typename T, int COMP, bool VEC> void run_risk(const T* y, long long pitch, long long n, long long items, int nb, int chunks, int nc, const double* cand,
                                                        double* out) {
    const size_t nrow = (size_t)items * nb * nc, nres = nrow * 3, npart = nres * (size_t)chunks;
    std::unique_ptr<T[]> table(new T[nrow]);                       // (exactly the table of the launch)
    for (size_t i = 0; i < nrow; ++i) table[i] = (T)cand[i];
    for (size_t i = 0; i < nres; ++i) out[i] = -7.0;
    if (chunks == 1) {
        const ndwt::BandRiskArgs<T> a = {y, pitch, n, table.get(), out, items, nb, 0, nb, 1, nc};
        run_blocks<ndwt::BandRisk<T, COMP, VEC>>(a, (long long)nb * items);
        return;
    }
    std::unique_ptr<double[]> part(new double[npart]);             // (exactly the partials of the launch)
    for (size_t i = 0; i < npart; ++i) part[i] = -7.0;
    const ndwt::BandRiskArgs<T> a = {y, pitch, n, table.get(), part.get(), items, nb, 0, nb, chunks, nc};
    run_blocks<ndwt::BandRisk<T, COMP, VEC>>(a, (long long)nb * items * chunks);
    const ndwt::RiskFinishArgs f = {part.get(), out, items, nb, 0, nb, chunks, nc};
    run_blocks<ndwt::RiskFinish<>>(f, (long long)nb * items);
}

template <typename T> void risk_kind(int comp, bool vec, const T* y, long long pitch, long long n, long long items, int nb, int chunks, int nc, const double* cand,
                                     double* out) {
    if (comp == 2) { if (vec) run_risk<T, 2, true>(y, pitch, n, items, nb, chunks, nc, cand, out); else run_risk<T, 2, false>(y, pitch, n, items, nb, chunks, nc, cand, out); }
    else { if (vec) run_risk<T, 1, true>(y, pitch, n, items, nb, chunks, nc, cand, out); else run_risk<T, 1, false>(y, pitch, n, items, nb, chunks, nc, cand, out); }
}

}  // namespace

// y: nb bands at `pitch` scalars, each items x n_scalars (complex: 2 per element); the last band ends with its last item.  vec: 1 the
// 4-scalar form (y, pitch and n_scalars multiples of 4 scalars, else -1), 0 one element at a time, -1 what the library's rule decides.
// cand: [items][nb][nc] doubles, a row that begins with a negative entry skips its block.  out: [items][nb][nc][3] doubles.
// Returns 1 if the 4-scalar form ran, 0 for the element-wise one, -1: not served.
extern "C" int ndwt_emu_band_risk(int f64, int comp, int vec, const void* y, long long pitch, long long n_scalars, long long items, int nb, int chunks, int nc,
                                  const double* cand, double* out) {
    if ((comp != 1 && comp != 2) || n_scalars < comp || n_scalars % comp != 0 || items < 1 || nb < 1 || chunks < 1 || pitch < items * n_scalars) return -1;
    if (nc < 1 || nc > ndwt::kRiskMaxCand) return -1;
    const bool can_vec = ndwt::select_vec((unsigned long long)(uintptr_t)y, n_scalars, f64 ? 8 : 4) && pitch % 4 == 0;
    if (vec == 1 && !can_vec) return -1;
    const bool v = vec == -1 ? can_vec : vec == 1;
    if (f64) risk_kind<double>(comp, v, (const double*)y, pitch, n_scalars, items, nb, chunks, nc, cand, out);
    else risk_kind<float>(comp, v, (const float*)y, pitch, n_scalars, items, nb, chunks, nc, cand, out);
    return v ? 1 : 0;
}
