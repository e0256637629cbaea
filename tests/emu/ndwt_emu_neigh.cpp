// Host emulation of the neighbourhood-shrinkage kernel (NeighShrink<T, COMP, ND, R>, csrc/ndwt_device_neigh.h) -- TEST INFRASTRUCTURE.
// Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports
//   ndwt_emu_neigh_shrink  every one of the 36 instances (float, complex64, double, complex128 x 1, 2, 3 filtered axes x radius 1, 2, 3)
//                          on every (band, item, chunk, tile) workgroup, from y into out; the squared thresholds formed as the library
//                          forms them, in a heap block of exactly nb doubles
//   ndwt_emu_neigh_tile    the tile of an instance
// tests/test_emulated_neigh.py builds it with ndwt_emu_neigh_main.cpp as a program for AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_neigh.h"

namespace {

template <class K> void run_blocks(const typename K::Args& a, long long nblocks) {
    const ndwt::SelectTaps tp = {0};
    for (long long b = 0; b < nblocks; ++b) {
        std::unique_ptr<typename K::Shared> sh(new typename K::Shared);
        std::memset(static_cast<void*>(sh.get()), 0xA5, sizeof(typename K::Shared));   // (LDS holds anything when a workgroup starts)
        EmuExec<typename K::State, K::NT> ex;
        K::block(ex, *sh, a, tp, (int)b);
    }
}

template <typename T, int COMP, int ND> int run_r(int r, const ndwt::NeighArgs<T>& a, long long blocks) {
    if (r == 1) run_blocks<ndwt::NeighShrink<T, COMP, ND, 1>>(a, blocks);
    else if (r == 2) run_blocks<ndwt::NeighShrink<T, COMP, ND, 2>>(a, blocks);
    else run_blocks<ndwt::NeighShrink<T, COMP, ND, 3>>(a, blocks);
    return 0;
}

template <typename T, int COMP> int run_nd(int nd, int r, const ndwt::NeighArgs<T>& a, long long blocks) {
    return nd == 1 ? run_r<T, COMP, 1>(r, a, blocks) : nd == 2 ? run_r<T, COMP, 2>(r, a, blocks) : run_r<T, COMP, 3>(r, a, blocks);
}

template <typename T> int run(int comp, int nd, int r, const T* y, T* out, long long pitch, const int* n, long long items, int nb, const int* geom,
                              const double* thr, int hard) {
    std::unique_ptr<double[]> tt(new double[(size_t)nb]);          // (exactly the table of the launch)
    for (int b = 0; b < nb; ++b) {
        const T t = (T)thr[b];
        tt[b] = thr[b] == 0.0 ? -1.0 : (double)t * (double)t;
    }
    const ndwt::NeighArgs<T> a = {y, out, pitch, (long long)n[0] * n[1] * n[2] * comp, tt.get(), items, n[0], n[1], n[2], 0, nb, geom[0], geom[1], geom[2], geom[3], hard};
    long long blocks = 0;
    if (!ndwt::neigh_launch_ok(a, comp, nd, r, &blocks)) return -1;
    return comp == 2 ? run_nd<T, 2>(nd, r, a, blocks) : run_nd<T, 1>(nd, r, a, blocks);
}

}  // namespace

// y, out: band 0 of two arrays of nb bands at `pitch` scalars, each items x n[0] x n[1] x n[2] elements (complex: 2 scalars each; n[k] = 1
// for an axis the instance does not have); the last band ends with its last item.  geom: ntx, nty, chunk, nchunks (neigh_geometry).
// thr: nb doubles.  Returns 0, or -1: arguments the launch refuses.
extern "C" int ndwt_emu_neigh_shrink(int f64, int comp, int nd, int r, const void* y, void* out, long long pitch, const int* n, long long items, int nb,
                                     const int* geom, const double* thr, int hard) {
    return f64 ? run<double>(comp, nd, r, (const double*)y, (double*)out, pitch, n, items, nb, geom, thr, hard)
               : run<float>(comp, nd, r, (const float*)y, (float*)out, pitch, n, items, nb, geom, thr, hard);
}

extern "C" void ndwt_emu_neigh_tile(int f64, int comp, int nd, int r, int* tx, int* ty) {
    *tx = ndwt::neigh_tx(nd);
    *ty = ndwt::neigh_ty(nd, (f64 ? 8 : 4) * comp, r);
}
