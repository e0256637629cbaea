// Host emulation of the tile form of the joint-shrinkage kernels (JointTile / GroupNormsTile, csrc/ndwt_device_joint_tile.h; NormsFinish
// of csrc/ndwt_device_norms.h) next to the chunk form they must agree with (JointShrink / GroupNorms, csrc/ndwt_device_joint.h) -- TEST
// INFRASTRUCTURE.
// Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports, for the four kinds (float real, complex64,
// double real, complex128):
//   ndwt_emu_jt_shrink  tile = 1: JointTile on every (band, strip) workgroup, the strips joint_tile_strips gives; tile = 0: JointShrink
//                       with one chunk per band, the group in registers by the library's rule.  In place; the thresholds converted to the
//                       scalar type as the library's upload converts them, in a heap block of exactly nb scalars
//   ndwt_emu_jt_norms   tile = 1: GroupNormsTile, and with more than one strip the partials in a heap block of exactly nb x strips x 4
//                       doubles, combined by NormsFinish, one workgroup per band; tile = 0: GroupNorms with one chunk per band
//   ndwt_emu_jt_sw / ndwt_emu_jt_j / ndwt_emu_jt_strips   the kernels' strip width and tile height, and the strips of a band
// tests/test_emulated_joint_tile.py builds it as a plain shared object; with ndwt_emu_joint_tile_main.cpp the same code is a program for
// AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_joint_tile.h"

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

template <typename T, int COMP, bool VEC> void run_shrink(bool tile, T* y, long long pitch, long long n, long long items, int nb, const double* thr, int hard) {
    std::unique_ptr<T[]> table(new T[(size_t)nb]);                  // (exactly the table of the launch)
    for (int b = 0; b < nb; ++b) table[b] = (T)thr[b];
    const int chunks = tile ? (int)ndwt::joint_tile_strips(n, COMP, VEC) : 1;
    const ndwt::JointShrinkArgs<T> a = {y, pitch, n, table.get(), items, nb, chunks, hard};
    if (tile) run_blocks<ndwt::JointTile<T, COMP, VEC>>(a, (long long)nb * chunks);
    else if (items <= ndwt::kJointReg) run_blocks<ndwt::JointShrink<T, COMP, VEC, true>>(a, nb);
    else run_blocks<ndwt::JointShrink<T, COMP, VEC, false>>(a, nb);
}

template <typename T, int COMP, bool VEC> void run_norms(bool tile, const T* y, long long pitch, long long n, long long items, int nb, double* out) {
    for (int i = 0; i < nb * 4; ++i) out[i] = -7.0;
    if (!tile) {
        const ndwt::GroupNormsArgs<T> a = {y, pitch, n, out, items, nb, 1};
        run_blocks<ndwt::GroupNorms<T, COMP, VEC>>(a, nb);
        return;
    }
    const int strips = (int)ndwt::joint_tile_strips(n, COMP, VEC);
    if (strips == 1) {
        const ndwt::GroupNormsArgs<T> a = {y, pitch, n, out, items, nb, 1};
        run_blocks<ndwt::GroupNormsTile<T, COMP, VEC>>(a, nb);
        return;
    }
    const size_t npart = (size_t)nb * strips * 4;
    std::unique_ptr<double[]> part(new double[npart]);             // (exactly the partials of the launch)
    for (size_t i = 0; i < npart; ++i) part[i] = -7.0;
    const ndwt::GroupNormsArgs<T> a = {y, pitch, n, part.get(), items, nb, strips};
    run_blocks<ndwt::GroupNormsTile<T, COMP, VEC>>(a, (long long)nb * strips);
    const ndwt::NormsFinishArgs f = {part.get(), out, 1, nb, 0, nb, strips};
    run_blocks<ndwt::NormsFinish<>>(f, nb);
}

template <class F> void by_kind(int comp, bool vec, F&& f) {
    if (comp == 2) { if (vec) f(std::integral_constant<int, 2>(), std::true_type()); else f(std::integral_constant<int, 2>(), std::false_type()); }
    else { if (vec) f(std::integral_constant<int, 1>(), std::true_type()); else f(std::integral_constant<int, 1>(), std::false_type()); }
}

// the 4-scalar form for this placement, by the library's rule; -2: the arguments cannot run
int form_of(int f64, int comp, int vec, const void* y, long long pitch, long long n_scalars, long long items, int nb) {
    if ((comp != 1 && comp != 2) || n_scalars < comp || n_scalars % comp != 0 || items < 1 || nb < 1 || pitch < items * n_scalars) return -2;
    const bool can_vec = ndwt::select_vec((unsigned long long)(uintptr_t)y, n_scalars, f64 ? 8 : 4) && pitch % 4 == 0;
    if (vec == 1 && !can_vec) return -2;
    return vec == -1 ? can_vec : vec == 1;
}

}  // namespace

extern "C" int ndwt_emu_jt_sw() { return ndwt::kJointTileSW; }
extern "C" int ndwt_emu_jt_j() { return ndwt::kJointTileJ; }
extern "C" long long ndwt_emu_jt_strips(long long n_scalars, int comp, int vec) { return ndwt::joint_tile_strips(n_scalars, comp, vec != 0); }

// y: nb bands at `pitch` scalars, each items x n_scalars (complex: 2 per element); the last band ends with its last item.  vec: 1 the
// 4-scalar form (y, pitch and n_scalars multiples of 4 scalars, else -1), 0 one element at a time, -1 what the library's rule decides.
// thr: nb doubles.  Returns 1 if the 4-scalar form ran, 0 for the element-wise one, -1: not served.
extern "C" int ndwt_emu_jt_shrink(int f64, int comp, int vec, int tile, void* y, long long pitch, long long n_scalars, long long items, int nb, const double* thr,
                                  int hard) {
    const int v = form_of(f64, comp, vec, y, pitch, n_scalars, items, nb);
    if (v < 0) return -1;
    if (f64) by_kind(comp, v != 0, [&](auto c, auto vv) { run_shrink<double, decltype(c)::value, decltype(vv)::value>(tile != 0, (double*)y, pitch, n_scalars, items, nb, thr, hard); });
    else by_kind(comp, v != 0, [&](auto c, auto vv) { run_shrink<float, decltype(c)::value, decltype(vv)::value>(tile != 0, (float*)y, pitch, n_scalars, items, nb, thr, hard); });
    return v;
}

// out: [nb][4] doubles.  Returns as ndwt_emu_jt_shrink.
extern "C" int ndwt_emu_jt_norms(int f64, int comp, int vec, int tile, const void* y, long long pitch, long long n_scalars, long long items, int nb, double* out) {
    const int v = form_of(f64, comp, vec, y, pitch, n_scalars, items, nb);
    if (v < 0) return -1;
    if (f64) by_kind(comp, v != 0, [&](auto c, auto vv) { run_norms<double, decltype(c)::value, decltype(vv)::value>(tile != 0, (const double*)y, pitch, n_scalars, items, nb, out); });
    else by_kind(comp, v != 0, [&](auto c, auto vv) { run_norms<float, decltype(c)::value, decltype(vv)::value>(tile != 0, (const float*)y, pitch, n_scalars, items, nb, out); });
    return v;
}
