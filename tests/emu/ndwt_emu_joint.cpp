// Host emulation of the joint-shrinkage kernels (JointShrink / GroupNorms, csrc/ndwt_device_joint.h; NormsFinish of
// csrc/ndwt_device_norms.h) -- TEST INFRASTRUCTURE.
// Takes EmuExec from ndwt_emu.cpp (an EMU_PART that selects none of its parts) and exports, for the four kinds (float real, complex64,
// double real, complex128):
//   ndwt_emu_joint_shrink  JointShrink on every (band, chunk) workgroup, in place; the thresholds converted to the scalar type as the
//                          library's upload converts them, in a heap block of exactly nb scalars
//   ndwt_emu_group_norms   GroupNorms on every (band, chunk) workgroup; with chunks > 1 the partials go to a heap block of exactly
//                          nb x chunks x 4 doubles and NormsFinish combines them, one workgroup per band
//   ndwt_emu_joint_kreg    kJointReg: the items JointShrink keeps in registers
// tests/test_emulated_joint.py builds it as a plain shared object; with ndwt_emu_joint_main.cpp the same code is a program for
// AddressSanitizer + UBSan.
#define EMU_PART 99
#include "ndwt_emu.cpp"
#include "ndwt_device_joint.h"

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

template <typename T, int COMP, bool VEC> void run_shrink(bool reg, T* y, long long pitch, long long n, long long items, int nb, int chunks, const double* thr,
                                                          int hard) {
    std::unique_ptr<T[]> table(new T[(size_t)nb]);                  // (exactly the table of the launch)
    for (int b = 0; b < nb; ++b) table[b] = (T)thr[b];
    const ndwt::JointShrinkArgs<T> a = {y, pitch, n, table.get(), items, nb, chunks, hard};
    if (reg) run_blocks<ndwt::JointShrink<T, COMP, VEC, true>>(a, (long long)nb * chunks);
    else run_blocks<ndwt::JointShrink<T, COMP, VEC, false>>(a, (long long)nb * chunks);
}

template <typename T, int COMP, bool VEC> void run_norms(const T* y, long long pitch, long long n, long long items, int nb, int chunks, double* out) {
    for (int i = 0; i < nb * 4; ++i) out[i] = -7.0;
    if (chunks == 1) {
        const ndwt::GroupNormsArgs<T> a = {y, pitch, n, out, items, nb, 1};
        run_blocks<ndwt::GroupNorms<T, COMP, VEC>>(a, nb);
        return;
    }
    const size_t npart = (size_t)nb * chunks * 4;
    std::unique_ptr<double[]> part(new double[npart]);             // (exactly the partials of the launch)
    for (size_t i = 0; i < npart; ++i) part[i] = -7.0;
    const ndwt::GroupNormsArgs<T> a = {y, pitch, n, part.get(), items, nb, chunks};
    run_blocks<ndwt::GroupNorms<T, COMP, VEC>>(a, (long long)nb * chunks);
    const ndwt::NormsFinishArgs f = {part.get(), out, 1, nb, 0, nb, chunks};
    run_blocks<ndwt::NormsFinish<>>(f, nb);
}

template <class F> void by_kind(int comp, bool vec, F&& f) {
    if (comp == 2) { if (vec) f(std::integral_constant<int, 2>(), std::true_type()); else f(std::integral_constant<int, 2>(), std::false_type()); }
    else { if (vec) f(std::integral_constant<int, 1>(), std::true_type()); else f(std::integral_constant<int, 1>(), std::false_type()); }
}

// the 4-scalar form for this placement, by the library's rule; -2: the arguments cannot run
int form_of(int f64, int comp, int vec, const void* y, long long pitch, long long n_scalars, long long items, int nb, int chunks) {
    if ((comp != 1 && comp != 2) || n_scalars < comp || n_scalars % comp != 0 || items < 1 || nb < 1 || chunks < 1 || pitch < items * n_scalars) return -2;
    const bool can_vec = ndwt::select_vec((unsigned long long)(uintptr_t)y, n_scalars, f64 ? 8 : 4) && pitch % 4 == 0;
    if (vec == 1 && !can_vec) return -2;
    return vec == -1 ? can_vec : vec == 1;
}

}  // namespace

extern "C" int ndwt_emu_joint_kreg() { return ndwt::kJointReg; }

// y: nb bands at `pitch` scalars, each items x n_scalars (complex: 2 per element); the last band ends with its last item.  vec: 1 the
// 4-scalar form (y, pitch and n_scalars multiples of 4 scalars, else -1), 0 one element at a time, -1 what the library's rule decides.
// reg: 1 the group in registers (items <= kJointReg, else -1), 0 two sweeps, -1 the library's rule.  thr: nb doubles.
// Returns (4-scalar form ran) + 2 * (registers form ran), or -1: not served.
extern "C" int ndwt_emu_joint_shrink(int f64, int comp, int vec, int reg, void* y, long long pitch, long long n_scalars, long long items, int nb, int chunks,
                                     const double* thr, int hard) {
    const int v = form_of(f64, comp, vec, y, pitch, n_scalars, items, nb, chunks);
    if (v < 0 || (reg == 1 && items > ndwt::kJointReg)) return -1;
    const bool r = reg == -1 ? items <= ndwt::kJointReg : reg == 1;
    if (f64) by_kind(comp, v != 0, [&](auto c, auto vv) { run_shrink<double, decltype(c)::value, decltype(vv)::value>(r, (double*)y, pitch, n_scalars, items, nb, chunks, thr, hard); });
    else by_kind(comp, v != 0, [&](auto c, auto vv) { run_shrink<float, decltype(c)::value, decltype(vv)::value>(r, (float*)y, pitch, n_scalars, items, nb, chunks, thr, hard); });
    return v + 2 * (int)r;
}

// out: [nb][4] doubles.  Returns 1 if the 4-scalar form ran, 0 for the element-wise one, -1: not served.
extern "C" int ndwt_emu_group_norms(int f64, int comp, int vec, const void* y, long long pitch, long long n_scalars, long long items, int nb, int chunks,
                                    double* out) {
    const int v = form_of(f64, comp, vec, y, pitch, n_scalars, items, nb, chunks);
    if (v < 0) return -1;
    if (f64) by_kind(comp, v != 0, [&](auto c, auto vv) { run_norms<double, decltype(c)::value, decltype(vv)::value>((const double*)y, pitch, n_scalars, items, nb, chunks, out); });
    else by_kind(comp, v != 0, [&](auto c, auto vv) { run_norms<float, decltype(c)::value, decltype(vv)::value>((const float*)y, pitch, n_scalars, items, nb, chunks, out); });
    return v;
}
