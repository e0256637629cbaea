// ndwt_taps_host.h -- the tap tables of the fused kernels as the host builds them: the one place that writes the scalars of Taps3<T, L>,
// Taps3Y<T, L> and TapsDen<T, L> (ndwt_device.h, whose static_asserts tie the structs to the counts reserved here) in their order.
// Plain C++: the library uploads what these functions return, and the host emulation of the kernels (tests/emu) copies the same
// scalars into its K::Taps, so the CPU check runs every kernel on the table the library would upload.
#pragma once
#include <vector>

#include "ndwt_device.h"

namespace ndwt {

struct FusedTapsD {       // per axis (0 = x, 1 = y, 2 = z), zero-padded to Lp, double precision: what the plan's device tap tables are filled from
    int Lp;
    double lo[3][kMaxTaps];
    double hi[3][kMaxTaps];
};

// the pairs (t[k], t[k-1]), k = 0..L, taps outside [0, L) = 0: what a kernel whose x stage works on two adjacent samples reads
template <typename T> void append_tap_pairs(std::vector<T>& h, const double* t, int L) {
    for (int k = 0; k <= L; ++k)
        for (int d = 0; d < 2; ++d) h.push_back(k - d >= 0 && k - d < L ? (T)t[k - d] : T(0));
}

// Taps3<T, Lp>: lo[3][Lp], hi[3][Lp]; with xpairs the rest of Taps3Y<T, Lp> after them: xplo[Lp+1][2], xphi[Lp+1][2]
template <typename T> void append_taps3(std::vector<T>& h, const FusedTapsD& t, bool xpairs) {
    h.reserve(h.size() + (size_t)(xpairs ? taps3y_scalars(t.Lp) : taps3_scalars(t.Lp)));
    for (int ax = 0; ax < 3; ++ax)
        for (int j = 0; j < t.Lp; ++j) h.push_back((T)t.lo[ax][j]);
    for (int ax = 0; ax < 3; ++ax)
        for (int j = 0; j < t.Lp; ++j) h.push_back((T)t.hi[ax][j]);
    if (xpairs) {
        append_tap_pairs(h, t.lo[0], t.Lp);
        append_tap_pairs(h, t.hi[0], t.Lp);
    }
}

// TapsDen<T, Lp> from the synthesis and the analysis taps: syn (Taps3Y), alo[3][Lp], azp[Lp][2] = (alo_z[j], ahi_z[j]), axp[Lp+1][2].
// false: the analysis taps of x or y are not the mirrored pair ahi[j] = (-1)^j alo[Lp-1-j] the kernel derives its high-pass taps by
template <typename T> bool build_taps_den(std::vector<T>& h, const FusedTapsD& syn, const FusedTapsD& ana) {
    const int L = syn.Lp;
    h.clear();
    h.reserve((size_t)tapsden_scalars(L));
    append_taps3(h, syn, true);
    for (int ax = 0; ax < 3; ++ax)
        for (int j = 0; j < L; ++j) h.push_back((T)ana.lo[ax][j]);
    for (int j = 0; j < L; ++j) {
        h.push_back((T)ana.lo[2][j]);
        h.push_back((T)ana.hi[2][j]);
    }
    append_tap_pairs(h, ana.lo[0], L);
    for (int ax = 0; ax < 2; ++ax)
        for (int j = 0; j < L; ++j)
            if ((T)ana.hi[ax][j] != ((j % 2) ? T(-1) : T(1)) * (T)ana.lo[ax][L - 1 - j]) return false;
    return true;
}

}  // namespace ndwt
