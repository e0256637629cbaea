// cascaded 2-D synthesis, double real data (Inv2C with scalar FMAs), tap lengths 2 .. 8
#include "ndwt_fused_kernels.h"
namespace ndwt {
template <class K> static int go(const typename K::Args& a, const void* taps_dev, hipStream_t s) {
    if (a.ntx != (a.n1 + K::WX - 1) / K::WX || a.ychunk < 1 || (long long)a.nyc * a.ychunk < a.n2) return -2;
    trace_kernel<K>(dim3(a.ntx * a.nyc), dim3(K::NT));
    hipLaunchKernelGGL(fused3_kernel<K>, dim3(a.ntx * a.nyc), dim3(K::NT), 0, s, a, (const typename K::Taps*)taps_dev);
    return (int)hipGetLastError();
}
#define NDWT_LAUNCH_R(T, EWV, LL, NLEV, PD, WPE)                                                       \
    if (k == Cascade2Instance{true, sizeof(T) == 8, EWV, LL, NLEV, PD}) {                             \
        static_assert(Inv2C<T, LL, NLEV, PD, WPE, EWV>::WX == cascade2_tile_width({true, sizeof(T) == 8, EWV, LL, NLEV, PD}), "tile width"); \
        return go<Inv2C<T, LL, NLEV, PD, WPE, EWV>>(a, taps_dev, s);                                  \
    }
int launch_cascade2_c128(const Cascade2Instance& k, const Fused2CIArgs<double>& a, const void* taps_dev, hipStream_t s);   // complex128
int launch_cascade2(const Cascade2Instance& k, const Fused2CIArgs<double>& a, const void* taps_dev, hipStream_t s) {
    if (k.ew != 1) return launch_cascade2_c128(k, a, taps_dev, s);
    NDWT_LIST_F64_INV2C(NDWT_LAUNCH_R)
    return -1;
}
}  // namespace ndwt
