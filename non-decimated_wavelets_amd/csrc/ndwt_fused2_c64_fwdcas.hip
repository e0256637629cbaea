// cascaded 2-D analysis, interleaved complex64 (Fwd2C with the x taps stepping over the (re, im) pairs), tap lengths 2 .. 8
#include "ndwt_fused_kernels.h"
namespace ndwt {
template <class K> static int go(const typename K::Args& a, const void* taps_dev, hipStream_t s) {
    if (a.ntx != (a.n1 + K::WX - 1) / K::WX || a.ychunk < 1 || (long long)a.nyc * a.ychunk < a.n2) return -2;
    trace_kernel<K>(dim3(a.ntx * a.nyc), dim3(K::NT));
    hipLaunchKernelGGL(fused3_kernel<K>, dim3(a.ntx * a.nyc), dim3(K::NT), 0, s, a, (const typename K::Taps*)taps_dev);
    return (int)hipGetLastError();
}
#define NDWT_LAUNCH_A(T, EWV, LL, NLEV, WPE)                                                           \
    if (k == Cascade2Instance{false, sizeof(T) == 8, EWV, LL, NLEV, 0}) {                             \
        static_assert(Fwd2C<T, LL, NLEV, WPE, EWV>::WX == cascade2_tile_width({false, sizeof(T) == 8, EWV, LL, NLEV, 0}), "tile width"); \
        return go<Fwd2C<T, LL, NLEV, WPE, EWV>>(a, taps_dev, s);                                      \
    }
int launch_cascade2_c64(const Cascade2Instance& k, const Fused2CArgs<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_C64_FWD2C(NDWT_LAUNCH_A)
    return -1;
}
}  // namespace ndwt
