// ndwt_fused_kernels.h -- __global__ wrappers + exact-match launches for the fused kernels (HIP only).
#pragma once
#include "ndwt_fused.h"
#include "ndwt_trace.h"

namespace ndwt {

template <class State> struct GpuExec {
    typedef State state_type;
    State st;
    template <class F> __device__ __forceinline__ void each(F&& f) { f((int)threadIdx.x, st); }   // (callers pass always-inline lambdas)
    __device__ __forceinline__ void barrier() { __syncthreads(); }
};

// amdgpu_waves_per_eu pins the register budget: without it hipcc aims at the LDS-limited occupancy and spills the
// filter windows to scratch (512-thread workgroups: 65 VGPRs + 176 B/lane of scratch).
// The taps live in a small device buffer owned by the plan and are read through the CONSTANT address space, so
// every tap is a scalar load into SGPRs (a by-value struct argument ends up partly in scratch once the stage
// functions nest a few lambdas deep).
template <class K>
__global__ __launch_bounds__(K::NT) __attribute__((amdgpu_waves_per_eu(K::WPE, K::WPE))) void fused3_kernel(
    const typename K::Args a, const typename K::Taps* __restrict__ taps_global) {
    __shared__ typename K::Shared sh;
    GpuExec<typename K::State> ex;
    typedef const __attribute__((address_space(4))) typename K::Taps* ctaps_ptr;
    const typename K::Taps& tp = *(const typename K::Taps*)(ctaps_ptr)taps_global;
    K::block(ex, sh, a, tp, (int)blockIdx.x);
}

// The march kernels (AxisMarch, AxisX: ndwt_march.hip; FwdMC / InvMC: ndwt_marchc_*.hip): arguments and taps by value, no LDS
template <class K>
__global__ __launch_bounds__(K::NT) void march_kernel(const typename K::Args a, const typename K::Taps tp) {
    typename K::Shared sh;
    GpuExec<typename K::State> ex;
    K::block(ex, sh, a, tp, (int)blockIdx.x);
}

// taps_dev: device buffer holding Taps3<T, Lp> (lo[3][Lp] then hi[3][Lp]) for this direction
template <class K> int launch_fused3(const typename K::Args& a, const void* taps_dev, hipStream_t s) {
    // the host computed the tiling for a tile shape (fused3_tile_shape); this kernel was compiled for one: they must be the same,
    // or workgroups would run off their tiles -- a status code here instead of a memory fault there
    if (a.ntx != (a.n1 + K::TX - 1) / K::TX || a.nty != (a.n2 + K::TY - 1) / K::TY || a.zchunk < 1 ||
        (long long)a.nzc * a.zchunk < a.n3 || (long long)(a.nzc - 1) * a.zchunk >= a.n3)
        return -2;
    const int nblocks = a.ntx * a.nty * a.nzc * a.nbatch;
    trace_kernel<K>(dim3(nblocks), dim3(K::NT));
    hipLaunchKernelGGL(fused3_kernel<K>, dim3(nblocks), dim3(K::NT), 0, s, a, (const typename K::Taps*)taps_dev);
    return (int)hipGetLastError();
}

// The 2-D kernels: one wave per tile of K::WX scalars and chunk of rows, times the batch items.  The same check of the host's tiling
// (fused2_geometry, cascade2_launch) against the tile this kernel was compiled for.
template <class K> int launch_wave_tiles(const typename K::Args& a, int nbatch, const void* taps_dev, hipStream_t s) {
    if (a.ntx != (a.n1 + K::WX - 1) / K::WX || a.ychunk < 1 || (long long)a.nyc * a.ychunk < a.n2) return -2;
    if (nbatch < 1 || (long long)a.ntx * a.nyc * nbatch > 0x7fffffffLL) return -2;   // (a stack: up to 2^20 - 1 items times the tiles of one)
    const int nblocks = a.ntx * a.nyc * nbatch;
    trace_kernel<K>(dim3(nblocks), dim3(K::NT));
    hipLaunchKernelGGL(fused3_kernel<K>, dim3(nblocks), dim3(K::NT), 0, s, a, (const typename K::Taps*)taps_dev);
    return (int)hipGetLastError();
}
template <class K> int launch_fused2(const typename K::Args& a, const void* taps_dev, hipStream_t s) {      // Fwd2S / Inv2S / Inv2P
    return launch_wave_tiles<K>(a, a.nbatch, taps_dev, s);
}
template <class K> int launch_cascade2_k(const typename K::Args& a, const void* taps_dev, hipStream_t s) {  // Fwd2C / Inv2C
    return launch_wave_tiles<K>(a, a.nbatch > 1 ? a.nbatch : 1, taps_dev, s);   // a stack: its items (a zeroed field: one image)
}

// The 1-D kernels of a batched plan (Fwd1C / Inv1C; Den1C, whose taps_dev holds Taps1D<T, L>, both directions): one wave per (signal,
// segment of K::WX scalars), four to the workgroup.  The host's segments (cascade1_tile_width, den1_tile_width) against the kernel's own,
// and a grid the launch can express, or -2: the caller takes one launch per level / the general route.
template <class K> int launch_wave_rows_k(const typename K::Args& a, const void* taps_dev, hipStream_t s) {
    if (a.row < 4 || a.row % 4 != 0 || a.row >= (1LL << 30) || a.outer < 1 || a.nseg != (a.row + K::WX - 1) / K::WX) return -2;
    const long long nblocks = (a.outer * a.nseg + K::NT / 64 - 1) / (K::NT / 64);
    if (nblocks > 0x7fffffffLL) return -2;
    trace_kernel<K>(dim3((unsigned)nblocks), dim3(K::NT));
    hipLaunchKernelGGL(fused3_kernel<K>, dim3((unsigned)nblocks), dim3(K::NT), 0, s, a, (const typename K::Taps*)taps_dev);
    return (int)hipGetLastError();
}

// One pass along the contiguous axis (AxisX): the same layout of waves, taps by value, rows of any length below 2^30 scalars.  The host's
// segments (axis_select: axisx_tile_width) against the kernel's own, and a grid the launch can express, or -2
template <class K> int launch_axisx_k(const typename K::Args& a, const double* lo, const double* hi, hipStream_t s) {
    typename K::Taps tp;
    typedef std::remove_reference_t<decltype(tp.lo[0])> T;
    for (int j = 0; j < K::L; ++j) { tp.lo[j] = (T)lo[j]; tp.hi[j] = (T)hi[j]; }
    if (a.row < 1 || a.row >= (1LL << 30) || a.outer < 1 || a.nseg != (a.row + K::WX - 1) / K::WX) return -2;
    const long long nblocks = (a.outer * a.nseg + K::NT / 64 - 1) / (K::NT / 64);
    if (nblocks > 0x7fffffffLL) return -2;
    trace_kernel<K>(dim3((unsigned)nblocks), dim3(K::NT));
    hipLaunchKernelGGL(march_kernel<K>, dim3((unsigned)nblocks), dim3(K::NT), 0, s, a, tp);
    return (int)hipGetLastError();
}

// The marches of one strided axis (AxisMarch: one level; FwdMC / InvMC: the cascade): 256 (item, group of 4 scalars) pairs per
// workgroup, times the chunks of the axis.  The host's chunks (march_chunks) must cover the axis exactly, or -2
template <class K> int launch_cascadem_k(const typename K::Args& a, const double* lo, const double* hi, hipStream_t s) {
    typename K::Taps tp;
    typedef std::remove_reference_t<decltype(tp.lo[0])> T;
    for (int j = 0; j < K::L; ++j) { tp.lo[j] = (T)lo[j]; tp.hi[j] = (T)hi[j]; }
    if (a.inner < 4 || a.inner % 4 != 0 || a.ngroups != a.inner / 4 || a.n < 1 || a.outer < 1 || a.chunk < 1 ||
        (long long)a.nchunks * a.chunk < a.n || (long long)(a.nchunks - 1) * a.chunk >= a.n)
        return -2;
    const long long nblocks = (a.ngroups * a.outer + K::NT - 1) / K::NT * a.nchunks;
    if (nblocks <= 0 || nblocks > 0x7fffffffLL) return -2;
    trace_kernel<K>(dim3((unsigned)nblocks), dim3(K::NT));
    hipLaunchKernelGGL(march_kernel<K>, dim3((unsigned)nblocks), dim3(K::NT), 0, s, a, tp);
    return (int)hipGetLastError();
}

// The order statistics of a band (BandHist / BandPick, ndwt_device_select.h): `nblocks` workgroups; buf_dev is the plan's select buffer,
// which stands in for the tap table these kernels do not have (a real device pointer: the wrapper forms a reference from it)
template <class K> int launch_select_k(const typename K::Args& a, int nblocks, const void* buf_dev, hipStream_t s) {
    if (nblocks < 1 || !buf_dev) return -2;
    trace_kernel<K>(dim3((unsigned)nblocks), dim3(K::NT));
    hipLaunchKernelGGL(fused3_kernel<K>, dim3((unsigned)nblocks), dim3(K::NT), 0, s, a, (const typename K::Taps*)buf_dev);
    return (int)hipGetLastError();
}

// One entry of an instance list (ndwt_fused_list.h) as an exact-match launch: the pick is this instance, or the next entry is asked.  A
// launch unit is its list expanded with these and a final "not mine" (-1).
#define NDWT_FUSED_K(KIND, INV, T, LL, V, VEC, ...)                                                          \
    KIND<T, LL, Fused3Tile<T, INV, V>::TX, Fused3Tile<T, INV, V>::TY, Fused3Tile<T, INV, V>::NT,             \
         Fused3Tile<T, INV, V>::RY, VEC, Fused3Tile<T, INV, V>::WPE, __VA_ARGS__>
#define NDWT_LAUNCH_F(T, LL, V, VEC, EWV, PIN, TPRE, WLDS)                                                   \
    if (k == fwd3_instance(sizeof(T) == 8, LL, V, VEC, EWV, PIN, TPRE, WLDS))                                \
        return launch_fused3<NDWT_FUSED_K(Fwd3, false, T, LL, V, VEC, EWV, false, TPRE, PIN, WLDS)>(a, taps_dev, s);
#define NDWT_LAUNCH_S(KIND, T, LL, V, VEC, EWV)                                                              \
    if (k == inv3s_instance(k##KIND, sizeof(T) == 8, LL, V, VEC, EWV)) return launch_fused3<NDWT_FUSED_K(KIND, true, T, LL, V, VEC, EWV)>(a, taps_dev, s);
#define NDWT_LAUNCH_Y(LL, VEC, EWV, DEPTH, UNI, XSC)                                                         \
    if (k == inv3y_instance(LL, VEC, EWV, DEPTH, UNI, XSC))                                                  \
        return launch_fused3<Inv3Y<float, LL, inv3y_tx(LL, EWV), inv3y_ty(LL, EWV), 1024, VEC, 4, DEPTH, EWV, inv3y_zlds(LL, DEPTH, EWV), 0, UNI, XSC>>(a, taps_dev, s);
// (the host lays a one-level 2-D launch out for fused2_tile_width, a cascade for cascade2_tile_width: they are the kernels' own WX)
#define NDWT_LAUNCH_W(KIND, T, LL, VEC, WPE, EWV)                                                            \
    if (k == Fused2SInstance{k##KIND == kInv2S, sizeof(T) == 8, VEC, LL, EWV, WPE}) {                        \
        static_assert(KIND<T, LL, VEC, WPE, EWV>::WX == fused2_tile_width(k##KIND == kInv2S, LL, EWV), "tile width"); \
        return launch_fused2<KIND<T, LL, VEC, WPE, EWV>>(a, taps_dev, s);                                    \
    }
#define NDWT_LAUNCH_P(T, LL, PD, PK) \
    if (k == Fused2PInstance{sizeof(T) == 8, LL, PD, PK}) return launch_fused2<Inv2P<T, LL, PD, 2, PK>>(a, taps_dev, s);
#define NDWT_LAUNCH_A(T, EWV, LL, NLEV, WPE)                                                                 \
    if (k == Cascade2Instance{false, sizeof(T) == 8, EWV, LL, NLEV, 0}) {                                    \
        static_assert(Fwd2C<T, LL, NLEV, WPE, EWV>::WX == cascade2_tile_width({false, sizeof(T) == 8, EWV, LL, NLEV, 0}), "tile width"); \
        return launch_cascade2_k<Fwd2C<T, LL, NLEV, WPE, EWV>>(a, taps_dev, s);                              \
    }
#define NDWT_LAUNCH_R(T, EWV, LL, NLEV, PD, WPE)                                                             \
    if (k == Cascade2Instance{true, sizeof(T) == 8, EWV, LL, NLEV, PD}) {                                    \
        static_assert(Inv2C<T, LL, NLEV, PD, WPE, EWV>::WX == cascade2_tile_width({true, sizeof(T) == 8, EWV, LL, NLEV, PD}), "tile width"); \
        return launch_cascade2_k<Inv2C<T, LL, NLEV, PD, WPE, EWV>>(a, taps_dev, s);                          \
    }
#define NDWT_LAUNCH_C(KIND, T, EWV, LL, NLEV)                                                                \
    if (k == Cascade1Instance{k##KIND == kInv1C, sizeof(T) == 8, EWV, LL, NLEV}) {                            \
        static_assert(KIND<T, LL, NLEV, EWV>::WX == cascade1_tile_width({k##KIND == kInv1C, sizeof(T) == 8, EWV, LL, NLEV}), "tile width"); \
        return launch_wave_rows_k<KIND<T, LL, NLEV, EWV>>(a, taps_dev, s);                                   \
    }
#define NDWT_LAUNCH_D(T, EWV, LL, NLEV)                                                                      \
    if (k == Den1Instance{sizeof(T) == 8, EWV, LL, NLEV}) {                                                  \
        static_assert(Den1C<T, LL, NLEV, EWV>::WX == den1_tile_width(LL, EWV, sizeof(T) == 8, NLEV), "tile width"); \
        return launch_wave_rows_k<Den1C<T, LL, NLEV, EWV>>(a, taps_dev, s);                                  \
    }
#define NDWT_LAUNCH_DR(T, EWV, LL, NLEV)                                                                 \
    if (k == Den1Instance{sizeof(T) == 8, EWV, LL, NLEV}) {                                                  \
        static_assert(Den1C<T, LL, NLEV, EWV, 4, true>::WX == den1_tile_width(LL, EWV, sizeof(T) == 8, NLEV), "tile width"); \
        return launch_wave_rows_k<Den1C<T, LL, NLEV, EWV, 4, true>>(a, taps_dev, s);                         \
    }
#define NDWT_LAUNCH_M(KIND, T, LL, NLEV) \
    if (k == CascadeMInstance{k##KIND == kInvMC, sizeof(T) == 8, LL, NLEV}) return launch_cascadem_k<KIND<T, LL, NLEV>>(a, lo, hi, s);
#define NDWT_LAUNCH_N(T, LL, SYN) \
    if (k == AxisMarchInstance{sizeof(T) == 8, SYN, LL}) return launch_cascadem_k<AxisMarch<T, LL, SYN>>(a, lo, hi, s);
#define NDWT_LAUNCH_X(T, LL, SYN, EWV, VEC)                                                                  \
    if (k == AxisXInstance{sizeof(T) == 8, SYN, VEC, LL, EWV}) {                                             \
        static_assert(AxisX<T, LL, SYN, EWV, VEC>::WX == axisx_tile_width({sizeof(T) == 8, SYN, VEC, LL, EWV}), "tile width"); \
        return launch_axisx_k<AxisX<T, LL, SYN, EWV, VEC>>(a, lo, hi, s);                                    \
    }

}  // namespace ndwt
