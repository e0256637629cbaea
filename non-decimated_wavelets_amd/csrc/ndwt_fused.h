// ndwt_fused.h -- host-callable launchers of the fused level kernels (their instances are spread over translation
// units so the build parallelises).  Every fused launch takes a pick that names its instance in full (ndwt_select.h, ndwt_fused_list.h)
// and asks the units in turn.  Returns 0 on success, -1 if no unit has the instance, -2 if the launch geometry is not the instance's
// tile, else a hipError_t.
#pragma once
#include <hip/hip_runtime.h>

#include "ndwt_device.h"
#include "ndwt_device_1d.h"
#include "ndwt_device_axis.h"
#include "ndwt_select.h"

namespace ndwt {

// The fused 3-D launch a pick names (ndwt_select.h: fused3_select).  The launch units are asked in turn; each runs the instance of its list
// (ndwt_fused_list.h) that the pick equals, or answers "not mine".  -1: no unit has the instance, -2: the launch geometry is not the
// instance's tile.
int launch_fused3_pick(const Fused3Pick& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s);
int launch_fused3_pick(const Fused3Pick& k, const Fused3Args<double>& a, const void* taps_dev, hipStream_t s);

// level 1 of a denoising step in one launch (Den3: in[0] = x, in[1] = approximation band) and the approximation-only analysis
// that goes with it (tall 64 x 32 tile); float, real data, tap lengths 2 .. 8: ndwt_fused3_f32_den.hip.  ndwt_denoise chooses these.
int launch_den3_f32(const Fused3Args<float>& a, int Lp, const void* taps_dev, hipStream_t s);
// (tile: the index into Fused3Tile the caller laid the launch out for -- 2 = 64 x 32, 0 = 64 x 16)
int launch_fwd3_low_f32(const Fused3Args<float>& a, int Lp, bool vec4, int tile, const void* taps_dev, hipStream_t s);

// The fused 2-D launch a pick names (fused2_select; register-only kernels, one wave per tile): the Fwd2S / Inv2S instance or the Inv2P
// instance of the pick, the launch units asked in turn as for 3-D.  -1: no unit has the instance, -2: the launch geometry is not the
// instance's tile (fused2_tile_width).
int launch_fused2_pick(const Fused2Pick& k, const Fused2Args<float>& a, const void* taps_dev, hipStream_t s);
int launch_fused2_pick(const Fused2Pick& k, const Fused2Args<double>& a, const void* taps_dev, hipStream_t s);
// Two or three levels of an image in one launch (Fwd2C / Inv2C), the instance named in full (ndwt_fused_list.h: Cascade2Instance, the
// table cascade2_levels reads; its tile: cascade2_tile_width).  Float real and interleaved complex64 take the float forms, double real and
// complex128 the double ones; -1: no unit has the instance, -2: the launch geometry is not the instance's tile.
int launch_cascade2(const Cascade2Instance& k, const Fused2CArgs<float>& a, const void* taps_dev, hipStream_t s);
int launch_cascade2(const Cascade2Instance& k, const Fused2CArgs<double>& a, const void* taps_dev, hipStream_t s);
int launch_cascade2(const Cascade2Instance& k, const Fused2CIArgs<float>& a, const void* taps_dev, hipStream_t s);
int launch_cascade2(const Cascade2Instance& k, const Fused2CIArgs<double>& a, const void* taps_dev, hipStream_t s);

// Two to four levels of the signals of a batched 1-D plan in one launch (Fwd1C / Inv1C), the instance named in full (ndwt_fused_list.h:
// Cascade1Instance, the table cascade1_levels reads; its tile: cascade1_tile_width).  -1: no unit has the instance, -2: the launch
// geometry is not the instance's tile, or the grid is too large.
int launch_cascade1(const Cascade1Instance& k, const Fused1CArgs<float>& a, const void* taps_dev, hipStream_t s);
int launch_cascade1(const Cascade1Instance& k, const Fused1CArgs<double>& a, const void* taps_dev, hipStream_t s);

// dec, per-band thresholding and rec of one to four levels of the signals of a batched 1-D plan in one launch (Den1C), the instance named
// in full (ndwt_fused_list.h: Den1Instance, the table denoise1_levels reads; its tile: den1_tile_width); taps_dev: Taps1D<T, L>.  -1: no
// unit has the instance, -2: the launch geometry is not the instance's tile, or the grid is too large.
int launch_den1(const Den1Instance& k, const Den1CArgs<float>& a, const void* taps_dev, hipStream_t s);
int launch_den1(const Den1Instance& k, const Den1CArgs<double>& a, const void* taps_dev, hipStream_t s);
// ... with a threshold row per signal, a.thr_rows (ndwt_denoise1r_*.hip: NDWT_LIST_*_DEN1R)
int launch_den1r(const Den1Instance& k, const Den1CArgs<float>& a, const void* taps_dev, hipStream_t s);
int launch_den1r(const Den1Instance& k, const Den1CArgs<double>& a, const void* taps_dev, hipStream_t s);

// Two to four levels of one strided axis inside one march (FwdMC / InvMC), the instance named in full (ndwt_fused_list.h:
// CascadeMInstance, the table cascadem_levels reads); lo / hi: the kernel-form taps of the direction, length k.L.  -1: no unit has the
// instance, -2: the grid is too large.
int launch_cascadem(const CascadeMInstance& k, const MarchCArgs<float>& a, const double* lo, const double* hi, hipStream_t s);
int launch_cascadem(const CascadeMInstance& k, const MarchCArgs<double>& a, const double* lo, const double* hi, hipStream_t s);

// One pass along one axis, the instance named in full (ndwt_fused_list.h: AxisMarchInstance / AxisXInstance, the tables axis_select
// reads): a strided axis with the window in registers, or the contiguous axis with lane shifts (its tile: axisx_tile_width).  lo / hi:
// the kernel-form taps of the direction, length k.L.  -1: not in the lists, -2: the chunks / segments are not the instance's, or the grid
// is too large -- after a pick, internal errors both.
int launch_axis_march(const AxisMarchInstance& k, const MarchArgs<float>& a, const double* lo, const double* hi, hipStream_t s);
int launch_axis_march(const AxisMarchInstance& k, const MarchArgs<double>& a, const double* lo, const double* hi, hipStream_t s);
int launch_axisx(const AxisXInstance& k, const AxisXArgs<float>& a, const double* lo, const double* hi, hipStream_t s);
int launch_axisx(const AxisXInstance& k, const AxisXArgs<double>& a, const double* lo, const double* hi, hipStream_t s);

}  // namespace ndwt
