/*
 * ndwt.h -- C ABI of the MI355X-native non-decimated wavelet transform engine (libndwt_hip.so).
 *
 * This is the drop-in boundary for the reference's native hot path:
 *   reference mex/nddwt.h:13-32   nd_dwt_dec / nd_dwt_rec / nd_dwt_{dec,rec}_1level / pointByPoint /
 *                                 init_fftw_plan      (the FFT-domain core, complex fp64 only)
 *   reference mex/nd_dwt_mex.c:8  mexFunction         (the MATLAB gateway the classes call:
 *                                 nd_dwt_1D.m:158,220  nd_dwt_2D.m:160,222  nd_dwt_3D.m:161,225
 *                                 nd_dwt_4D.m:158,219)
 *
 * The reference hands FFT-domain data (x_f, f_dec) across that boundary; this engine takes the
 * SIGNAL-domain array and a plan that carries the per-axis Daubechies taps, and computes the same
 * coefficients with direct periodic filter banks in hand-written HIP kernels (gfx950).  Plain C types
 * only: pointers, sizes, int status codes.  No torch, no C++ types.
 *
 * Layout (identical to the reference, nd_dwt_mex.c:72-83): column-major, dims[0] fastest; coefficient
 * arrays are band-planar with the band axis last, bands = 2^d + (2^d-1)(level-1); band 0 is the coarsest
 * approximation, the last 2^d-1 bands are the level-1 details; inside a level band b uses the high-pass
 * on axis a iff bit a of b is set (Functions/nd_dwt_3D.m:45-52,334-341).
 *
 * Threading: a plan may be used by one host thread at a time; different plans are independent.
 * Every compute entry point is asynchronous on the given HIP stream unless it takes host pointers.
 */
#ifndef NDWT_H
#define NDWT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDWT_MAX_DIMS 4
#define NDWT_MAX_TAPS 20 /* db10 */

typedef struct ndwt_plan ndwt_plan; /* opaque */

/* status codes (the reference core returns void and cannot fail cleanly; nd_dwt_mex.c raises
 * "MATLAB:FFT2mx:invalidNumInputs" for every error -- the mex shim maps these codes onto that) */
enum {
    NDWT_OK = 0,
    NDWT_ERR_INVALID_ARG = 1,  /* bad ndim / dims / level / null pointer */
    NDWT_ERR_UNKNOWN_WAVELET = 2, /* wave_filters.m:159 "Unknown Wavelet Name" */
    NDWT_ERR_FILTER_TOO_LONG = 3, /* nd_dwt_3D.m:277-286 "... Dimension of Data is shorter than the wavelet filter being used" */
    NDWT_ERR_NO_DEVICE = 4,    /* no HIP device / HIP runtime failure at plan creation */
    NDWT_ERR_HIP = 5,          /* a HIP call failed; see ndwt_last_error() */
    NDWT_ERR_ALLOC = 6,
    NDWT_ERR_UNSUPPORTED = 7
};

enum { NDWT_F32 = 0, NDWT_F64 = 1 };                 /* 'precision' = single / double (nd_dwt_3D.m:130-132) */
enum { NDWT_REAL = 0, NDWT_COMPLEX_INTERLEAVED = 1 }; /* split complex: call twice (re, im) -- the filters are real */
enum { NDWT_DILATION_REFERENCE = 0, /* same un-dilated taps at every level: what the reference computes (nd_dwt_3D.m:178-186, nddwt.c:214-234) */
       NDWT_DILATION_ATROUS = 1 };   /* tap stride 2^(level-1): textbook stationary wavelet transform.  An axis only has to hold the
                                        un-dilated filter: axes shorter than a level's dilated filter are served, the filter periodised
                                        (it wraps round the axis, taps that land on one sample add up) */
enum { NDWT_PATH_AUTO = 0,    /* fused kernels where they apply, per-axis kernels otherwise */
       NDWT_PATH_GENERIC = 1  /* force the per-axis kernels (used by the parity tests to cross-check the fused ones) */ };

/* ---- filters: Functions/wave_filters.m:1-174 ------------------------------------------------------
 * wname = "db1" .. "db10" (case-insensitive).  Writes LO_D and HI_D (length *len = 2K) exactly as the
 * reference returns them: LO_D[m] = h[L-1-m], HI_D[m] = (-1)^(m+1) h[m].  Buffers hold NDWT_MAX_TAPS. */
int ndwt_wave_filters(const char* wname, double* lo_d, double* hi_d, int* len);

/* ---- band bookkeeping -------------------------------------------------------------------------------
 * nd_dwt_mex.c:83 and the level inference of rec() (nd_dwt_1D.m:213, 2D:215, 3D:217, 4D:213). */
int64_t ndwt_num_bands(int ndim, int level);
int ndwt_level_from_bands(int ndim, int64_t bands); /* returns level >= 1, or -1 if `bands` is not a valid count */

/* ---- plan: replaces the class constructor's get_filters() (nd_dwt_3D.m:263-342) and the per-call
 *      FFTW planning of nddwt.c:110-111 ----------------------------------------------------------------
 * ndim 1..4; dims[0] fastest; wnames[a] per axis; dtype NDWT_F32/F64; complexity NDWT_REAL or
 * NDWT_COMPLEX_INTERLEAVED; pres_l2_norm as in the classes; dilation NDWT_DILATION_*; max_level = the
 * largest level dec/rec will be asked for (sizes the scratch); device = HIP device ordinal. */
int ndwt_plan_create(ndwt_plan** plan, int ndim, const int64_t* dims, const char* const* wnames, int dtype,
                     int complexity, int pres_l2_norm, int dilation, int max_level, int device);
/* Batched plan: `howmany` >= 1 signals of dims[0] elements transformed by one call (anything else: NDWT_ERR_INVALID_ARG).  ndim must be 1 in
 * this version; 2 .. 4 is NDWT_ERR_UNSUPPORTED.  Both are checked before any device call.
 * Layout: signal k at x + k * n elements; every band is a contiguous [howmany][n] block, band b at b * bs with bs = howmany * n (packed)
 * or the caller's band_pitch >= howmany * n (ndwt_band_pitch: howmany * n plus the usual skew) -- [n, howmany, bands] in MATLAB terms.
 * Band order and normalisation are those of a 1-D plan.
 * At the reference's dilation two to four levels run in ONE launch wherever the rows allow it (n * comp a multiple of 4 and >= 8 taps'
 * worth, 2 .. 8 taps, 16- / 32-byte aligned pointers): the approximations between them stay in registers, and the result equals one
 * launch per level bit for bit.  ndwt_plan_set_variant(plan, 9, 9, ...) switches that off per direction.  Everything else (a-trous
 * levels, longer filters, odd n) runs the per-axis kernels over all signals at once.
 * Served: ndwt_dec, ndwt_rec, ndwt_dec_pitched, ndwt_rec_pitched, ndwt_shrink, ndwt_shrink_pitched, ndwt_denoise (dec, the shrink pass,
 * rec), ndwt_dec_split / ndwt_rec_split, ndwt_plan_set_*, ndwt_plan_describe, profiling and the trace.
 * Refused with NDWT_ERR_UNSUPPORTED (they size a buffer by one array's dimensions): the host-pointer forms ndwt_dec_host, ndwt_rec_host,
 * ndwt_denoise_host, ndwt_dec_split_host, ndwt_rec_split_host; every ndwt_coef_* that takes a plan; the slab entry points
 * ndwt_analysis_level_slab*, ndwt_synthesis_level_slab*; ndwt_slab_segments and ndwt_slab_segments_strided. */
int ndwt_plan_create_many(ndwt_plan** plan, int ndim, const int64_t* dims, int64_t howmany, const char* const* wnames,
                          int dtype, int complexity, int pres_l2_norm, int dilation, int max_level, int device);
/* Plan that filters SOME axes of an array: dims[0 .. ndim) is the whole array (ndim 1 .. 4), bit a of `axes` set = axis a is filtered --
 * swtn(..., axes=...) of other wavelet packages.  Served in this version: the k lowest bits, 1 <= k <= ndim (the leading axes).
 * axes == 0, a bit at or above ndim, ndim outside 1 .. 4: NDWT_ERR_INVALID_ARG; any other mask (0x5, 0x2, ...): NDWT_ERR_UNSUPPORTED, the
 * message names the mask.  All of it is checked before any device call.
 * k == ndim is exactly ndwt_plan_create.  k < ndim is a STACK: the K = prod(dims[k .. ndim)) items of prod(dims[0 .. k)) elements lie back
 * to back and each gets the periodic k-D transform on its own (k == 1: the batched plan of ndwt_plan_create_many with howmany = K).
 * wnames has ndim entries; those of the axes left alone are ignored and may be NULL.  The reference's length check (filter <= axis, the
 * same messages) applies to the filtered axes only; an axis left alone needs length >= 1.
 * Layout: ndwt_num_bands(k, level) bands, each a whole array [dims]; band b at b * bs with bs = prod(dims) (packed) or the caller's
 * band_pitch (ndwt_band_pitch: prod(dims) plus the usual skew); item j of a band at j * prod(dims[0 .. k)) -- [n1, n2, K, bands] in MATLAB
 * terms.  Band order and normalisation are those of a k-D plan.
 * Kernels: a level at tap stride 1 is ONE fused 2-D / 3-D launch with the items in its batch slot; a-trous levels and whatever the fused
 * kernels refuse run the per-axis kernels over all items at once.  Two or three levels of a stack of images can run in one launch
 * (Fwd2C / Inv2C with the item taken from the block id) under the per-item conditions of a single image: unasked from the
 * item height and total size at which that was measured to win (float: items of 128 rows (dec) / 256 rows (rec) in 64 MiB; the other
 * kinds 512 rows in 128 MiB: DESIGN.md 4.3b), else on request (ndwt_plan_set_variant(plan, 11, 11, ...)); 9 / 9 switches it off.  ndwt_plan_describe: "stack2d cascade",
 * "stack2d fused", "stack3d fused" or "stack axis".
 * Served and refused entry points: the lists of ndwt_plan_create_many, with the same message. */
int ndwt_plan_create_axes(ndwt_plan** plan, int ndim, const int64_t* dims, unsigned axes, const char* const* wnames, int dtype,
                          int complexity, int pres_l2_norm, int dilation, int max_level, int device);
/* Plan over INTERLEAVED SAMPLES: each sample is `inner` >= 1 elements that lie together (fastest in memory), the filtered axes come next,
 * `howmany` >= 1 items last -- the array is [inner, dims.., howmany] in MATLAB terms.  ndim 1 .. 4; dims / wnames describe ONE item.  A
 * dynamic series [nx, ny, nt] filtered in time only is inner = nx * ny, dims = {nt}; channels-first images [C, n1, n2] are inner = C.
 * inner < 1, howmany < 1, ndim outside 1 .. 4: NDWT_ERR_INVALID_ARG, the message names the argument; checked before any device call.
 * Layout: element (c, i, j) at c + inner * (i + prod(dims) * j); item j of the input and of every band at j * inner * prod(dims); band b
 * at b * bs with bs = inner * prod(dims) * howmany (packed) or the caller's band_pitch (ndwt_band_pitch: the same plus the usual skew).
 * Interleaved complex stays innermost (2 scalars per element).  Band order, normalisation and the length checks (on dims only, the
 * reference's messages) are those of an ndim-D plan.  inner == 1 is the plan ndwt_plan_create_axes makes for [dims.., howmany] with its
 * leading axes filtered: the same routes, the same bits.
 * Kernels: every filtered axis is strided, so a level runs one per-axis pass per axis (the register-window march where comp * inner is a
 * multiple of 4 and the pointers are 16- / 32-byte aligned, the element-wise kernels otherwise: RGB, inner = 3) -- every data kind, both
 * dilations, every tap length.  With ndim == 1, the reference's dilation, 2 .. 8 taps and comp * inner a multiple of 4, two to four
 * levels can run inside ONE march (FwdMC / InvMC: the approximations between levels stay in registers, level + 2 volumes of traffic
 * instead of 3 level), equal to one launch per level bit for bit: on request (ndwt_plan_set_variant(plan, 11, 11, ...)), and unasked only
 * where it was measured to win; 9 / 9 switches it off per direction.  ndwt_plan_describe: "interleaved cascade" or
 * "interleaved axis".  ndwt_denoise runs dec, the shrink pass, rec.
 * Served and refused entry points: the lists of ndwt_plan_create_many, with the same message. */
int ndwt_plan_create_interleaved(ndwt_plan** plan, int ndim, const int64_t* dims, int64_t inner, int64_t howmany,
                                 const char* const* wnames, int dtype, int complexity, int pres_l2_norm, int dilation, int max_level,
                                 int device);
/* Plan for ONE SLAB of a volume sharded on its outermost axis (the *_slab entry points below): dims describe the local slab,
 * global_outer is the length of the sharded axis of the whole volume.  The reference's length check (nd_dwt_3D.m:277-286:
 * filter <= axis) applies to the WHOLE axis: a slab may be thinner than the filter (cfg5: 32 frames over 8 ranks = 4, db4 = 8
 * taps) -- the slab kernels read halo planes and never wrap.  ndwt_dec / ndwt_rec (periodic on every axis) refuse such a plan
 * when the local length is shorter than the filter. */
int ndwt_plan_create_slab(ndwt_plan** plan, int ndim, const int64_t* dims_local, int64_t global_outer, const char* const* wnames,
                          int dtype, int complexity, int pres_l2_norm, int dilation, int max_level, int device);
/* Plan for ONE SLAB of a volume sharded on axis `shard_axis` (counted from the fastest axis, 0 = x): ndim - 1 is the outermost axis
 * (exactly ndwt_plan_create_slab, global_len = global_outer), 2 with ndim == 4 shards a (3-D + time) volume on z and keeps t whole on
 * every rank; anything else is NDWT_ERR_UNSUPPORTED.  dims_local[shard_axis] = the local planes, global_len = the length of the sharded
 * axis of the whole volume: the reference's filter-length check (nd_dwt_3D.m:277-286, "Third Dimension of Data is shorter ...")
 * applies to it, the local slab may be thinner than the filter.
 * Layouts of a z-slab (a "plane" = one (ny, nx) plane of one frame; memory order t, z, y, x as always):
 *   input with halo of ndwt_analysis_level_slab         (nt, ab + n + aa, ny, nx)
 *   halo buffers of ndwt_analysis_level_slab_split      (nt, ab, ny, nx) and (nt, aa, ny, nx)
 *   every band of ndwt_synthesis_level_slab             (nt, sb + n + sa, ny, nx)
 *   output of ndwt_synthesis_level_slab_ext             (nt, sa + n + sb, ny, nx)
 * with ab, aa, sb, sa = ndwt_slab_halo (from the z filter).  A level is nd_dwt_4D.m's dec / rec: the periodic t pass over the z-extended
 * frames, then the fused 3-D kernel with the halo on z batched over the frames (reverse order in the synthesis); plans the fused kernels do
 * not take (fp64 long filters, dilated levels, a z filter shorter than another axis' ...) run the per-axis passes with the halo on z.
 * The split form assembles the slab and its two halo buffers in a plan-owned scratch (one ndwt_slab_segments_strided launch) first.
 * ndwt_synthesis_level_slab_ext needs the fused kernels with the z filter the longest, at tap stride 1; the run-of-planes forms
 * (_part, _runs) return NDWT_ERR_UNSUPPORTED for z-slabs. */
int ndwt_plan_create_slab_axis(ndwt_plan** plan, int ndim, const int64_t* dims_local, int shard_axis, int64_t global_len,
                               const char* const* wnames, int dtype, int complexity, int pres_l2_norm, int dilation, int max_level, int device);
/* A plan owns scratch (the approximation ping-pong between levels, temporaries): use it from ONE host thread and ONE stream
 * at a time.  Calls on different streams must be ordered by the caller (an event), or use one plan per stream. */
int ndwt_plan_destroy(ndwt_plan* plan);
int ndwt_plan_set_path(ndwt_plan* plan, int path); /* NDWT_PATH_* */
/* which kernels a level of this plan runs: writes a short static string such as "fused3d", "fused2d",
 * "axis" into buf (for tests and logs) */
int ndwt_plan_describe(const ndwt_plan* plan, char* buf, int buflen);
/* tuning hook (tests, benchmarks): workgroup count the fused kernels aim for and/or a forced number of
 * outer-axis planes per workgroup; 0 restores the default.  Results never depend on it. */
int ndwt_plan_set_tuning(ndwt_plan* plan, int target_blocks, int force_zchunk);
/* test / tuning hook of tools/ (interleaved A/B runs): kernel variant per direction, marched chunk per direction, fp64 on the
 * fused (1) or per-axis (0) kernels.  Negative = leave unchanged.  Every variant computes the same transform (bit-identical where
 * only the schedule differs; to rounding where the order of the FMAs does: packed / scalar forms, kernel families); the library never
 * reads the environment.  The numbers (named in csrc/ndwt_select.h: FwdVariant / InvVariant, with the full table):
 *   variant_fwd  0 default | 1 one column per thread, 512 threads | 2 tall 64x32 tile (and denoise's band-0 analysis on it) | 3 keeps the
 *                small tile / the spilling long-filter forms | 6 tall tile, y items of 2 rows | 7 4-D: t axis folded in | 8 no pinned taps |
 *                2-D: 9 no cascade (either direction) | 10 cascade always, kernel mode 1 | 11 cascade always
 *   variant_inv  0 default | 3-D: 2 dilated levels keep Inv3S | 3 LDS kernel Inv3 (8 taps) | 4 Inv3S | 5 Inv3Y depth 1 | 9 no shared y / z
 *                taps | 10 scatter x stage wherever it exists | 11 gather x stage everywhere | 2-D: 1 keeps Inv2S | 2 / 4 Inv2P depth 2 / 4
 *                on Inv2S's geometry | 6 depth 2, 1024 waves | 7 unpacked FMAs | cascade: 9 off | 11 always | 12 always, two rows in flight
 *   The 2-D cascade (two or three levels of an image in one launch) serves float and double images, real or interleaved complex, whose
 *   rows are whole groups of 4 scalars, up to 8 taps (float real analysis: also 12): by default beyond a size per data kind, on request
 *   (10 / 11 / 12) at any size; "two rows in flight" where that instance exists (float real, complex64), one row otherwise. */
int ndwt_plan_set_variant(ndwt_plan* plan, int variant_fwd, int variant_inv, int zchunk_fwd, int zchunk_inv, int fp64_fused);
/* test / tuning hook: 0 makes ndwt_denoise keep the level-1 detail bands in memory (dec, thresholding fused into the synthesis
 * loads, rec); 1 (default) = level 1 in one launch that recomputes them where that is faster (float, real, 3-D, one tap length
 * <= 6 on every axis); 2 = also with 8 taps (compute-bound there: 3 % slower than the materialising path at 512^3). */
int ndwt_plan_set_fused_level1(ndwt_plan* plan, int enable);
/* per-kernel timing with HIP events recorded on the launch stream around every kernel this plan launches
 * (what bench.py's roofline line is computed from).  ndwt_plan_get_profile() synchronises the device, sums and
 * clears the records of one kernel kind. */
enum { NDWT_KERNEL_FUSED_ANALYSIS = 0, NDWT_KERNEL_FUSED_SYNTHESIS = 1, NDWT_KERNEL_AXIS_ANALYSIS = 2, NDWT_KERNEL_AXIS_SYNTHESIS = 3 };
int ndwt_plan_set_profiling(ndwt_plan* plan, int enable);
int ndwt_plan_get_profile(ndwt_plan* plan, int kind, double* total_ms, int64_t* launches);

/* ---- the transform: replaces nd_dwt_dec / nd_dwt_rec (nddwt.c:189-292) and the 1-level forms
 *      (nddwt.c:98-186) -----------------------------------------------------------------------------------
 * x: prod(dims) elements (x2 scalars if complex); y: prod(dims)*ndwt_num_bands(ndim, level) elements.
 * Device pointers, caller-allocated, inputs are never modified (the reference's rec overwrites its
 * input, nddwt.c:163).  stream is a hipStream_t passed as void* (NULL = the null stream). */
int ndwt_dec(ndwt_plan* plan, const void* x_dev, void* y_dev, int level, void* stream);
int ndwt_rec(ndwt_plan* plan, const void* y_dev, void* x_dev, int level, void* stream);
/* The same with a PITCHED coefficient array: band b starts at y_dev + b * band_pitch elements (band_pitch >= prod(dims);
 * 0 = packed, i.e. ndwt_dec / ndwt_rec).  The packed layout is the reference's (a MATLAB array [dims, bands]); callers that
 * own the coefficient buffer (iterative solvers, the Python classes with 'band_pitch', ndwt_denoise's scratch) gain 4 - 12 %
 * on the synthesis of power-of-two volumes by keeping the 2^d band streams a few hundred bytes off a power-of-two distance:
 * with every band at the same address modulo 1 KiB the fabric traffic of the 512^3 synthesis is 1.23x its algorithmic bytes
 * (1.44x before the library skewed the one band it owns, the approximation scratch), with band_pitch = ndwt_band_pitch(plan)
 * (prod(dims) + 256 bytes) 1.08x.  Results are identical. */
int ndwt_dec_pitched(ndwt_plan* plan, const void* x_dev, void* y_dev, int64_t band_pitch, int level, void* stream);
int ndwt_rec_pitched(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, void* x_dev, int level, void* stream);
int64_t ndwt_band_pitch(const ndwt_plan* plan);   /* the recommended pitch in elements */

/* Host-pointer forms for the mex shim (stage through device memory, synchronous). */
int ndwt_dec_host(ndwt_plan* plan, const void* x_host, void* y_host, int level);
int ndwt_rec_host(ndwt_plan* plan, const void* y_host, void* x_host, int level);

/* Staging of the host-pointer forms is owned by the plan, grown on demand and kept across calls (a 512^3 3-level transform stages
 * 12.3 GB: allocating and freeing it per call costs milliseconds, and the gateway is called thousands of times by an iterative
 * solver, README.md:2).  ndwt_plan_release_staging gives the memory back (the next host-pointer call allocates again). */
int ndwt_plan_release_staging(ndwt_plan* plan);

/* ---- device-resident coefficients ------------------------------------------------------------------------
 * The reference's gateway moves the whole coefficient array through host memory on every call (y = nd_dwt_mex(...) at
 * nd_dwt_3D.m:161, x = nd_dwt_mex(y, ...) at :225): 11.8 GB per direction for a 512^3 3-level transform, 0.2 s over PCIe against
 * 3 ms of compute.  A solver that only needs rec(shrink(dec(x))) -- or that keeps y between iterations -- can leave the coefficients
 * on the device behind an opaque handle: only the signal crosses the link.  The handle is bound to the plan that made it (same
 * dims / wavelets / precision); it owns a pitched coefficient array (ndwt_band_pitch) and must be released before its plan is
 * destroyed (ndwt_plan_destroy refuses while handles of the plan are alive).  All calls are synchronous on the null stream, like the other host-pointer forms. */
typedef struct ndwt_coef ndwt_coef;
int ndwt_coef_create(ndwt_plan* plan, int level, ndwt_coef** coef);                       /* uninitialised coefficients of `level` levels */
int ndwt_coef_release(ndwt_coef* coef);
int ndwt_coef_info(const ndwt_coef* coef, int* level, int64_t* bands, int64_t* band_pitch, void** dev_ptr);
/* dec: x_host -> coefficients on the device.  *coef == NULL: a new handle is returned; else that handle (same plan and level) is refilled */
int ndwt_coef_dec_host(ndwt_plan* plan, const void* x_host, int level, ndwt_coef** coef);
int ndwt_coef_rec_host(ndwt_plan* plan, const ndwt_coef* coef, void* x_host);             /* rec: coefficients on the device -> x_host */
int ndwt_coef_shrink(ndwt_plan* plan, ndwt_coef* coef, double threshold, int mode);       /* NDWT_SHRINK_* of the detail bands, in place */
/* the whole array in the reference's packed layout [dims, bands] to / from host memory (for callers that do need y) */
int ndwt_coef_get_host(ndwt_plan* plan, const ndwt_coef* coef, void* y_host);
int ndwt_coef_put_host(ndwt_plan* plan, int level, const void* y_host, ndwt_coef** coef);

/* ---- consumers for iterative solvers (extension; the reference's users threshold the bands in MATLAB, README.md:2) ----
 * ndwt_shrink: in-place soft / hard thresholding of every detail band of a level-`level` coefficient array (band 0, the
 *   coarsest approximation, is kept); complex data: the magnitude is shrunk, the phase kept.
 * ndwt_denoise: dec -> shrink -> rec in one call; the coefficients live in a scratch array owned by the plan, so only
 *   the signal crosses the boundary (x and out may be the same buffer).  The host form moves 2 x prod(dims) elements
 *   over PCIe instead of 2 x prod(dims) x bands.  Float, real, 3-D plans with one tap length <= 6 on every axis and
 *   16-byte aligned, non-overlapping x / out run the FINEST LEVEL WITHOUT ITS DETAIL BANDS IN MEMORY: one launch recomputes
 *   them from x, thresholds them in registers and reconstructs (5 volumes moved at level 1 instead of 18); the values are
 *   those of dec -> shrink -> rec up to fp32 rounding (the recomputed coefficients are not rounded through memory).
 *   x == out keeps the materialising path. */
enum { NDWT_SHRINK_SOFT = 0, NDWT_SHRINK_HARD = 1 };
int ndwt_shrink(ndwt_plan* plan, void* y_dev, int level, double threshold, int mode, void* stream);
int ndwt_shrink_pitched(ndwt_plan* plan, void* y_dev, int64_t band_pitch, int level, double threshold, int mode, void* stream);
int ndwt_denoise(ndwt_plan* plan, const void* x_dev, void* out_dev, int level, double threshold, int mode, void* stream);
int ndwt_denoise_host(ndwt_plan* plan, const void* x_host, void* out_host, int level, double threshold, int mode);
/* ---- one threshold per band ----
 * A non-decimated transform does not keep white noise white across its bands: unit-variance noise arrives in band b with the standard
 * deviation gains[b] (db4, 4 levels, pres_l2_norm: 0.620, 0.143, 0.178, 0.252, 0.707 for bands 0 .. 4), so one number for every band is
 * wrong by construction and a caller sets thresholds[b] = k * sigma * gains[b].
 * ndwt_band_gains: host only -- no device, no plan.  gains[b], b in [0, ndwt_num_bands(ndim, level)), is the l2 norm of band b of the
 *   periodic dec of a unit impulse on an array of `dims` (the filtered axes of ONE item: stacks, batches and interleaved plans pass
 *   those), computed in double from the periodised convolution of the levels' taps at their tap strides (either dilation), so it is
 *   exact where an axis is shorter than the equivalent filter and the filter wraps.  level 1 .. 30; the argument checks are those of
 *   ndwt_plan_create, with its codes and messages.
 * thresholds: a HOST array of ndwt_num_bands(k, level) doubles (k = filtered axes), read before the call returns.  Entry b shrinks band
 *   b with the arithmetic of ndwt_shrink (soft or hard; complex data: the magnitude); band 0 is a band like any other.  A threshold of
 *   exactly 0 leaves its band untouched (nothing is launched for it).  A null array, a negative or NaN entry: NDWT_ERR_INVALID_ARG, the
 *   message names the band.
 * ndwt_shrink_bands: every plan kind ndwt_shrink_pitched serves (band_pitch 0 = packed); one pass of the shrink kernel per band.
 * ndwt_denoise_bands: every plan kind ndwt_denoise serves: dec into the plan's pitched scratch, ndwt_shrink_bands, rec.  A batched 1-D
 *   plan (ndwt_plan_create_many) at the reference's dilation, 2 .. 8 taps, 1 .. 4 levels, rows as for its cascades, can run the whole
 *   call in ONE launch (Den1C: analysis, thresholding and synthesis in registers -- one read of the signals and one write instead of
 *   4 level + 4 volumes; measured 1.3x to 5.5x faster than ndwt_denoise): unasked for float, complex64 and double data,
 *   on request for complex128 (ndwt_plan_set_variant(plan, 11, 11, ...)); 9 in either slot switches it off.  x and out must then be
 *   16- / 32-byte aligned and must not overlap, else the call takes the general route, silently.  The values are those of the general route up to
 *   rounding (the coefficients are not rounded through memory).  ndwt_denoise and ndwt_shrink are unchanged. */
int ndwt_band_gains(int ndim, const int64_t* dims, const char* const* wnames, int pres_l2_norm, int dilation, int level, double* gains);
int ndwt_shrink_bands(ndwt_plan* plan, void* y_dev, int64_t band_pitch, int level, const double* thresholds, int mode, void* stream);
int ndwt_denoise_bands(ndwt_plan* plan, const void* x_dev, void* out_dev, int level, const double* thresholds, int mode, void* stream);
/* ---- the sigma of thresholds[b] = k * sigma * gains[b]: exact order statistics of a band's |c|, on the device ----
 * ndwt_band_select: values[i] = the k[i]-th smallest (0-based) |c| of band `band` of a level-`level` coefficient array on the device
 *   (band_pitch 0 = packed), for nk = 1 .. 4 ranks in one call; a rank may be given twice.  Real data: |c| exactly (the value's own
 *   bits, widened to double).  Interleaved complex data: the magnitude sqrt(re^2 + im^2) in the plan's scalar type, as the shrink
 *   computes and compares it.  A NaN orders after every number, -0 and +0 are equal.  A band is the plan's WHOLE array: all signals of
 *   a batch and all items of a stack pooled (as ndwt_shrink_bands sees it); per item: ndwt_band_select_items, below.  Every plan kind
 *   ndwt_shrink_bands serves.  The band is read 3 times (float, complex64) or 6 times (double, complex128), whatever nk -- a radix
 *   select on the bit pattern, no sort, no copy -- and never written; the plan keeps 32 KB of device scratch for it.  Bands of 2^32
 *   elements or more: NDWT_ERR_UNSUPPORTED.
 *   k and values are HOST pointers, so the call is synchronous like the other forms with host pointers: it enqueues on `stream`, copies
 *   the nk results back, synchronises the stream and returns.  plan, y_dev, k or values null, band outside [0, ndwt_num_bands), nk
 *   outside 1 .. 4, a k[i] outside [0, elements of the band): NDWT_ERR_INVALID_ARG, the message names the argument.
 * ndwt_estimate_sigma_coef: the standard deviation of white noise in the SIGNAL, estimated from a level-`level` coefficient array
 *   (Donoho and Johnstone): m = the median of |c| over the LAST band -- level 1, high-pass on every filtered axis -- (an even count:
 *   the mean of the two middle order statistics), g = that band's gain (what ndwt_band_gains returns for the plan's filtered axes,
 *   pres_l2_norm and dilation), and
 *     real data     sigma = m / 0.6744897501960817 / g   (the median of |N(0, 1)|)
 *     complex data  sigma = m / 1.1774100225154747 / g   (|c| is Rayleigh distributed; sqrt(2 ln 2) is its median for unit parts):
 *                   the standard deviation of EACH of the real and imaginary parts, not of the complex sample (that is sqrt(2) larger).
 *   *sigma is a HOST pointer: synchronous, as above.
 * ndwt_estimate_sigma: the same from a signal on the device: one level-1 dec into the plan's coefficient scratch (as ndwt_denoise_bands
 *   runs it), then the coefficient path.  x is not modified. */
int ndwt_band_select(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, int64_t band, int nk, const int64_t* k,
                     double* values, void* stream);
int ndwt_estimate_sigma_coef(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* sigma, void* stream);
int ndwt_estimate_sigma(ndwt_plan* plan, const void* x_dev, double* sigma, void* stream);
/* ---- the same per ITEM: channels, coils, traces and slices do not share one noise level ----
 * An item is one signal of ndwt_plan_create_many, one image or volume of a stack (ndwt_plan_create_axes), one of the `howmany` blocks of
 * ndwt_plan_create_interleaved: its part of a band is one contiguous run of scalars, item j behind item j - 1.  `items` below is their
 * number; an unbatched plan is one item, and every call here then equals its band-wide form.
 * ndwt_band_select_items: values[j * nk + i] = the k[i]-th smallest |c| of item j's part of band `band`; key, NaN ordering, -0 / +0 and
 *   the complex magnitude exactly as ndwt_band_select, k[i] in [0, elements of ONE item).  Synchronous like it, never writes the band,
 *   every plan kind ndwt_shrink_bands serves; the refusals are those of ndwt_band_select and name the argument; items of 2^32 elements
 *   or more (or 2^31 items): NDWT_ERR_UNSUPPORTED.  With at least as many items as the device has compute units, of up to 2^22 scalars
 *   each, the whole call is ONE launch (ItemSelect: one workgroup runs the radix select of one item with its histogram in LDS; 4096 float
 *   signals of 4096 samples: 0.25 ms), and so it is where that was measured to win: from 8 items on for items of up to
 *   2^14 scalars, from 64 on up to 2^18.  Otherwise the band-wide passes run once per item on that item's part, with one copy back at the end.
 *   ndwt_plan_set_variant(plan, *, 11, ...) forces the one launch, 9 the loop; real values are the same bit for bit.  The plan keeps
 *   64 bytes of device scratch per item on top of ndwt_band_select's.
 * ndwt_estimate_sigma_coef_items / ndwt_estimate_sigma_items: sigma[j] = the formula of ndwt_estimate_sigma_coef on item j (the same
 *   gain, the same constants, an even count takes the mean of the two middle order statistics).  sigma: HOST, `items` doubles.
 * thresholds (ndwt_shrink_bands_items / ndwt_denoise_bands_items): a HOST table, thresholds[j * nb + b] for item j and band b, nb =
 *   ndwt_num_bands(filtered axes, level), the bands in the order of the coefficient array; read before the call returns.  An entry of 0
 *   leaves that item's part of that band alone; an all-zero table launches no shrink.  A null table, a negative or NaN entry:
 *   NDWT_ERR_INVALID_ARG, the message names the item and the band.  The arithmetic is that of ndwt_shrink_bands; every (band, item)
 *   block is shrunk in ONE launch (ShrinkItems), with the values ndwt_shrink_bands gives on a plan of that one item.  The table reaches
 *   the device through a pinned host buffer and a device buffer that the plan owns and only grows (nothing is allocated per call after
 *   the first); the copy is enqueued on `stream`, and a later call waits for it before it overwrites the pinned buffer, so calls back to
 *   back on one stream each use their own table.  That wait blocks the HOST (hipEventSynchronize) until the previous call's copy has
 *   run, so a call is at most one call ahead of the device, and the two calls cannot be captured into a graph.  (Calls of one plan on
 *   different streams are not ordered with each other, as for every call that uses the plan's scratch.)
 * ndwt_shrink_bands_items: every plan kind ndwt_shrink_bands serves.  ndwt_denoise_bands_items: every plan kind ndwt_denoise_bands
 *   serves -- dec into the plan's pitched scratch, the one shrink launch, rec.  A batched 1-D plan runs the whole call in ONE launch
 *   under exactly the conditions of ndwt_denoise_bands (Den1C with a threshold row per signal, read from a device table of 5 scalars per
 *   signal: unasked for float, complex64 and double, ndwt_plan_set_variant(plan, 11, 11, ...) for complex128, 9 in either slot off; x and
 *   out 16- / 32-byte aligned and not overlapping, else the route above, silently); signal j's values are those of ndwt_denoise_bands
 *   with row j, bit for bit.
 * Not built: a device-pointer form of the table; thresholds per item inside the fused synthesis kernels' loads.  The band-wide calls,
 *   the host-pointer forms, the handles, the slab entry points and the MATLAB gateway are unchanged. */
int ndwt_band_select_items(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, int64_t band, int nk, const int64_t* k,
                           double* values, void* stream);
int ndwt_estimate_sigma_coef_items(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* sigma, void* stream);
int ndwt_estimate_sigma_items(ndwt_plan* plan, const void* x_dev, double* sigma, void* stream);
int ndwt_shrink_bands_items(ndwt_plan* plan, void* y_dev, int64_t band_pitch, int level, const double* thresholds, int mode, void* stream);
int ndwt_denoise_bands_items(ndwt_plan* plan, const void* x_dev, void* out_dev, int level, const double* thresholds, int mode, void* stream);
/* ---- sums of a band: what an iterative solver evaluates every iteration (its objective, its stopping rule) and what a data-driven
 * threshold needs next to sigma -- the l1 norm, the energy, the largest magnitude and the count of non-zeros, in ONE read of the array ----
 * For every (band, item) block of a level-`level` coefficient array on the device (band_pitch 0 = packed), four doubles in this order:
 *   NDWT_NORM_L1    real data: the sum of |c|.  Interleaved complex data: the sum of the magnitude sqrt(re^2 + im^2) computed in the plan's
 *                   scalar type, exactly as the shrink compares it and ndwt_band_select orders it, then widened
 *   NDWT_NORM_L2SQ  the sum of c^2; complex data: of re^2 + im^2, from the widened parts
 *   NDWT_NORM_MAX   the largest |c|; complex data: the largest of that magnitude (bit for bit ndwt_band_select's last order statistic)
 *   NDWT_NORM_NNZ   the count of elements with c != 0; complex data: with re != 0 or im != 0
 *   All four are accumulated in double whatever the data kind, the squares with a fused multiply-add, the count in a 64-bit integer that
 *   is converted to double at the end.  A NaN in a block makes that block's l1, l2sq and max NaN and counts as non-zero; -0 is zero.
 *   There are no floating-point atomics and no hand-off between workgroups inside a launch: the order of every sum is a fixed function
 *   of the shape and the launch geometry (the device's compute units, ndwt_plan_set_tuning's target_blocks), so two calls on one device
 *   return the same bits.
 * nb = ndwt_num_bands(filtered axes, level); band 0 is a band like any other.
 * ndwt_band_norms: a band is the plan's WHOLE array, all signals of a batch and all items of a stack pooled, as ndwt_shrink_bands and
 *   ndwt_band_select see it.  norms: HOST, [nb][4] doubles.
 * ndwt_band_norms_items: the items of ndwt_band_select_items, above; norms: HOST, [items][nb][4] doubles, norms[(j * nb + b) * 4 + s].
 *   An unbatched plan is one item, and the call then equals ndwt_band_norms.
 *   Both are synchronous like the other forms with host pointers: they enqueue on `stream`, copy the results back once, synchronise the
 *   stream once and return.
 * ndwt_band_norms_dev: the same values (per_item != 0: the layout of ndwt_band_norms_items, else of ndwt_band_norms) into DEVICE memory
 *   at norms_dev, 8-byte aligned.  It only enqueues -- no copy, no synchronisation; the results are there in stream order: the form a
 *   solver uses to keep its objective on the device.
 * Every plan kind ndwt_shrink_bands serves.  All blocks are read in ONE launch (BandNorms, workgroups of 256 threads, each block split
 *   into chunks while every thread keeps 8 turns of its loop and the grid stays within 16 workgroups per compute unit); where a block has
 *   more than one chunk a second, small launch (NormsFinish) adds the chunks' partial results in a fixed order.  The partials, and the
 *   results of the host forms, live in a device buffer the plan owns and only grows: nothing is allocated per call after the first.  The
 *   coefficient array is never written.  plan, y_dev, norms or norms_dev null, a level outside the plan's, a band pitch smaller than a
 *   band, norms_dev not 8-byte aligned: NDWT_ERR_INVALID_ARG, the message names the argument, and nothing is launched; 2^31 items or
 *   more: NDWT_ERR_UNSUPPORTED.  (Calls of one plan on different streams are not ordered with each other, as for every call that uses
 *   the plan's scratch.)
 * Not built: a statistic fused into the shrink or the synthesis loads; weighted norms on the device.  The existing calls, the
 *   host-pointer forms, the handles, the slab entry points and the MATLAB gateway are unchanged. */
enum { NDWT_NORM_L1 = 0, NDWT_NORM_L2SQ = 1, NDWT_NORM_MAX = 2, NDWT_NORM_NNZ = 3, NDWT_NORM_COUNT = 4 };
int ndwt_band_norms(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* norms, void* stream);
int ndwt_band_norms_items(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* norms, void* stream);
int ndwt_band_norms_dev(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, int per_item, double* norms_dev, void* stream);
/* ---- SURE thresholds (SureShrink): what Stein's unbiased estimate of the risk of a soft threshold needs of a band, at up to
 * NDWT_RISK_MAX_CAND candidate thresholds in ONE read of the array; the estimate; and the search for the threshold that minimises it ----
 * ndwt_band_risk, ndwt_band_risk_items: for every (band, item) block of a level-`level` coefficient array on the device (band_pitch 0 =
 *   packed) and every candidate i < nc of that block, three doubles in this order.  t = the candidate rounded once to the plan's scalar
 *   type, as the shrink rounds its threshold; m = the magnitude of an element: |c|, of interleaved complex data sqrt(re^2 + im^2) computed
 *   in the plan's scalar type -- the bits the shrink compares, ndwt_band_select orders and NDWT_NORM_MAX returns.
 *   NDWT_RISK_COUNT   the count of elements with !(m > t): those a shrink at t sets to zero.  A NaN counts.  An integer, written as a double
 *   NDWT_RISK_ENERGY  the sum of c^2 (complex: re^2 + im^2) over those elements, accumulated in double from the widened parts with a fused
 *                     multiply-add, as NDWT_NORM_L2SQ is.  A NaN in the block makes it NaN for every candidate
 *   NDWT_RISK_INVSUM  complex data: the sum of 1.0 / (double)m over the elements with m > t.  Real data: 0, nothing is computed for it
 *   nc: 1 .. NDWT_RISK_MAX_CAND.  nb = ndwt_num_bands(filtered axes, level).
 *   cand: HOST, [nb][nc] doubles (ndwt_band_risk: a band is the plan's whole array, as ndwt_band_norms sees it) or [items][nb][nc]
 *   (ndwt_band_risk_items: the items of ndwt_band_norms_items), cand[((j * nb + b) * nc + i)].  A candidate is >= 0; +inf is allowed (it
 *   counts every element).  A row whose FIRST entry is negative skips its block: no workgroup reads that block and its nc * 3 results are
 *   0 -- how the approximation band is left out.  A NaN, or a negative entry elsewhere in a row: NDWT_ERR_INVALID_ARG, the message names
 *   the band, (the item,) and the position, and nothing is launched.
 *   risk: HOST, [nb][nc][3] or [items][nb][nc][3] doubles, risk[((j * nb + b) * nc + i) * 3 + s].
 *   Blocks, items, pooling, band_pitch, the grid (one launch, BandRisk, over all blocks; a second small one, RiskFinish, where a block
 *   has more than one chunk), the plan-owned buffer and the fixed order of every sum -- no floating-point atomics, two calls on one device
 *   return the same bits -- are those of ndwt_band_norms, and so are the plan kinds served and the refusals (plan, y_dev, cand or risk
 *   null, level, pitch: NDWT_ERR_INVALID_ARG; 2^31 items: NDWT_ERR_UNSUPPORTED).  The candidates go to the device as the threshold table
 *   of ndwt_shrink_bands_items does, with its host wait for the previous table's copy.  Synchronous like ndwt_band_norms: enqueue on
 *   `stream`, one copy back, one synchronisation.  The coefficient array is never written.
 * ndwt_sure_from_risk: HOST only, no device and no plan.  With d = comp (1 real, 2 complex), n the elements of the block, s the standard
 *   deviation of the noise in each real part of a coefficient of the band (sigma * the band's gain, ndwt_band_gains) and t = cand[i],
 *   C, E, I = the three statistics risk[3 * i ..] of candidate i:
 *     sure[i] = n d s^2 + E + t^2 (n - C) - 2 s^2 (d C + (d - 1) t I)
 *   Stein's unbiased estimate of the risk of soft thresholding at t; for d = 2 of the magnitude shrink the library performs.  (Where
 *   nothing lies above t -- t = +inf -- the terms in n - C and I are 0.)  comp not 1 or 2, n or s negative, NaN or infinite, nc < 1, a
 *   null pointer: NDWT_ERR_INVALID_ARG.
 * ndwt_sure_thresholds, ndwt_sure_thresholds_items: the soft threshold of every block that minimises that estimate, searched on the
 *   device's statistics.  sigma: the noise level of the data (the items form: HOST, [items]), finite and >= 0; thresholds: HOST, [nb] or
 *   [items][nb] -- a row ndwt_shrink_bands(_items) and ndwt_denoise_bands(_items) take as it is; sure: HOST, the estimate at the
 *   threshold returned, same shape, or null.  rounds: 1 .. 8; 0 means 3.
 *   Band 0 gets the threshold 0 (and the estimate 0) and is never read.  For every other block, with s = sigma * the plan's own gain of
 *   the band, N the elements of ONE item's filtered axes and n the elements of the block (n = N but for a pooled batch or interleaved
 *   samples): t_max = s sqrt(2 ln N), the universal threshold; the search starts from lo = 0, hi = t_max and best = (t = 0, n d s^2: the
 *   estimate at 0).  Every round forms the 8 candidates lo + (hi - lo) (i + 1) / 8 in double, rounds each to the plan's scalar type -- the
 *   statistics are then those of exactly the threshold a later shrink applies --, runs ONE ndwt_band_risk(_items) over all blocks, takes
 *   the first candidate with the smallest estimate, makes it `best` if it is below, and with step = (hi - lo) / 8 continues on
 *   lo = max(best.t - step, 0), hi = min(best.t + step, t_max).  Three rounds resolve t_max / 128.  A block with s = 0, with one element,
 *   or with a NaN keeps the threshold 0.  The detail bands are read `rounds` times.  Refusals: those of ndwt_band_risk; sigma or
 *   thresholds null, sigma negative, NaN or infinite, rounds outside 0 .. 8: NDWT_ERR_INVALID_ARG, nothing is launched.
 * Not built: a device-pointer form of either table; more than 8 candidates in a call; groups across items (the joint form of the
 *   estimate); the MATLAB gateway. */
enum { NDWT_RISK_COUNT = 0, NDWT_RISK_ENERGY = 1, NDWT_RISK_INVSUM = 2, NDWT_RISK_STATS = 3 };
#define NDWT_RISK_MAX_CAND 8
int ndwt_band_risk(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, int nc, const double* cand, double* risk, void* stream);
int ndwt_band_risk_items(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, int nc, const double* cand, double* risk, void* stream);
int ndwt_sure_from_risk(int comp, double n, double s, int nc, const double* cand, const double* risk, double* sure);
int ndwt_sure_thresholds(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double sigma, int rounds, double* thresholds, double* sure, void* stream);
int ndwt_sure_thresholds_items(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, const double* sigma, int rounds, double* thresholds, double* sure,
                               void* stream);
/* ---- joint shrinkage across the items of a plan: the prox of the l2,1 norm (group soft thresholding), and that norm ----
 * The items of a batched, stack or interleaved plan are often coils, echoes, channels, colour planes or traces of ONE object, and the
 * regulariser is joint sparsity: a coefficient survives if the GROUP of coefficients at its position across all items is large.
 * With K = the plan's items and N = the elements of one item of a band, the group at (band b, position p in [0, N)) is c_j = y[b][j][p],
 * j = 0 .. K - 1, every c_j a scalar or an interleaved complex element.  T = the plan's scalar type.  Per group:
 *   s = the sum over j in ascending order of re_j^2 (+ im_j^2, re before im), accumulated in double with a fused multiply-add on the
 *       widened parts, from 0 (the way NDWT_NORM_L2SQ is accumulated);
 *   m = sqrt((T)s): one rounding of s to T, then T's square root;   t = (T)thresholds[b];
 *   m > t: every part of every c_j is multiplied in T by g = 1 (NDWT_SHRINK_HARD) or g = (m - t) / m (NDWT_SHRINK_SOFT, computed in T);
 *   else every part of the group is stored as +0 -- an explicit zero, not c * 0: a group that holds a NaN (m > t is then false) becomes
 *       zeros, as a NaN does in ndwt_shrink of real data.
 * thresholds: HOST, nb = ndwt_num_bands(filtered axes, level) doubles, each >= 0, band 0 a band like any other; thresholds[b] == 0 leaves
 *   band b untouched (no workgroup of that band writes anything); an all-zero array launches and uploads nothing.
 * ndwt_shrink_joint: in place on a level-`level` coefficient array on the device (band_pitch 0 = packed), all bands in ONE launch
 *   (JointShrink) that reads the array once and writes it once where K <= 8 (the group of a step stays in registers); with more items a
 *   workgroup sweeps the items twice, the second sweep reads them again.  The thresholds reach the device as ndwt_shrink_bands_items'
 *   table does, through the plan's pinned host buffer and a copy enqueued on `stream` (items_table_upload, nb entries): a later call
 *   of any of the table forms waits for that copy before it overwrites the pinned buffer.  That wait blocks the HOST
 *   (hipEventSynchronize) until the previous call's copy has run, so a call is at most one call ahead of the device, and two such calls
 *   cannot be captured into a graph.
 * ndwt_denoise_joint: dec into the plan's scratch, the joint shrink, rec -- always this general route.
 * ndwt_group_norms: for every band four doubles in the slots of NDWT_NORM_*, norms: HOST, [nb][4]:
 *   NDWT_NORM_L1    the sum over p of m, every m widened and summed in double: the l2,1 norm of the band
 *   NDWT_NORM_L2SQ  the sum over p of s
 *   NDWT_NORM_MAX   the largest m; a NaN sticks
 *   NDWT_NORM_NNZ   the count of groups with s != 0; a NaN counts
 *   No floating-point atomics; the order of every sum is a fixed function of the shape and the launch geometry, as for ndwt_band_norms.
 *   Synchronous like ndwt_band_norms: enqueues on `stream`, copies the results back once, synchronises the stream once.
 * ndwt_group_norms_dev: the same values into DEVICE memory at norms_dev ([nb][4] doubles, 8-byte aligned); it only enqueues.
 * Every plan kind ndwt_shrink_bands serves; an unbatched plan is one item, and the group is the element.  One launch (GroupNorms),
 *   plus NormsFinish where a band has more than one workgroup; the grid of both kernels: workgroups of 256 threads, a band split into
 *   chunks while every thread keeps max(1, 8 / K) steps -- one step moves a load of every item -- within 16 workgroups per compute unit
 *   and ndwt_plan_set_tuning's target_blocks.  Refusals are those of ndwt_shrink_bands and ndwt_band_norms: plan, y_dev, x_dev, out_dev,
 *   thresholds, norms or norms_dev null, a threshold below 0 or NaN, a mode that is neither, a level outside the plan's, a band pitch
 *   smaller than a band, norms_dev not 8-byte aligned: NDWT_ERR_INVALID_ARG, the message names the argument, nothing is launched.
 * Many short items -- a batch of thousands of traces of a few thousand samples -- take another pair of kernels, JointTile and
 *   GroupNormsTile: a band of few steps gives the kernels above too few workgroups, each thread of which walks all K items one load
 *   behind the other.  There a workgroup takes a strip of 8 steps of a band, all its 256 threads load, 128 items at a time through an
 *   LDS tile, and the threads that own a position still add the items in ascending order: every stored scalar, every s and m, nnz and
 *   max are the same bits as above; l1 and l2sq add the positions in another fixed order (a strip's in LDS, the strips in NormsFinish),
 *   still without atomics.  Taken unasked for data in groups of 4 scalars (y_dev, band_pitch and the item length multiples of 4) where
 *   it was measured at least 10 % faster for the shrink AND for the norms: from 64 items on for items of up to 16384 scalars, from 256
 *   items on for up to 65536 (4096 float signals of 4096 samples: 95 us against 2209 us for the shrink, 55 us against 1342 us for the
 *   norms; torch 150 and 249 us).  With fewer than 64 items, with longer items and for data off the groups of 4 it is never taken
 *   unasked.  The hook is ndwt_plan_set_variant's: variant_inv 11 takes it wherever a launch can number its workgroups (fewer than 2^31
 *   strips in all), variant_inv 9 never takes it; the values do not depend on the route.
 * Not built: a joint form inside the one-launch denoise of a batched 1-D plan (Den1C: a signal lives in one wave there, its neighbours
 *   in other waves); groups over the `inner` axis of an interleaved plan (the samples of one element: they belong to one item); per-item
 *   weights inside the group; a norm fused into the shrink.  The handles, the slab entry points and the MATLAB gateway are unchanged. */
int ndwt_shrink_joint(ndwt_plan* plan, void* y_dev, int64_t band_pitch, int level, const double* thresholds, int mode, void* stream);
int ndwt_denoise_joint(ndwt_plan* plan, const void* x_dev, void* out_dev, int level, const double* thresholds, int mode, void* stream);
int ndwt_group_norms(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* norms, void* stream);
int ndwt_group_norms_dev(ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* norms_dev, void* stream);
/* ---- neighbourhood shrinkage: the energy of a small window inside a coefficient's own band decides that coefficient ----
 * In an undecimated frame an edge or a spike is a cluster of large coefficients at adjacent positions; noise does not cluster.  The rules
 * that use this -- NeighShrink (Chen, Bui and Krzyzak), NeighBlock and NeighCoeff (Cai and Silverman), the locally adaptive Wiener rule
 * (Mihcak et al.) -- share one primitive, built here.  T = the plan's scalar type; d = the filtered axes of one item, 1, 2 or 3, of
 * lengths n_a, axis 0 the fastest; r = radius, 1, 2 or 3; M = (2r + 1)^d.  Positions are those of one item's part of one band, and
 * every index wraps periodically within that item -- the transform's own boundary rule -- never into the next item or band.
 * The window sum at position p, all of it in double:
 *   A(p) = over dx = -r .. r in ascending order along axis 0, for each neighbour re before im, a = fma((double)e, (double)e, a) from
 *          a = 0.0: every square added with a fused multiply-add on the widened part (the way the joint shrink accumulates s);
 *   B(p) = the sum over dy = -r .. r in ascending order along axis 1 of A, plain double additions, the first term first;
 *   C(p) = the same sum over dz along axis 2 of B;
 *   S(p) = A for d = 1, B for d = 2, C for d = 3.  The sum along the last axis is formed anew from its 2r + 1 terms at every position:
 *          no running sum that adds a term and takes one away, so no value depends on where a workgroup's march began.
 * t = (T)thresholds[b]; tt = (double)t * (double)t, formed on the host.
 *   S > tt, compared in double: NDWT_SHRINK_SOFT g = (T)((S - tt) / S) -- a double subtraction, a double division, one rounding to T --
 *       and every part of the coefficient is multiplied by g in T; NDWT_SHRINK_HARD the coefficient is copied;
 *   else every part is stored as +0 -- an explicit zero: a window that holds a NaN turns its centre into zero, as in the joint shrink.
 *   A band with thresholds[b] == 0 is copied to the output bit for bit: NaN, -0 and everything else pass unchanged.
 * The soft rule is c * max(1 - t^2 / S, 0).  With s = sigma * the band's gain (ndwt_band_gains) and N the elements of an item:
 *   t = s * sqrt(2 ln N) is NeighShrink; t^2 = M s^2 the local Wiener estimate c * max(S / M - s^2, 0) / (S / M);
 *   t^2 = 4.50524 M s^2 Cai and Silverman's constant, the root of lambda - ln(lambda) = 3.
 * thresholds: HOST, nb = ndwt_num_bands(filtered axes, level) doubles, each >= 0, band 0 a band like any other -- the rules and the
 *   messages of ndwt_shrink_bands.  The squared thresholds reach the device as the joint shrink's table does, through the plan's
 *   pinned host buffer and a copy enqueued on `stream` (items_table_upload, nb doubles): a later call of any of the table forms waits
 *   on the HOST (hipEventSynchronize) for that copy before it overwrites the pinned buffer, so a call is at most one call ahead of the
 *   device, and two such calls cannot be captured into a graph.
 * ndwt_shrink_neigh is OUT OF PLACE: a neighbour's original value is needed after the neighbour's owner has been processed, so no
 *   in-place form exists across workgroups.  out_dev has the layout and the pitch of y_dev (band_pitch 0 = packed); the call never
 *   writes y_dev and never writes the scalars between the bands of out_dev.  The two arrays may overlap in exactly ONE form,
 *   out_dev == y_dev - band_pitch (in scalars of the pitch: the output is the input moved one band slot down); any other overlap is
 *   refused with NDWT_ERR_INVALID_ARG, "out_dev overlaps y_dev".  In that form band b is written where band b - 1 was read, so the
 *   bands run in ascending order, one launch per band in stream order, and a zero-threshold band is one device-to-device copy.  In
 *   every other case all (band, item) blocks run in ONE launch (NeighShrink), a zero-threshold band is copied inside the kernel, and
 *   an all-zero array uploads and launches nothing: the bands are copied.
 *   The grid: workgroups of 256 threads, nb x items x chunks x tiles of them in the one launch (items x chunks x tiles in a launch
 *   of the shifted form).  A tile is 256 positions of axis 0 for d <= 2, and 64 x 16 positions of axes 0 and 1 for d = 3 (64 x 8 for
 *   complex128, and for double and complex64 at radius 3); the last axis of d >= 2 is marched, split into chunks of at least 2r + 1
 *   planes only while the launch has fewer workgroups than 8 per compute unit (ndwt_plan_set_tuning's target_blocks > 0 stands in for
 *   that count).  No atomics, no hand-off between workgroups: two calls give the same bits whatever the grid.
 * ndwt_denoise_neigh: dec, the shrink, rec without a second coefficient array: the plan's coefficient scratch grows to nb + 1 band
 *   slots (on the first such call only; no other call sees a different scratch), dec writes slots 1 .. nb, the shrink runs one slot
 *   down, rec reads from slot 0.
 * Served: unbatched plans of 1, 2 and 3 dimensions, batched 1-D plans (ndwt_plan_create_many), stacks of images and volumes
 *   (ndwt_plan_create_axes), float, complex64, double and complex128, any band pitch >= a band.
 * Refused with NDWT_ERR_UNSUPPORTED, the message naming the reason: interleaved plans (ndwt_plan_create_interleaved with inner > 1:
 *   the neighbours lie `inner` elements apart); four filtered axes; a filtered axis shorter than 2r + 1 (the window would count an
 *   element twice); an item whose line (plane, for d = 3) reaches 2^31 scalars.
 * Refused with NDWT_ERR_INVALID_ARG, the message naming the argument, nothing launched: plan, y_dev, x_dev, out_dev or thresholds
 *   null, a radius outside 1 .. 3, a mode that is neither, a level outside the plan's, a band pitch smaller than a band, a threshold
 *   below 0 or NaN.
 * Not built: interleaved plans and four filtered axes (refused above); a threshold row per item; a window across levels (parent and
 *   child); the window sum as an output of its own; a statistic fused in; the handles, the slab entry points and the MATLAB gateway. */
int ndwt_shrink_neigh(ndwt_plan* plan, const void* y_dev, void* out_dev, int64_t band_pitch, int level, int radius, const double* thresholds, int mode,
                      void* stream);
int ndwt_denoise_neigh(ndwt_plan* plan, const void* x_dev, void* out_dev, int level, int radius, const double* thresholds, int mode, void* stream);

/* Split complex: separate real / imaginary arrays, the layout the reference's gateway receives from MATLAB
 * (mxGetPr / mxGetPi, nd_dwt_mex.c:55-58,90-93) and hands to nd_dwt_dec / nd_dwt_rec (outR/outI, imageR/imageI,
 * nddwt.h:13-20).  The plan must be NDWT_REAL (real filters: each part is transformed on its own); the imaginary
 * pointers may both be NULL (real data).  Device-pointer and host-pointer forms. */
int ndwt_dec_split(ndwt_plan* plan, const void* x_re, const void* x_im, void* y_re, void* y_im, int level, void* stream);
int ndwt_rec_split(ndwt_plan* plan, const void* y_re, const void* y_im, void* x_re, void* x_im, int level, void* stream);
int ndwt_dec_split_host(ndwt_plan* plan, const void* x_re, const void* x_im, void* y_re, void* y_im, int level);
int ndwt_rec_split_host(ndwt_plan* plan, const void* y_re, const void* y_im, void* x_re, void* x_im, int level);

/* ---- one level on a slab of the outermost axis (multi-GPU building block; no reference counterpart:
 *      the reference is single-process) ------------------------------------------------
 * The plan's dims describe the LOCAL slab (dims[ndim-1] = local planes).  `stride` is the tap stride of
 * this level (1 in reference mode).  Analysis: `in` holds halo_before + local + halo_after planes of the
 * approximation band, halo_before = (L/2-1)*stride, halo_after = (L/2)*stride for the outer axis' filter
 * length L; the 2^d outputs are local-sized.  Synthesis: every one of the 2^d inputs holds
 * halo_before = (L/2)*stride and halo_after = (L/2-1)*stride planes around the local slab.
 * ndwt_slab_halo() reports those four numbers. */
/* 1 when the plan offers the slab forms that read a slab in place (split-halo analysis, runs of the zero-extended synthesis:
 * a 3-D plan on the fused kernels whose outer-axis filter is its longest; z-slab plans: the zero-extended synthesis, i.e. the fused
 * kernels with the z filter the longest), else 0 */
int ndwt_plan_slab_fast(const ndwt_plan* plan);
int ndwt_slab_halo(const ndwt_plan* plan, int stride, int64_t* ana_before, int64_t* ana_after,
                   int64_t* syn_before, int64_t* syn_after);
int ndwt_analysis_level_slab(ndwt_plan* plan, const void* in_with_halo, void* const* out_bands, int stride, void* stream);
int ndwt_synthesis_level_slab(ndwt_plan* plan, const void* const* in_bands_with_halo, void* out, int stride, void* stream);
/* Copy-free forms for fused 3-D plans (NDWT_ERR_UNSUPPORTED otherwise; the outer-axis filter must be the longest):
 * analysis reads the local slab and the two halo buffers (as received from the neighbours) from separate pointers;
 * synthesis treats the local coefficient slab as zero outside and writes syn_after + local + syn_before planes:
 * the local result plus the partial sums owed to the neighbouring slabs (they are sent there and added -- 1 band of
 * exchange instead of the halo of all 2^d bands).  The zero-extended synthesis also takes 4-D plans sharded on t (16 bands:
 * the 3-D part runs per frame, the t-axis pass over zero-padded frames). */
int ndwt_analysis_level_slab_split(ndwt_plan* plan, const void* in_local, const void* halo_before, const void* halo_after,
                                   void* const* out_bands, int stride, void* stream);
int ndwt_synthesis_level_slab_ext(ndwt_plan* plan, const void* const* in_bands_local, void* out_ext, int stride, void* stream);

/* Runs of planes of the two calls above, so that the exchange can overlap with the planes that do not wait for it.
 * analysis_part: n_planes output planes; in_local points at the first of them, halo_before at the (L/2-1) planes
 *   before it and halo_after at the (L/2) planes after the run -- each may point into the slab itself or into a
 *   received buffer; out[b] points at the first output plane of band b.
 * synthesis_part: output planes [e0, e0 + n_out) of the zero-extended synthesis of n_in coefficient planes
 *   (in_local[b] = first plane of band b; result plane e sums coefficient planes e-(L-1)..e, so planes
 *   [0, L/2-1) and [n_in + L/2-1, n_in + L-1) are the partial sums owed to the neighbours). */
int ndwt_analysis_level_slab_part(ndwt_plan* plan, const void* in_local, const void* halo_before, const void* halo_after,
                                  void* const* out_bands, int stride, int64_t n_planes, void* stream);
int ndwt_synthesis_level_slab_part(ndwt_plan* plan, const void* const* in_local, int64_t n_in, int64_t e0, int64_t n_out,
                                   void* out, int stride, void* stream);
/* Several equal runs in one launch (the two ends of a slab):
 * analysis_runs: the input carries its halo contiguously (as for ndwt_analysis_level_slab); run r reads from
 *   in_with_halo + r*run_stride planes and writes n_planes planes at out[b] + r*run_stride planes.
 * synthesis_runs: run r = planes [e0 + r*e_stride, +n_out) of the zero-extended result, written to out + r*n_out planes. */
int ndwt_analysis_level_slab_runs(ndwt_plan* plan, const void* in_with_halo, void* const* out_bands, int stride, int64_t n_planes,
                                  int64_t n_runs, int64_t run_stride, void* stream);
int ndwt_synthesis_level_slab_runs(ndwt_plan* plan, const void* const* in_local, int64_t n_in, int64_t e0, int64_t e_stride,
                                   int64_t n_runs, int64_t n_out, void* out, int stride, void* stream);

/* Up to NDWT_MAX_SEGMENTS runs of planes copied (op NDWT_SEG_COPY) or added (NDWT_SEG_ADD: dst[i] += src[i]) in ONE launch on
 * `stream`, on the plan's device: the halo planes a slab takes from itself, and the partial sums received from the two neighbours
 * added to the slab's edge planes -- a launch costs about 6 us on MI355X whatever it moves, and a level has two such runs.
 * count[i] = elements (of the plan's scalar type; complex data: 2 per element) of run i; runs must not overlap each other. */
#define NDWT_MAX_SEGMENTS 8
#define NDWT_SEG_COPY 0
#define NDWT_SEG_ADD 1
int ndwt_slab_segments(ndwt_plan* plan, int op, int nseg, void* const* dst, const void* const* src, const int64_t* count, void* stream);
/* The strided form: `nrep` repetitions of every run in ONE launch, repetition r of run i at dst[i] + r * dst_stride[i] and
 * src[i] + r * src_stride[i] (scalars, like count) -- the planes of a z-slab are one run per frame (nt runs per halo).  Repetitions of a
 * run must not overlap in dst (dst_stride[i] >= count[i] when nrep > 1).  The pointers may lie on another device with peer access. */
int ndwt_slab_segments_strided(ndwt_plan* plan, int op, int nseg, void* const* dst, const void* const* src, const int64_t* count, int64_t nrep,
                               const int64_t* dst_stride, const int64_t* src_stride, void* stream);

/* ---- single-process multi-device plan (hard part 5; section 8b `devices[]`) ---------------------------
 * The reference's host is ONE process calling one gateway (nd_dwt_3D.m:161,225): this is the multi-GPU path that fits behind
 * that call.  The volume is sharded in slabs on its outermost axis over devices[0..ndev) (a device may appear more than once:
 * independent slabs and streams on one GPU); one host thread drives all of them, planes move between slabs with asynchronous
 * device-to-device (peer, xGMI) copies ordered by events.  ndim 2..4.  Errors: ndwt_mplan_last_error().
 *   ndwt_mdec / ndwt_mrec: DEVICE-RESIDENT data, one pointer per slab (ndwt_mplan_slab gives its device and planes): x_slabs[i] =
 *     the n_i planes of the signal on slab i's device, y_slabs[i] = its coefficient slab, band b at b * n_i planes.  The kernels
 *     read and write these buffers in place.  The data must be complete when the call is made; the call returns when the result is.
 *   ndwt_mdec_host / ndwt_mrec_host: whole-volume host arrays (the layout of ndwt_dec_host / ndwt_rec_host), staged through
 *     slab buffers of the plan.
 *   Exchange per level: analysis -- halo planes of the approximation band (bit-identical to one device).  Synthesis --
 *     NDWT_EXCHANGE_SCATTER (default where every level runs the fused 3-D kernels): each slab reconstructs its own coefficients
 *     zero-extended and sends ONE band of partial sums for the L-1 planes around it, which their owners add in a fixed order
 *     (equal to one device to rounding); NDWT_EXCHANGE_GATHER: halo planes of all 2^d bands assembled with a copy of the slab
 *     (bit-identical to one device; what plans on the per-axis kernels, dilated levels, 2-D and 4-D plans use anyway). */
typedef struct ndwt_mplan ndwt_mplan;
enum { NDWT_EXCHANGE_SCATTER = 0, NDWT_EXCHANGE_GATHER = 1 };
int ndwt_mplan_create(ndwt_mplan** plan, int ndim, const int64_t* dims, const char* const* wnames, int dtype, int complexity,
                      int pres_l2_norm, int dilation, int max_level, const int* devices, int ndev);
/* The same with the sharded axis chosen (ndwt_plan_create_slab_axis): ndim - 1 = ndwt_mplan_create, 2 with ndim == 4 = z-slabs, t whole
 * on every slab.  ndwt_mplan_slab then reports first plane and planes along z; the slab buffers of ndwt_mdec / ndwt_mrec are
 * (nt, nz_i, ny, nx), band-planar ((bands, nt, nz_i, ny, nx)); the host forms take the whole-volume arrays as before.  Planes move between
 * slabs with ndwt_slab_segments_strided where the devices are the same or have peer access, else one peer copy per frame.  The exchange
 * schemes and barriers are those of t-slabs (scatter where the slab plans offer the zero-extended synthesis); the overlapped schedule is
 * not offered (exchange, then compute). */
int ndwt_mplan_create_axis(ndwt_mplan** plan, int ndim, const int64_t* dims, const char* const* wnames, int dtype, int complexity,
                           int pres_l2_norm, int dilation, int max_level, const int* devices, int ndev, int shard_axis);
int ndwt_mplan_destroy(ndwt_mplan* plan);
int ndwt_mplan_num_slabs(const ndwt_mplan* plan);
int ndwt_mplan_slab(const ndwt_mplan* plan, int idx, int* device, int64_t* first_plane, int64_t* planes);
int ndwt_mplan_set_exchange(ndwt_mplan* plan, int exchange);
/* 1 (default): the planes moved between slabs travel on per-slab copy streams while the launches that do not need them run (fused 3-D
 * plans at tap stride 1 whose slabs are thicker than twice the halo; the interior planes first, then the ends / the partial sums first,
 * then the slab's own planes); 0: exchange, then one launch per slab and level.  Same results either way.  (2: like 1, with the partial
 * sums staged through the receive buffers even between slabs that share a device -- how the tests run that path on one GPU.) */
int ndwt_mplan_set_overlap(ndwt_mplan* plan, int overlap);
int ndwt_mplan_describe(const ndwt_mplan* plan, char* buf, int buflen);   /* slabs, exchange schemes, peer-access findings */
/* 1 (default with more than one slab): one host thread per slab queues that slab's work (persistent workers of the plan: asleep between
 * calls; the calling thread drives slab 0 and returns when every device has finished, as before); 0: the calling thread queues everything.
 * Same work on the same streams in the same per-stream order: identical results.  Queueing a 512^3 db4 dec + rec for 8 slabs from one
 * thread takes 1.7 ms of host time -- more than one of 8 devices needs to compute its share. */
int ndwt_mplan_set_threads(ndwt_mplan* plan, int threads);
/* diagnostic: host microseconds the last ndwt_mdec / ndwt_mrec spent QUEUEING work for all slabs (one host thread drives every device: with
 * many devices this, not the devices, can bound a call); -1 without a plan */
double ndwt_mplan_last_enqueue_us(const ndwt_mplan* plan);
int ndwt_mdec(ndwt_mplan* plan, const void* const* x_slabs, void* const* y_slabs, int level);
int ndwt_mrec(ndwt_mplan* plan, const void* const* y_slabs, void* const* x_slabs, int level);
int ndwt_mdec_host(ndwt_mplan* plan, const void* x_host, void* y_host, int level);
int ndwt_mrec_host(ndwt_mplan* plan, const void* y_host, void* x_host, int level);
const char* ndwt_mplan_last_error(void);

/* ---- exchange of the one-process-per-GPU driver: RCCL point-to-point calls on the caller's stream ------------------------------------
 * (ncclSend / ncclRecv inside ncclGroupStart / ncclGroupEnd between ring neighbours.)  torch.distributed's
 * batch_isend_irecv runs its RCCL work on a stream of its own: every exchange then pays two cross-stream dependencies (40 + 14 us around a
 * 15-us RCCL kernel on one MI355X, six times per dec + rec step of 0.83 ms); enqueued on the stream that runs the transform, the same grouped
 * send / receive is one more kernel in stream order.  librccl is opened at run time (no link-time dependency).
 * Rank 0 obtains a 128-byte id (ndwt_comm_unique_id) and hands it to every rank by whatever means the host has (the Python driver
 * broadcasts it through torch.distributed); every rank then calls ndwt_comm_create (collective).  ndwt_comm_exchange enqueues one group of
 * sends / receives: op i moves bytes[i] bytes at ptrs[i] to (is_send[i] != 0) or from rank peers[i]; between two ranks, sends and receives are
 * matched in the order they are listed.  Stream-ordered: the buffers may be reused by later work on `stream` without further waiting. */
typedef struct ndwt_comm ndwt_comm;
int ndwt_comm_unique_id(void* id128);
int ndwt_comm_create(ndwt_comm** comm, const void* id128, int nranks, int rank, int device);
int ndwt_comm_destroy(ndwt_comm* comm);
int ndwt_comm_exchange(ndwt_comm* comm, int nops, const int* is_send, void* const* ptrs, const int64_t* bytes, const int* peers, void* stream);
const char* ndwt_comm_last_error(void);

/* ---- errors ------------------------------------------------------------------------------------------ */
const char* ndwt_last_error(void); /* thread-local message of the last failing call */
const char* ndwt_version(void);

/* ---- launch trace (tests / diagnostics) -------------------------------------------------------------- */
/* Off by default.  While on, every kernel launch of this library (worker threads of ndwt_mplan_* included) appends one record
 * "<kernel type> grid=(x,y,z) block=(x,y,z)" to a process-global log; the kernel type is the compiler's spelling, which leaves out
 * trailing template arguments equal to their defaults.  Host-side only: it changes no result and no launch.
 * ndwt_trace_enable: on != 0 clears the log and starts recording, 0 stops; returns the previous state.
 * ndwt_trace_get: copies the newline-separated records (NUL-terminated, truncated to buflen - 1 bytes) and returns the buffer
 * length the whole log needs, terminator included. */
int ndwt_trace_enable(int on);
int ndwt_trace_get(char* buf, int buflen);

#ifdef __cplusplus
}
#endif
#endif /* NDWT_H */
