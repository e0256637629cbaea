"""Host-side mirror of the reference's class API for the NDWT hot path.

Reference: Functions/nd_dwt_1D.m, nd_dwt_2D.m, nd_dwt_3D.m, nd_dwt_4D.m -- constructor
`nd_dwt_3D(wname, sizes, 'pres_l2_norm', b, 'compute', c, 'precision', p)`, `dec(x, level)`, `rec(y)`
and the public properties (nd_dwt_3D.m:67-75).  Everything is computed by the HIP library behind
include/ndwt.h; PyTorch only provides device memory and the current stream.

Shapes follow MATLAB: x is `sizes` = [n1, ..., nd]; coefficients are [n1, ..., nd, bands] with the
band order of the reference (nd_dwt_3D.m:45-52).  Memory is column-major like MATLAB's: the tensors
returned are permuted views of contiguous (bands, nd, ..., n1) buffers, and column-major inputs are
consumed without a copy.

`compute` values: 'hip' -- torch tensors on the GPU in and out (the analogue of the reference's
'gpu'); 'hip_off' -- host arrays (numpy / CPU tensors) in and out, staged through the GPU (the
analogue of 'gpu_off').  The reference's own names are accepted as aliases for the data placement
they imply ('gpu' -> 'hip'; 'gpu_off', 'mat', 'mex' -> 'hip_off'); the arithmetic is always the HIP
engine's.  There is no CPU compute path.
"""
from __future__ import annotations

import ctypes
import warnings

import numpy as np
import torch

from . import _lib as L

_ORD = ["First", "Second", "Third", "Fourth"]


class Plan:
    """Thin RAII wrapper over ndwt_plan (include/ndwt.h)."""

    def __init__(self, dims, wnames, dtype, complex_interleaved=False, pres_l2_norm=False, dilation="reference",
                 max_level=1, device=0, global_outer=None, shard_axis=None, howmany=None, axes=None, inner=None):
        """howmany: None = one array (ndwt_plan_create); a number = a batched plan of that many 1-D signals (ndwt_plan_create_many):
        signal k at k * dims[0] elements, every band a contiguous (howmany, n) block.
        axes: a tuple of axis numbers (0 = the fastest) = only these axes of `dims`, the WHOLE array, are filtered
        (ndwt_plan_create_axes; served: the leading axes (0, .., k-1)).  With k < len(dims) the plan is a stack: the prod(dims[k:]) items
        lie back to back and each gets the k-D transform; every band is a whole array.  Not together with `howmany`.
        A run of adjacent axes (a, .., a+k-1) with a > 0 is a plan over interleaved samples (ndwt_plan_create_interleaved):
        inner = prod(dims[:a]), the filtered axes dims[a:a+k], howmany = prod(dims[a+k:]); the names of the axes left alone are ignored.
        inner: a number = each sample is that many elements lying together, the array is [inner, dims.., howmany] (howmany: None = 1) and
        `dims` / `wnames` describe one item (ndwt_plan_create_interleaved).  Not together with `axes`.
        global_outer: length of the sharded axis of the WHOLE volume when `dims` describe one slab of it (multi-GPU):
        the reference's filter-length check then applies to the whole axis, a slab may be thinner than the filter.
        shard_axis: the sharded axis, counted from the fastest (0 = x); None = the outermost (ndwt_plan_create_slab), 2 of a 4-D
        volume = z-slabs (ndwt_plan_create_slab_axis)"""
        self.dims = [int(d) for d in dims]
        self.ndim = len(self.dims)
        self.wnames = list(wnames)
        self.dtype = dtype
        self.max_level = int(max_level)
        self.device = int(device)
        self._h = ctypes.c_void_p(None)
        dims_c = (ctypes.c_int64 * self.ndim)(*self.dims)
        names_c = (ctypes.c_char_p * self.ndim)(*[None if w is None else w.encode() for w in self.wnames])
        dt = L.NDWT_F32 if dtype in (torch.float32, np.float32, "single") else L.NDWT_F64
        dil = {"reference": L.NDWT_DILATION_REFERENCE, "atrous": L.NDWT_DILATION_ATROUS}[dilation]
        cplx = L.NDWT_COMPLEX_INTERLEAVED if complex_interleaved else L.NDWT_REAL
        self.shard_axis = self.ndim - 1 if shard_axis is None else int(shard_axis)
        self.howmany = None if howmany is None else int(howmany)
        self.axes = None if axes is None else tuple(int(a) for a in axes)
        self.inner = None if inner is None else int(inner)
        if inner is not None and axes is not None:
            raise ValueError("'axes' and 'inner' are two ways to say the same thing: give one of them")
        if axes is not None and howmany is None and shard_axis is None and global_outer is None:
            ax = sorted(self.axes)
            if (len(set(ax)) == len(ax) and ax[0] > 0 and ax[-1] < self.ndim and ax == list(range(ax[0], ax[-1] + 1))):
                # a run of adjacent axes that does not start at 0: the axes below it are the sample, those above it the items
                whole, names = self.dims, self.wnames
                self.inner = int(np.prod(whole[:ax[0]], dtype=np.int64))
                self.howmany = int(np.prod(whole[ax[-1] + 1:], dtype=np.int64))
                item = whole[ax[0]:ax[-1] + 1]
                self._create_interleaved(item, names[ax[0]:ax[-1] + 1], dt, cplx, pres_l2_norm, dil)
                return
        if inner is not None:
            if shard_axis is not None or global_outer is not None:
                raise ValueError("a plan over interleaved samples is not a slab plan")
            self.howmany = 1 if howmany is None else int(howmany)
            self._create_interleaved(self.dims, self.wnames, dt, cplx, pres_l2_norm, dil)
        elif axes is not None:
            if howmany is not None:
                raise ValueError("'axes' and 'howmany' are two ways to say the same thing: give one of them")
            if shard_axis is not None or global_outer is not None:
                raise ValueError("a plan over some axes is not a slab plan")
            if any(a < 0 or a > 31 for a in self.axes) or len(set(self.axes)) != len(self.axes):
                raise ValueError(f"axes must be distinct axis numbers >= 0 (got {self.axes})")
            mask = 0
            for a in self.axes:
                mask |= 1 << a
            L.check(L.lib().ndwt_plan_create_axes(ctypes.byref(self._h), self.ndim, dims_c, mask, names_c, dt, cplx,
                                                  int(bool(pres_l2_norm)), dil, self.max_level, self.device))
        elif howmany is not None:
            if shard_axis is not None or global_outer is not None:
                raise ValueError("a batched plan is not a slab plan")
            L.check(L.lib().ndwt_plan_create_many(ctypes.byref(self._h), self.ndim, dims_c, self.howmany, names_c, dt, cplx,
                                                  int(bool(pres_l2_norm)), dil, self.max_level, self.device))
        elif shard_axis is not None:
            L.check(L.lib().ndwt_plan_create_slab_axis(ctypes.byref(self._h), self.ndim, dims_c, self.shard_axis,
                                                       int(global_outer if global_outer is not None else self.dims[self.shard_axis]),
                                                       names_c, dt, cplx, int(bool(pres_l2_norm)), dil, self.max_level, self.device))
        elif global_outer is None:
            L.check(L.lib().ndwt_plan_create(ctypes.byref(self._h), self.ndim, dims_c, names_c, dt, cplx,
                                             int(bool(pres_l2_norm)), dil, self.max_level, self.device))
        else:
            L.check(L.lib().ndwt_plan_create_slab(ctypes.byref(self._h), self.ndim, dims_c, int(global_outer), names_c, dt, cplx,
                                                  int(bool(pres_l2_norm)), dil, self.max_level, self.device))

    def _create_interleaved(self, item_dims, item_names, dt, cplx, pres_l2_norm, dil):
        k = len(item_dims)
        dims_c = (ctypes.c_int64 * max(k, 1))(*item_dims)
        names_c = (ctypes.c_char_p * max(k, 1))(*[None if w is None else w.encode() for w in item_names])
        L.check(L.lib().ndwt_plan_create_interleaved(ctypes.byref(self._h), k, dims_c, self.inner, self.howmany, names_c, dt, cplx,
                                                     int(bool(pres_l2_norm)), dil, self.max_level, self.device))

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                L.lib().ndwt_plan_destroy(self._h)
                self._h = ctypes.c_void_p(None)
        except Exception:
            pass

    def set_path(self, generic: bool):
        L.check(L.lib().ndwt_plan_set_path(self._h, L.NDWT_PATH_GENERIC if generic else L.NDWT_PATH_AUTO))

    def set_tuning(self, target_blocks=0, force_zchunk=0):
        L.check(L.lib().ndwt_plan_set_tuning(self._h, int(target_blocks), int(force_zchunk)))

    def set_variant(self, fwd=-1, inv=-1, zchunk_fwd=-1, zchunk_inv=-1, fp64_fused=-1):
        """tuning hook of tools/ (A/B runs of kernel variants; same values): negative = unchanged"""
        L.check(L.lib().ndwt_plan_set_variant(self._h, int(fwd), int(inv), int(zchunk_fwd), int(zchunk_inv), int(fp64_fused)))
        return self

    def set_fused_level1(self, mode):
        """tuning hook: 0 / False = denoise() keeps the level-1 detail bands in memory; 1 / True (default) = level 1 in one launch where
        that is faster (tap lengths <= 6); 2 = wherever the kernel exists (8 taps too)"""
        L.check(L.lib().ndwt_plan_set_fused_level1(self._h, int(mode)))
        return self

    def set_variant_from_env(self):
        """tools/ only: NDWT_VARIANT_FWD / NDWT_VARIANT_INV / NDWT_ZCHUNK_FWD / NDWT_ZCHUNK_INV / NDWT_FP64_FUSED of the caller's
        environment, applied through set_variant (the library itself never reads the environment)"""
        import os
        g = lambda k: int(os.environ[k]) if os.environ.get(k) not in (None, "") else -1
        return self.set_variant(g("NDWT_VARIANT_FWD"), g("NDWT_VARIANT_INV"), g("NDWT_ZCHUNK_FWD"), g("NDWT_ZCHUNK_INV"), g("NDWT_FP64_FUSED"))

    def set_profiling(self, on: bool):
        L.check(L.lib().ndwt_plan_set_profiling(self._h, int(bool(on))))

    def get_profile(self, kind: int):
        """(total_ms, launches) of kernel kind 0 fused analysis, 1 fused synthesis, 2 axis analysis, 3 axis synthesis"""
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        L.check(L.lib().ndwt_plan_get_profile(self._h, int(kind), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def describe(self) -> str:
        buf = ctypes.create_string_buffer(64)
        L.check(L.lib().ndwt_plan_describe(self._h, buf, 64))
        return buf.value.decode()

    def band_pitch(self) -> int:
        """recommended band pitch of a pitched coefficient buffer, in elements (include/ndwt.h: ndwt_band_pitch)"""
        return int(L.lib().ndwt_band_pitch(self._h))

    def dec(self, x_ptr, y_ptr, level, stream=0, band_pitch=0):
        """band_pitch: elements between consecutive bands of y (0 = packed, the reference layout)"""
        L.check(L.lib().ndwt_dec_pitched(self._h, x_ptr, y_ptr, int(band_pitch), int(level), ctypes.c_void_p(stream)))

    def rec(self, y_ptr, x_ptr, level, stream=0, band_pitch=0):
        L.check(L.lib().ndwt_rec_pitched(self._h, y_ptr, int(band_pitch), x_ptr, int(level), ctypes.c_void_p(stream)))

    def shrink(self, y_ptr, level, threshold, hard=False, stream=0, band_pitch=0):
        """in-place soft (default) / hard thresholding of the detail bands"""
        L.check(L.lib().ndwt_shrink_pitched(self._h, y_ptr, int(band_pitch), int(level), float(threshold), int(bool(hard)), ctypes.c_void_p(stream)))

    def denoise(self, x_ptr, out_ptr, level, threshold, hard=False, stream=0):
        """dec -> shrink -> rec with the coefficients in a scratch array owned by the plan"""
        L.check(L.lib().ndwt_denoise(self._h, x_ptr, out_ptr, int(level), float(threshold), int(bool(hard)), ctypes.c_void_p(stream)))

    def _check_band_count(self, t, level):
        nb = num_bands(self.ndim if self.axes is None else len(self.axes), level)   # (the filtered axes)
        if t.size != nb:
            raise ValueError(f"{nb} thresholds expected (one per band of a {level}-level transform), got {t.size}")

    @staticmethod
    def _thresholds(thresholds):
        t = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
        return t, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def shrink_bands(self, y_ptr, level, thresholds, hard=False, stream=0, band_pitch=0):
        """in-place thresholding with one threshold per band (num_bands of them, band 0 included; 0 = leave the band alone)"""
        t, tp = self._thresholds(thresholds)
        self._check_band_count(t, level)
        L.check(L.lib().ndwt_shrink_bands(self._h, y_ptr, int(band_pitch), int(level), tp, int(bool(hard)), ctypes.c_void_p(stream)))

    def denoise_bands(self, x_ptr, out_ptr, level, thresholds, hard=False, stream=0):
        """dec -> per-band shrink -> rec; a batched 1-D plan can run it in one launch (set_variant(fwd=11, inv=11))"""
        t, tp = self._thresholds(thresholds)
        self._check_band_count(t, level)
        L.check(L.lib().ndwt_denoise_bands(self._h, x_ptr, out_ptr, int(level), tp, int(bool(hard)), ctypes.c_void_p(stream)))

    def band_select(self, y_ptr, level, band, ks, stream=0, band_pitch=0):
        """the ks[i]-th smallest (0-based) |c| of band `band` of a level-`level` coefficient array on the device, exactly, as a numpy array
        of doubles (include/ndwt.h: ndwt_band_select): up to 4 ranks per call; complex data: the magnitude the shrink compares.  The band
        is the plan's whole array (all signals of a batch, all items of a stack).  Synchronous: the results are host values."""
        k = np.ascontiguousarray(np.asarray(ks, dtype=np.int64).reshape(-1))
        out = np.zeros(max(k.size, 1))
        L.check(L.lib().ndwt_band_select(self._h, y_ptr, int(band_pitch), int(level), int(band), int(k.size), k.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_void_p(stream)))
        return out[:k.size]

    def estimate_sigma_coef(self, y_ptr, level, stream=0, band_pitch=0):
        """sigma of white noise in the SIGNAL from a coefficient array on the device: median |c| of the last band / 0.6745 / its gain
        (complex data: / 1.1774, the sigma of each of the real and imaginary parts) -- include/ndwt.h: ndwt_estimate_sigma_coef"""
        s = ctypes.c_double(0.0)
        L.check(L.lib().ndwt_estimate_sigma_coef(self._h, y_ptr, int(band_pitch), int(level), ctypes.byref(s), ctypes.c_void_p(stream)))
        return float(s.value)

    def estimate_sigma(self, x_ptr, stream=0):
        """the same from a signal on the device: one level-1 dec into the plan's coefficient scratch, then estimate_sigma_coef"""
        s = ctypes.c_double(0.0)
        L.check(L.lib().ndwt_estimate_sigma(self._h, x_ptr, ctypes.byref(s), ctypes.c_void_p(stream)))
        return float(s.value)

    # -- the per-item forms (include/ndwt.h): an item is one signal of a batch, one image / volume of a stack, one block of interleaved samples --
    @property
    def items(self):
        """items of the plan: the signals of a batch, the images / volumes of a stack (the axes of `dims` that are not filtered), the
        blocks of interleaved samples; 1 for one array"""
        if self.howmany:
            return int(self.howmany)
        if self.axes is not None:
            return int(np.prod([d for a, d in enumerate(self.dims) if a not in self.axes], dtype=np.int64))
        return 1

    def _item_table(self, thresholds, level):
        nb = num_bands(self.ndim if self.axes is None else len(self.axes), level)   # (the filtered axes)
        t = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64))
        if t.shape != (self.items, nb):
            raise ValueError(f"a [{self.items}, {nb}] array of thresholds expected (items x bands of a {level}-level transform), got {list(t.shape)}")
        return t, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def band_select_items(self, y_ptr, level, band, ks, stream=0, band_pitch=0):
        """band_select for every item: an [items, len(ks)] array, row j the ks[i]-th smallest |c| of item j's part of the band; the ranks
        count inside ONE item (include/ndwt.h: ndwt_band_select_items).  Synchronous."""
        k = np.ascontiguousarray(np.asarray(ks, dtype=np.int64).reshape(-1))
        out = np.zeros((self.items, max(k.size, 1)))
        L.check(L.lib().ndwt_band_select_items(self._h, y_ptr, int(band_pitch), int(level), int(band), int(k.size), k.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_void_p(stream)))
        return out.reshape(-1)[:self.items * k.size].reshape(self.items, k.size)

    def estimate_sigma_coef_items(self, y_ptr, level, stream=0, band_pitch=0):
        """estimate_sigma_coef for every item: a length-`items` array"""
        s = np.zeros(self.items)
        L.check(L.lib().ndwt_estimate_sigma_coef_items(self._h, y_ptr, int(band_pitch), int(level), s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                       ctypes.c_void_p(stream)))
        return s

    def estimate_sigma_items(self, x_ptr, stream=0):
        """estimate_sigma for every item: a length-`items` array"""
        s = np.zeros(self.items)
        L.check(L.lib().ndwt_estimate_sigma_items(self._h, x_ptr, s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_void_p(stream)))
        return s

    def shrink_bands_items(self, y_ptr, level, thresholds, hard=False, stream=0, band_pitch=0):
        """in-place thresholding with an [items, num_bands] array: entry [j, b] for item j's part of band b (0 = leave it alone), all in one launch"""
        t, tp = self._item_table(thresholds, level)
        L.check(L.lib().ndwt_shrink_bands_items(self._h, y_ptr, int(band_pitch), int(level), tp, int(bool(hard)), ctypes.c_void_p(stream)))

    def denoise_bands_items(self, x_ptr, out_ptr, level, thresholds, hard=False, stream=0):
        """dec -> shrink_bands_items -> rec with the coefficients in the plan's scratch"""
        t, tp = self._item_table(thresholds, level)
        L.check(L.lib().ndwt_denoise_bands_items(self._h, x_ptr, out_ptr, int(level), tp, int(bool(hard)), ctypes.c_void_p(stream)))

    # -- the band norms (include/ndwt.h: ndwt_band_norms): column NDWT_NORM_L1 / _L2SQ / _MAX / _NNZ of every band, in one read --
    def _num_bands(self, level):
        return num_bands(self.ndim if self.axes is None else len(self.axes), level)   # (the filtered axes)

    def band_norms(self, y_ptr, level, stream=0, band_pitch=0):
        """an [nb, 4] array: sum |c|, sum |c|^2, max |c| and the count of non-zeros of every band of a level-`level` coefficient array on the
        device, the band being the plan's whole array (all items pooled); complex data: the magnitude the shrink compares.  Synchronous."""
        out = np.zeros((self._num_bands(level), L.NDWT_NORM_COUNT))
        L.check(L.lib().ndwt_band_norms(self._h, y_ptr, int(band_pitch), int(level), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_void_p(stream)))
        return out

    def band_norms_items(self, y_ptr, level, stream=0, band_pitch=0):
        """band_norms for every item: an [items, nb, 4] array, [j, b] from item j's part of band b alone.  Synchronous."""
        out = np.zeros((self.items, self._num_bands(level), L.NDWT_NORM_COUNT))
        L.check(L.lib().ndwt_band_norms_items(self._h, y_ptr, int(band_pitch), int(level), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              ctypes.c_void_p(stream)))
        return out

    def band_norms_dev(self, y_ptr, level, out_ptr, per_item=False, stream=0, band_pitch=0):
        """the same into DEVICE memory at out_ptr ([nb, 4] doubles, per_item: [items, nb, 4]; 8-byte aligned): enqueued on `stream` only, no
        copy and no synchronisation -- the results are there in stream order"""
        L.check(L.lib().ndwt_band_norms_dev(self._h, y_ptr, int(band_pitch), int(level), int(bool(per_item)), out_ptr, ctypes.c_void_p(stream)))

    # -- the SURE statistics and the threshold search (include/ndwt.h: ndwt_band_risk, ndwt_sure_thresholds) --
    def _risk_table(self, cand, level, items):
        nb = self._num_bands(level)
        c = np.ascontiguousarray(np.asarray(cand, dtype=np.float64))
        lead = (nb,) if items is None else (items, nb)
        if c.shape[:-1] != lead or c.ndim != len(lead) + 1:
            raise ValueError(f"a {list(lead) + ['nc']} array of candidate thresholds expected, got {list(c.shape)}")
        if not 1 <= c.shape[-1] <= L.NDWT_RISK_MAX_CAND:
            raise ValueError(f"1 to {L.NDWT_RISK_MAX_CAND} candidates per block, got {c.shape[-1]}")
        return c, np.zeros(c.shape + (L.NDWT_RISK_STATS,))

    def band_risk(self, y_ptr, level, cand, stream=0, band_pitch=0):
        """an [nb, nc, 3] array: for every band of a level-`level` coefficient array on the device (the plan's whole array, all items
        pooled) and every candidate threshold cand[b, i] the count of |c| <= t, the energy of those elements and (complex data) the sum
        of 1 / |c| over the others, in one read of the array.  cand: [nb, nc], nc <= 8; a row that begins with a negative entry skips
        its band (zeros).  Synchronous."""
        c, out = self._risk_table(cand, level, None)
        dp = ctypes.POINTER(ctypes.c_double)
        L.check(L.lib().ndwt_band_risk(self._h, y_ptr, int(band_pitch), int(level), int(c.shape[-1]), c.ctypes.data_as(dp), out.ctypes.data_as(dp), ctypes.c_void_p(stream)))
        return out

    def band_risk_items(self, y_ptr, level, cand, stream=0, band_pitch=0):
        """band_risk for every item: cand [items, nb, nc], an [items, nb, nc, 3] array.  Synchronous."""
        c, out = self._risk_table(cand, level, self.items)
        dp = ctypes.POINTER(ctypes.c_double)
        L.check(L.lib().ndwt_band_risk_items(self._h, y_ptr, int(band_pitch), int(level), int(c.shape[-1]), c.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                             ctypes.c_void_p(stream)))
        return out

    def sure_thresholds(self, y_ptr, level, sigma, rounds=3, stream=0, band_pitch=0):
        """(thresholds, sure): for every band the soft threshold that minimises Stein's unbiased risk estimate on [0, sigma * gain *
        sqrt(2 ln N)], searched in `rounds` reads of the detail bands, and the estimate there; band 0 gets 0.  Two length-nb arrays."""
        nb = self._num_bands(level)
        thr, sure = np.zeros(nb), np.zeros(nb)
        dp = ctypes.POINTER(ctypes.c_double)
        L.check(L.lib().ndwt_sure_thresholds(self._h, y_ptr, int(band_pitch), int(level), float(sigma), int(rounds), thr.ctypes.data_as(dp), sure.ctypes.data_as(dp),
                                             ctypes.c_void_p(stream)))
        return thr, sure

    def sure_thresholds_items(self, y_ptr, level, sigma, rounds=3, stream=0, band_pitch=0):
        """sure_thresholds for every item with its own sigma (a length-`items` sequence): two [items, nb] arrays"""
        s = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(-1))
        if s.size != self.items:
            raise ValueError(f"{self.items} values of sigma expected, one per item, got {s.size}")
        nb = self._num_bands(level)
        thr, sure = np.zeros((self.items, nb)), np.zeros((self.items, nb))
        dp = ctypes.POINTER(ctypes.c_double)
        L.check(L.lib().ndwt_sure_thresholds_items(self._h, y_ptr, int(band_pitch), int(level), s.ctypes.data_as(dp), int(rounds), thr.ctypes.data_as(dp),
                                                   sure.ctypes.data_as(dp), ctypes.c_void_p(stream)))
        return thr, sure

    # -- joint shrinkage across the items and the norms of the groups (include/ndwt.h: ndwt_shrink_joint) --
    def shrink_joint(self, y_ptr, level, thresholds, hard=False, stream=0, band_pitch=0):
        """in-place group thresholding: the group is the coefficients at one position of a band across all items of the plan; one threshold
        per band (num_bands of them, band 0 included; 0 = leave the band alone), all bands in one launch"""
        t, tp = self._thresholds(thresholds)
        self._check_band_count(t, level)
        L.check(L.lib().ndwt_shrink_joint(self._h, y_ptr, int(band_pitch), int(level), tp, int(bool(hard)), ctypes.c_void_p(stream)))

    def denoise_joint(self, x_ptr, out_ptr, level, thresholds, hard=False, stream=0):
        """dec -> shrink_joint -> rec, the coefficients in the plan's scratch"""
        t, tp = self._thresholds(thresholds)
        self._check_band_count(t, level)
        L.check(L.lib().ndwt_denoise_joint(self._h, x_ptr, out_ptr, int(level), tp, int(bool(hard)), ctypes.c_void_p(stream)))

    def group_norms(self, y_ptr, level, stream=0, band_pitch=0):
        """an [nb, 4] array in the columns of band_norms, over the groups of every band: the sum of the groups' magnitudes (the l2,1 norm), the
        sum of their squares, the largest and the count of groups that are not all zero.  Synchronous."""
        out = np.zeros((self._num_bands(level), L.NDWT_NORM_COUNT))
        L.check(L.lib().ndwt_group_norms(self._h, y_ptr, int(band_pitch), int(level), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_void_p(stream)))
        return out

    def group_norms_dev(self, y_ptr, level, out_ptr, stream=0, band_pitch=0):
        """the same into DEVICE memory at out_ptr ([nb, 4] doubles, 8-byte aligned): enqueued on `stream` only"""
        L.check(L.lib().ndwt_group_norms_dev(self._h, y_ptr, int(band_pitch), int(level), out_ptr, ctypes.c_void_p(stream)))

    # -- neighbourhood shrinkage: the energy of a window inside a coefficient's own band decides it (include/ndwt.h: ndwt_shrink_neigh) --
    def shrink_neigh(self, y_ptr, out_ptr, level, thresholds, radius=1, hard=False, stream=0, band_pitch=0):
        """out of place, from y_ptr into out_ptr (the same layout and pitch): a coefficient is scaled by max(1 - t^2 / S, 0), S the sum of
        squares over the periodic window of (2 radius + 1) positions per filtered axis around it, inside its own item of its own band; one
        threshold per band (num_bands of them, band 0 included; 0 = copy the band), all bands in one launch.  out_ptr may be y_ptr one
        band slot down (y_ptr - band pitch) and nothing else that overlaps y_ptr."""
        t, tp = self._thresholds(thresholds)
        self._check_band_count(t, level)
        L.check(L.lib().ndwt_shrink_neigh(self._h, y_ptr, out_ptr, int(band_pitch), int(level), int(radius), tp, int(bool(hard)), ctypes.c_void_p(stream)))

    def denoise_neigh(self, x_ptr, out_ptr, level, thresholds, radius=1, hard=False, stream=0):
        """dec -> shrink_neigh -> rec, the coefficients in the plan's scratch (one band slot more than a transform fills)"""
        t, tp = self._thresholds(thresholds)
        self._check_band_count(t, level)
        L.check(L.lib().ndwt_denoise_neigh(self._h, x_ptr, out_ptr, int(level), int(radius), tp, int(bool(hard)), ctypes.c_void_p(stream)))

    def denoise_host(self, x_ptr, out_ptr, level, threshold, hard=False):
        L.check(L.lib().ndwt_denoise_host(self._h, x_ptr, out_ptr, int(level), float(threshold), int(bool(hard))))

    def dec_split(self, x_re, x_im, y_re, y_im, level, stream=0):
        """split complex (separate re / im device arrays, the mxGetPr / mxGetPi layout); x_im, y_im may be None"""
        L.check(L.lib().ndwt_dec_split(self._h, x_re, x_im, y_re, y_im, int(level), ctypes.c_void_p(stream)))

    def rec_split(self, y_re, y_im, x_re, x_im, level, stream=0):
        L.check(L.lib().ndwt_rec_split(self._h, y_re, y_im, x_re, x_im, int(level), ctypes.c_void_p(stream)))

    def dec_split_host(self, x_re, x_im, y_re, y_im, level):
        L.check(L.lib().ndwt_dec_split_host(self._h, x_re, x_im, y_re, y_im, int(level)))

    def rec_split_host(self, y_re, y_im, x_re, x_im, level):
        L.check(L.lib().ndwt_rec_split_host(self._h, y_re, y_im, x_re, x_im, int(level)))

    def slab_segments(self, add, dsts, srcs, counts, stream=0):
        """up to 8 runs of elements copied (add=False) or added (dst += src) in one launch (include/ndwt.h: ndwt_slab_segments)"""
        n = len(dsts)
        L.check(L.lib().ndwt_slab_segments(self._h, 1 if add else 0, n, (ctypes.c_void_p * n)(*dsts), (ctypes.c_void_p * n)(*srcs),
                                           (ctypes.c_int64 * n)(*counts), ctypes.c_void_p(stream)))

    def slab_segments_strided(self, add, dsts, srcs, counts, nrep, dst_strides, src_strides, stream=0):
        """up to 8 runs, each repeated `nrep` times (repetition r at r * stride, per run and side), copied or added in one launch
        (include/ndwt.h: ndwt_slab_segments_strided); counts and strides in scalars"""
        n = len(dsts)
        L.check(L.lib().ndwt_slab_segments_strided(self._h, 1 if add else 0, n, (ctypes.c_void_p * n)(*dsts), (ctypes.c_void_p * n)(*srcs),
                                                   (ctypes.c_int64 * n)(*counts), int(nrep), (ctypes.c_int64 * n)(*dst_strides),
                                                   (ctypes.c_int64 * n)(*src_strides), ctypes.c_void_p(stream)))

    def release_staging(self):
        L.check(L.lib().ndwt_plan_release_staging(self._h))

    def slab_halo(self, stride=1):
        v = [ctypes.c_int64(0) for _ in range(4)]
        L.check(L.lib().ndwt_slab_halo(self._h, int(stride), *[ctypes.byref(t) for t in v]))
        return tuple(t.value for t in v)   # (ana_before, ana_after, syn_before, syn_after)

    def analysis_level_slab(self, in_ptr, out_ptrs, stride=1, stream=0):
        arr = (ctypes.c_void_p * len(out_ptrs))(*out_ptrs)
        L.check(L.lib().ndwt_analysis_level_slab(self._h, in_ptr, arr, int(stride), ctypes.c_void_p(stream)))

    def analysis_level_slab_split(self, in_ptr, halo_before_ptr, halo_after_ptr, out_ptrs, stride=1, stream=0):
        arr = (ctypes.c_void_p * len(out_ptrs))(*out_ptrs)
        L.check(L.lib().ndwt_analysis_level_slab_split(self._h, in_ptr, halo_before_ptr, halo_after_ptr, arr, int(stride),
                                                       ctypes.c_void_p(stream)))

    def synthesis_level_slab_ext(self, in_ptrs, out_ext_ptr, stride=1, stream=0):
        arr = (ctypes.c_void_p * len(in_ptrs))(*in_ptrs)
        L.check(L.lib().ndwt_synthesis_level_slab_ext(self._h, arr, out_ext_ptr, int(stride), ctypes.c_void_p(stream)))

    def analysis_level_slab_part(self, in_ptr, halo_before_ptr, halo_after_ptr, out_ptrs, n_planes, stride=1, stream=0):
        arr = (ctypes.c_void_p * len(out_ptrs))(*out_ptrs)
        L.check(L.lib().ndwt_analysis_level_slab_part(self._h, in_ptr, halo_before_ptr, halo_after_ptr, arr, int(stride),
                                                      int(n_planes), ctypes.c_void_p(stream)))

    def synthesis_level_slab_part(self, in_ptrs, n_in, e0, n_out, out_ptr, stride=1, stream=0):
        arr = (ctypes.c_void_p * len(in_ptrs))(*in_ptrs)
        L.check(L.lib().ndwt_synthesis_level_slab_part(self._h, arr, int(n_in), int(e0), int(n_out), out_ptr, int(stride),
                                                       ctypes.c_void_p(stream)))

    def analysis_level_slab_runs(self, in_ptr, out_ptrs, n_planes, n_runs, run_stride, stride=1, stream=0):
        arr = (ctypes.c_void_p * len(out_ptrs))(*out_ptrs)
        L.check(L.lib().ndwt_analysis_level_slab_runs(self._h, in_ptr, arr, int(stride), int(n_planes), int(n_runs), int(run_stride),
                                                      ctypes.c_void_p(stream)))

    def synthesis_level_slab_runs(self, in_ptrs, n_in, e0, e_stride, n_runs, n_out, out_ptr, stride=1, stream=0):
        arr = (ctypes.c_void_p * len(in_ptrs))(*in_ptrs)
        L.check(L.lib().ndwt_synthesis_level_slab_runs(self._h, arr, int(n_in), int(e0), int(e_stride), int(n_runs), int(n_out),
                                                       out_ptr, int(stride), ctypes.c_void_p(stream)))

    def synthesis_level_slab(self, in_ptrs, out_ptr, stride=1, stream=0):
        arr = (ctypes.c_void_p * len(in_ptrs))(*in_ptrs)
        L.check(L.lib().ndwt_synthesis_level_slab(self._h, arr, out_ptr, int(stride), ctypes.c_void_p(stream)))


def neigh_threshold_row(sigma, gains, sizes, radius=1, rule="universal"):
    """Host arithmetic of _NdDwtBase.neigh_thresholds: sigma the noise of the signal, gains the band gains, sizes the filtered axes of one
    item.  A row of len(gains) thresholds, entry 0 zero."""
    if rule not in ("universal", "wiener", "block"):
        raise ValueError("rule must be 'universal', 'wiener' or 'block'")
    if int(radius) not in (1, 2, 3):
        raise ValueError("radius must be 1, 2 or 3")
    s = float(sigma) * np.asarray(gains, dtype=np.float64)
    N = float(np.prod(np.atleast_1d(sizes), dtype=np.float64))
    M = float((2 * int(radius) + 1) ** len(np.atleast_1d(sizes)))
    k = np.sqrt(2.0 * np.log(N)) if rule == "universal" else np.sqrt(M) if rule == "wiener" else np.sqrt(4.50524 * M)
    thr = k * s
    thr[0] = 0.0
    return thr


class Coefficients:
    """Device-resident coefficients behind an opaque handle (include/ndwt.h: ndwt_coef_*): what the MATLAB gateway's `dec_keep` /
    `rec_handle` commands hold between calls -- only the signal crosses PCIe (the reference's gateway moves the whole coefficient
    array through host memory per call, nd_dwt_3D.m:161,225).  Host arrays are numpy, kernel order ((bands,) nd, ..., n1)."""

    def __init__(self, plan: Plan, handle: ctypes.c_void_p):
        self.plan, self._h = plan, handle

    @classmethod
    def dec(cls, plan: Plan, x: np.ndarray, level: int, reuse: "Coefficients | None" = None):
        h = reuse._h if reuse is not None else ctypes.c_void_p(None)
        x = np.ascontiguousarray(x)
        L.check(L.lib().ndwt_coef_dec_host(plan._h, x.ctypes.data_as(ctypes.c_void_p), int(level), ctypes.byref(h)))
        return reuse if reuse is not None else cls(plan, h)

    @classmethod
    def put(cls, plan: Plan, y: np.ndarray, level: int):
        h = ctypes.c_void_p(None)
        y = np.ascontiguousarray(y)
        L.check(L.lib().ndwt_coef_put_host(plan._h, int(level), y.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)))
        return cls(plan, h)

    def info(self):
        lev, nb, pitch, ptr = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_void_p(None)
        L.check(L.lib().ndwt_coef_info(self._h, ctypes.byref(lev), ctypes.byref(nb), ctypes.byref(pitch), ctypes.byref(ptr)))
        return {"level": lev.value, "bands": nb.value, "band_pitch": pitch.value, "dev_ptr": ptr.value}

    def rec(self, out: np.ndarray):
        assert out.flags.c_contiguous
        L.check(L.lib().ndwt_coef_rec_host(self.plan._h, self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def shrink(self, threshold, hard=False):
        L.check(L.lib().ndwt_coef_shrink(self.plan._h, self._h, float(threshold), int(bool(hard))))
        return self

    def get(self, out: np.ndarray):
        assert out.flags.c_contiguous
        L.check(L.lib().ndwt_coef_get_host(self.plan._h, self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def release(self):
        if self._h is not None and self._h.value:
            L.lib().ndwt_coef_release(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class MultiPlan:
    """Single-process multi-device plan (include/ndwt.h, ndwt_mplan_*): ONE host thread drives the listed devices; the volume is
    sharded in slabs on its outermost axis (a device listed twice holds two slabs).  Host arrays in kernel order
    ((bands,) nd, ..., n1, contiguous) in and out -- the path behind the MATLAB gateway, where the host is one process."""

    def __init__(self, dims, wnames, dtype, devices, complex_interleaved=False, pres_l2_norm=False, dilation="reference", max_level=3,
                 shard_axis=None):
        """shard_axis: None = the outermost axis; 2 of a 4-D volume = z-slabs (t whole on every slab; slab tensors (nt, nz_i, ny, nx))"""
        self.dims = [int(d) for d in dims]
        self.ndim = len(self.dims)
        self.shard_axis = self.ndim - 1 if shard_axis is None else int(shard_axis)
        self.np_dtype = np.float32 if dtype in (torch.float32, np.float32, "single") else np.float64
        self.complex = bool(complex_interleaved)
        self.max_level = int(max_level)
        self._h = ctypes.c_void_p(None)
        dims_c = (ctypes.c_int64 * self.ndim)(*self.dims)
        names_c = (ctypes.c_char_p * self.ndim)(*[w.encode() for w in wnames])
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        dt = L.NDWT_F32 if self.np_dtype == np.float32 else L.NDWT_F64
        dil = {"reference": L.NDWT_DILATION_REFERENCE, "atrous": L.NDWT_DILATION_ATROUS}[dilation]
        if shard_axis is None:
            L.mcheck(L.lib().ndwt_mplan_create(ctypes.byref(self._h), self.ndim, dims_c, names_c, dt,
                                               L.NDWT_COMPLEX_INTERLEAVED if self.complex else L.NDWT_REAL, int(bool(pres_l2_norm)), dil,
                                               self.max_level, devs, len(devices)))
        else:
            L.mcheck(L.lib().ndwt_mplan_create_axis(ctypes.byref(self._h), self.ndim, dims_c, names_c, dt,
                                                    L.NDWT_COMPLEX_INTERLEAVED if self.complex else L.NDWT_REAL, int(bool(pres_l2_norm)), dil,
                                                    self.max_level, devs, len(devices), self.shard_axis))

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                L.lib().ndwt_mplan_destroy(self._h)
                self._h = ctypes.c_void_p(None)
        except Exception:
            pass

    def slabs(self):
        out = []
        for i in range(L.lib().ndwt_mplan_num_slabs(self._h)):
            d, z0, n = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
            L.mcheck(L.lib().ndwt_mplan_slab(self._h, i, ctypes.byref(d), ctypes.byref(z0), ctypes.byref(n)))
            out.append((d.value, z0.value, n.value))
        return out

    def _check(self, a, bands):
        cdt = {np.float32: np.complex64, np.float64: np.complex128}[self.np_dtype] if self.complex else self.np_dtype
        shape = ((bands,) if bands else ()) + tuple(reversed(self.dims))
        if not (isinstance(a, np.ndarray) and a.dtype == cdt and a.flags.c_contiguous and a.shape == shape):
            raise ValueError(f"expected a C-contiguous {np.dtype(cdt).name} array of shape {shape}")

    def dec(self, x, level):
        """x: numpy (nd, ..., n1) -> numpy (bands, nd, ..., n1)"""
        self._check(x, 0)
        y = np.empty((num_bands(self.ndim, level),) + x.shape, dtype=x.dtype)
        L.mcheck(L.lib().ndwt_mdec_host(self._h, x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), int(level)))
        return y

    def rec(self, y):
        level = L.lib().ndwt_level_from_bands(self.ndim, int(y.shape[0]))
        if level < 1:
            raise ValueError(f"{y.shape[0]} bands is not a valid {self.ndim}-D coefficient count")
        self._check(y, y.shape[0])
        x = np.empty(y.shape[1:], dtype=y.dtype)
        L.mcheck(L.lib().ndwt_mrec_host(self._h, y.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p), level))
        return x

    def set_exchange(self, scheme):
        """'scatter' (default: one band of partial sums per level; equal to one device to rounding) or 'gather' (bit-identical)"""
        L.mcheck(L.lib().ndwt_mplan_set_exchange(self._h, {"scatter": 0, "gather": 1}[scheme]))
        return self

    def set_overlap(self, on):
        """True (default): copies between slabs on their own streams, overlapped with the launches that do not wait for them"""
        L.mcheck(L.lib().ndwt_mplan_set_overlap(self._h, int(on)))
        return self

    def set_threads(self, on):
        """True (default): one host thread per slab queues that slab's work; False: the calling thread queues everything.  Same results."""
        L.mcheck(L.lib().ndwt_mplan_set_threads(self._h, int(bool(on))))
        return self

    def describe(self) -> str:
        buf = ctypes.create_string_buffer(512)
        L.mcheck(L.lib().ndwt_mplan_describe(self._h, buf, 512))
        return buf.value.decode()

    def _slab_tensors(self, tensors, bands):
        sl = self.slabs()
        tdt = {np.float32: torch.float32, np.float64: torch.float64}[self.np_dtype]
        if self.complex:
            tdt = {torch.float32: torch.complex64, torch.float64: torch.complex128}[tdt]
        if len(tensors) != len(sl):
            raise ValueError(f"{len(sl)} slab tensors expected")
        for t, (dev, _, n) in zip(tensors, sl):
            local = list(self.dims)
            local[self.shard_axis] = n
            shape = ((bands,) if bands else ()) + tuple(reversed(local))
            if not (t.is_cuda and t.device.index == dev and t.dtype == tdt and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f"slab tensor: contiguous {tdt} of shape {shape} on cuda:{dev} expected")
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def dec_device(self, x_slabs, level):
        """device-resident form: x_slabs[i] = torch tensor (n_i, ..., n1) on slab i's device -> list of (bands, n_i, ..., n1) tensors
        (z-slabs: (nt, nz_i, ny, nx) -> (bands, nt, nz_i, ny, nx)).
        Ordered against torch by host synchronisation: every slab device is synchronised before the call; returns when the result is."""
        xs = self._slab_tensors(x_slabs, 0)
        nbt = num_bands(self.ndim, level)
        ys = [torch.empty((nbt,) + tuple(t.shape), dtype=t.dtype, device=t.device) for t in x_slabs]
        self._sync(x_slabs)
        L.mcheck(L.lib().ndwt_mdec(self._h, xs, self._slab_tensors(ys, nbt), int(level)))
        return ys

    @staticmethod
    def _sync(tensors):
        """The plan's private streams are ordered against torch by HOST synchronisation only: the inputs must be complete, and the output
        tensors just allocated may be blocks the caching allocator recycled from tensors whose kernels are still queued on a torch
        stream -- every slab device is synchronised before the plan's streams touch them."""
        for dev in sorted({t.device.index for t in tensors}):
            torch.cuda.synchronize(dev)

    def rec_device(self, y_slabs):
        nbt = int(y_slabs[0].shape[0])
        level = L.lib().ndwt_level_from_bands(self.ndim, nbt)
        if level < 1:
            raise ValueError(f"{nbt} bands is not a valid {self.ndim}-D coefficient count")
        ys = self._slab_tensors(y_slabs, nbt)
        xs = [torch.empty(tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in y_slabs]
        self._sync(y_slabs)
        L.mcheck(L.lib().ndwt_mrec(self._h, ys, self._slab_tensors(xs, 0), level))
        return xs


def num_bands(ndim, level):
    return int(L.lib().ndwt_num_bands(int(ndim), int(level)))


def _current_stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class _NdDwtBase:
    """Common implementation of nd_dwt_{1,2,3,4}D (reference files cited per method)."""

    NDIM = 0

    def __init__(self, wname, sizes, *varargin, **kwargs):
        d = self.NDIM
        sizes = [int(s) for s in np.atleast_1d(sizes)]
        self._check_sizes(sizes)
        self.sizes = sizes
        self.wname = self._check_wname(wname)
        # defaults: nd_dwt_3D.m:101-103 (compute defaults to the HIP engine here)
        self.pres_l2_norm = 0
        self.precision = "double"
        self.compute = "hip"
        self.dilation = "reference"
        self.device = None
        self.devices = None
        self.band_pitch = "packed"
        self.batch = None
        self.stack = None
        self.inner = None
        # name/value pairs as in MATLAB (nd_dwt_3D.m:105-120); keyword arguments are accepted too
        if len(varargin) % 2:
            raise ValueError("Optional inputs must come in pairs")
        opts = [(varargin[i], varargin[i + 1]) for i in range(0, len(varargin), 2)] + list(kwargs.items())
        for ind, (key, val) in enumerate(opts):
            k = str(key).lower()
            if k == "pres_l2_norm":
                self.pres_l2_norm = int(bool(val))
            elif k == "compute":
                self.compute = str(val)
            elif k == "precision":
                self.precision = str(val)
            elif k == "dilation":
                self.dilation = str(val).lower()
            elif k == "device":
                self.device = val
            elif k == "band_pitch":                # 'packed' (reference layout) | 'auto' | elements between bands of dec()'s result
                self.band_pitch = val if isinstance(val, str) else int(val)
            elif k == "batch":                     # nd_dwt_1D only: this many signals per call, x = [n, batch] (column k = signal k)
                self.batch = int(val)
            elif k == "stack":                     # nd_dwt_2D / nd_dwt_3D: this many images / volumes per call, x = [sizes, stack]
                self.stack = int(val)
            elif k == "inner":                     # nd_dwt_1D / 2D / 3D: each sample is this many elements (a number or a list of sizes) lying
                self.inner = [int(v) for v in np.atleast_1d(val)]   # together: x = [inner.., sizes, (batch | stack)]
            elif k == "devices":                   # shard the outermost axis over these devices (host arrays, one process)
                self.devices = [int(v) for v in np.atleast_1d(val)]
            else:   # unknown keys only warn (nd_dwt_3D.m:118)
                warnings.warn(f"Unknown optional input #{2 * ind + 1} ingoring!")
        if self.compute.lower() == "mex" and self.precision.lower() == "single":   # nd_dwt_3D.m:122-124
            raise ValueError("Single precsision is not currently supported for mex computation")
        c = self.compute.lower()
        if c in ("hip", "gpu"):
            self._offload = False
        elif c in ("hip_off", "gpu_off", "mat", "mex"):
            self._offload = True
        else:
            raise ValueError(f"unknown compute '{self.compute}'")
        if self.precision.lower() not in ("double", "single"):
            raise ValueError("precision must be 'double' or 'single'")
        if self.dilation not in ("reference", "atrous"):
            raise ValueError("dilation must be 'reference' or 'atrous'")
        if isinstance(self.band_pitch, str) and self.band_pitch.lower() not in ("packed", "auto"):
            raise ValueError("band_pitch must be 'packed', 'auto' or a number of elements")
        if self.band_pitch != "packed" and self._offload:
            raise ValueError("'band_pitch' lays out device tensors: use compute='hip'")
        if self.devices is not None and (not self._offload or d < 2):
            raise ValueError("'devices' shards host arrays of 2-D .. 4-D transforms: use compute='hip_off'")
        if self.batch is not None:
            if d != 1:
                raise ValueError("'batch' is an option of nd_dwt_1D: the other classes transform one array per call")
            if self.devices is not None:
                raise ValueError("'batch' and 'devices' do not combine: a batched plan lives on one device")
            if self.batch < 1:
                raise ValueError("'batch' must be a number of signals >= 1")
        if self.stack is not None:
            if d == 1:
                raise ValueError("'stack' is an option of nd_dwt_2D and nd_dwt_3D: many signals per call are nd_dwt_1D's 'batch'")
            if d == 4:
                raise ValueError("'stack' is an option of nd_dwt_2D and nd_dwt_3D: a stack of 4-D arrays is not supported")
            if self.devices is not None:
                raise ValueError("'stack' and 'devices' do not combine: a stack plan lives on one device")
            if self.stack < 1:
                raise ValueError("'stack' must be a number of items >= 1")
        if self.inner is not None:
            if d == 4:
                raise ValueError("'inner' is an option of nd_dwt_1D, nd_dwt_2D and nd_dwt_3D: interleaved samples of 4-D arrays are not supported")
            if self.devices is not None:
                raise ValueError("'inner' and 'devices' do not combine: a plan over interleaved samples lives on one device")
            if len(self.inner) < 1 or any(v < 1 for v in self.inner):
                raise ValueError("'inner' must be a number of elements >= 1, or a list of such sizes")
        # the shape of x in MATLAB terms: `sizes`, for a batched 1-D object [n, batch], for a stack [sizes, stack]; with 'inner' its sizes
        # come first: [inner.., sizes, (batch | stack)]
        self._shape = (self.inner or []) + sizes + ([self.batch] if self.batch is not None else []) + ([self.stack] if self.stack is not None else [])
        # get_filters (nd_dwt_3D.m:263-342): per-axis taps instead of N-D FFT-domain kernels
        self.f_dec = [L.wave_filters(w) for w in self.wname[:d]]
        self.f_size = {f"s{a + 1}": len(self.f_dec[a][0]) for a in range(d)}
        for a in range(d):
            if self.f_size[f"s{a + 1}"] > sizes[a]:   # nd_dwt_3D.m:277-286
                raise ValueError(f"{_ORD[a]} Dimension of Data is shorter than the wavelet filter being used")
        self._plans = {}

    # -- per-dimension validation (messages of the reference) --
    def _check_sizes(self, sizes):
        raise NotImplementedError

    def _check_wname(self, wname):
        raise NotImplementedError

    def _level_from_bands(self, n):
        raise NotImplementedError

    # -- plumbing --
    def _torch_dtype(self, is_complex):
        single = self.precision.lower() == "single"
        if is_complex:
            return torch.complex64 if single else torch.complex128
        return torch.float32 if single else torch.float64

    def _dev(self, x=None):
        if self.device is not None:
            return torch.device(self.device)
        if x is not None and isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
        return torch.device("cuda", torch.cuda.current_device())

    def _plan(self, is_complex, level, dev):
        # ONE plan per (data kind, device): a plan owns scratch (GBs for large volumes) and serves one stream at a time
        # (include/ndwt.h).  A call on another torch stream than the plan's previous one first makes the new stream wait for
        # everything queued on the old one, so the scratch is never shared by two streams in flight and nothing accumulates per stream.
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        key = (is_complex, idx)
        p = self._plans.get(key)
        if p is None or p.max_level < level:
            real_dt = torch.float32 if self.precision.lower() == "single" else torch.float64
            if p is not None:
                torch.cuda.synchronize(idx)                           # the plan being replaced may still be running
            if self.inner is not None:                                # interleaved samples: every filtered axis is strided
                p = Plan(self.sizes, self.wname[: self.NDIM], real_dt, is_complex, self.pres_l2_norm, self.dilation, max_level=max(level, 3),
                         device=idx, inner=int(np.prod(self.inner, dtype=np.int64)), howmany=self.batch or self.stack or 1)
            elif self.stack is not None:                              # the whole array, its leading axes filtered
                p = Plan(self.sizes + [self.stack], self.wname[: self.NDIM] + [None], real_dt, is_complex, self.pres_l2_norm,
                         self.dilation, max_level=max(level, 3), device=idx, axes=tuple(range(self.NDIM)))
            else:
                p = Plan(self.sizes, self.wname[: self.NDIM], real_dt, is_complex, self.pres_l2_norm, self.dilation,
                         max_level=max(level, 3), device=idx, howmany=self.batch)
            p._last_stream = None
            self._plans[key] = p
        cur = torch.cuda.current_stream(torch.device("cuda", idx))
        if p._last_stream is not None and p._last_stream != cur:
            cur.wait_event(p._last_stream.record_event())
        p._last_stream = cur
        return p

    def _to_device_kernel_order(self, x, dev, ndim_expected):
        """user array (MATLAB shape) -> contiguous tensor in kernel order (reversed dims) on `dev`."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(np.transpose(x)))     # kernel order on the host
            kernel_order = True
        else:
            kernel_order = False
        if not isinstance(x, torch.Tensor):
            raise TypeError("x must be a torch.Tensor or numpy.ndarray")
        if not self._offload and not x.is_cuda:
            raise ValueError("compute='hip' expects tensors on the GPU (use compute='hip_off' for host arrays)")
        if not kernel_order:
            x = x.permute(*reversed(range(x.dim())))
        dt = self._torch_dtype(x.is_complex())
        return x.to(device=dev, dtype=dt).contiguous()

    def _from_device(self, t_kernel, like_numpy, dev_in):
        out = t_kernel.permute(*reversed(range(t_kernel.dim())))            # MATLAB shape, column-major memory
        if self._offload:
            out = out.cpu()
            if like_numpy:
                return out.numpy()
        return out

    # -- nd_dwt_3D.m:142-199 --
    def dec(self, x, level):
        level = int(level)
        if level < 1:
            raise ValueError("level must be >= 1")
        like_numpy = isinstance(x, np.ndarray)
        x = self._prep_dec_input(x)
        if list(x.shape) != self._shape:
            raise ValueError(f"input size {list(x.shape)} does not match the object's sizes {self._shape}")
        if self.devices is not None:
            return self._multi(x, level, None)
        dev = self._dev(x if isinstance(x, torch.Tensor) else None)
        xk = self._to_device_kernel_order(x, dev, self.NDIM)
        is_c = xk.is_complex()
        plan = self._plan(is_c, level, dev)
        nb = num_bands(self.NDIM, level)
        vol = int(np.prod(xk.shape))
        pitch = self._pitch(plan, vol)
        if pitch:
            # a pitched coefficient tensor: same shape and indexing, band b at b * pitch elements (a view of one allocation);
            # .contiguous() gives the packed reference layout
            flat = torch.empty(nb * pitch, dtype=xk.dtype, device=dev)
            cs = [1] * xk.dim()
            for i in range(xk.dim() - 2, -1, -1):
                cs[i] = cs[i + 1] * int(xk.shape[i + 1])
            yk = flat.as_strided((nb,) + tuple(xk.shape), (pitch,) + tuple(cs))
        else:
            yk = torch.empty((nb,) + tuple(xk.shape), dtype=xk.dtype, device=dev)
        with torch.cuda.device(dev):
            plan.dec(xk.data_ptr(), yk.data_ptr(), level, _current_stream(dev), band_pitch=pitch)
        return self._from_device(yk, like_numpy, dev)   # real in -> real out (nd_dwt_3D.m:189-192) by construction

    def _pitch(self, plan, vol):
        if self.band_pitch == "packed":
            return 0
        if isinstance(self.band_pitch, str):
            return plan.band_pitch()
        if self.band_pitch < vol:
            raise ValueError(f"band_pitch {self.band_pitch} is smaller than a band ({vol} elements)")
        return 0 if self.band_pitch == vol else int(self.band_pitch)

    def _coef_kernel_order(self, y, dev):
        """coefficient array (MATLAB shape [dims, bands]) -> (tensor in kernel order, band pitch): a device tensor whose bands are
        each contiguous and evenly spaced (what dec() returns, packed or pitched) is used where it lies"""
        if isinstance(y, torch.Tensor) and y.is_cuda and y.device == dev and y.dtype == self._torch_dtype(y.is_complex()):
            yk = y.permute(*reversed(range(y.dim())))
            if yk[0].is_contiguous() and yk.shape[0] > 1 and yk.stride(0) > yk[0].numel():
                return yk, int(yk.stride(0))
        return self._to_device_kernel_order(y, dev, self.NDIM + 1), 0

    # -- nd_dwt_3D.m:202-256 --
    def rec(self, y):
        like_numpy = isinstance(y, np.ndarray)
        if y.ndim != len(self._shape) + 1 or list(y.shape[:-1]) != self._shape:
            raise ValueError(f"coefficient array must have shape {self._shape + ['bands']}")
        level = self._level_from_bands(int(y.shape[-1]))
        if num_bands(self.NDIM, level) != int(y.shape[-1]):
            raise ValueError(f"{int(y.shape[-1])} bands is not a valid {self.NDIM}-D coefficient count")
        if self.devices is not None:
            return self._multi(y, level, "rec")
        dev = self._dev(y if isinstance(y, torch.Tensor) else None)
        yk, pitch = self._coef_kernel_order(y, dev)
        plan = self._plan(yk.is_complex(), level, dev)
        xk = torch.empty(tuple(yk.shape[1:]), dtype=yk.dtype, device=dev)
        with torch.cuda.device(dev):
            plan.rec(yk.data_ptr(), xk.data_ptr(), level, _current_stream(dev), band_pitch=pitch)
        return self._from_device(xk, like_numpy, dev)

    # -- consumers for iterative solvers (extension; not in the reference) --
    def shrink(self, y, threshold, mode="soft", joint=False):
        """Soft / hard thresholding of every detail band of a coefficient array (band 0, the coarsest approximation,
        is kept); complex data: the magnitude is shrunk.  Returns a new array of the same kind as `y`.
        joint=True: the K signals of a batch / items of a stack are thresholded together -- the magnitude compared and shrunk is that of
        the group of K coefficients at one position (group soft thresholding, the prox of the l2,1 norm); a scalar threshold: every
        detail band, band 0 kept; a sequence: one threshold per band."""
        if mode not in ("soft", "hard"):
            raise ValueError("mode must be 'soft' or 'hard'")
        like_numpy = isinstance(y, np.ndarray)
        if y.ndim != len(self._shape) + 1 or list(y.shape[:-1]) != self._shape:
            raise ValueError(f"coefficient array must have shape {self._shape + ['bands']}")
        level = self._level_from_bands(int(y.shape[-1]))
        thr = self._joint_thresholds(threshold, level) if joint else self._band_thresholds(threshold, level)
        dev = self._dev(y if isinstance(y, torch.Tensor) else None)
        yk, pitch = self._coef_kernel_order(y, dev)
        if isinstance(y, torch.Tensor) and yk.data_ptr() == y.data_ptr():
            if pitch:                                          # never modify the caller's array: copy, keeping the pitch
                flat = torch.empty(yk.shape[0] * pitch, dtype=yk.dtype, device=dev)
                cp = flat.as_strided(tuple(yk.shape), tuple(yk.stride()))
                cp.copy_(yk)
                yk = cp
            else:
                yk = yk.clone()
        plan = self._plan(yk.is_complex(), level, dev)
        with torch.cuda.device(dev):
            if joint:
                plan.shrink_joint(yk.data_ptr(), level, thr, mode == "hard", _current_stream(dev), band_pitch=pitch)
            elif thr is None:
                plan.shrink(yk.data_ptr(), level, threshold, mode == "hard", _current_stream(dev), band_pitch=pitch)
            elif thr.ndim == 2:
                plan.shrink_bands_items(yk.data_ptr(), level, thr, mode == "hard", _current_stream(dev), band_pitch=pitch)
            else:
                plan.shrink_bands(yk.data_ptr(), level, thr, mode == "hard", _current_stream(dev), band_pitch=pitch)
        return self._from_device(yk, like_numpy, dev)

    def denoise(self, x, level, threshold, mode="soft", joint=False):
        """rec(shrink(dec(x, level), threshold)) in one call: the coefficients stay in a scratch array of the plan.  joint: as shrink's."""
        if mode not in ("soft", "hard"):
            raise ValueError("mode must be 'soft' or 'hard'")
        level = int(level)
        if level < 1:
            raise ValueError("level must be >= 1")
        thr = self._joint_thresholds(threshold, level) if joint else self._band_thresholds(threshold, level)
        like_numpy = isinstance(x, np.ndarray)
        x = self._prep_dec_input(x)
        if list(x.shape) != self._shape:
            raise ValueError(f"input size {list(x.shape)} does not match the object's sizes {self._shape}")
        dev = self._dev(x if isinstance(x, torch.Tensor) else None)
        xk = self._to_device_kernel_order(x, dev, self.NDIM)
        plan = self._plan(xk.is_complex(), level, dev)
        out = torch.empty_like(xk)
        with torch.cuda.device(dev):
            if joint:
                plan.denoise_joint(xk.data_ptr(), out.data_ptr(), level, thr, mode == "hard", _current_stream(dev))
            elif thr is None:
                plan.denoise(xk.data_ptr(), out.data_ptr(), level, threshold, mode == "hard", _current_stream(dev))
            elif thr.ndim == 2:
                plan.denoise_bands_items(xk.data_ptr(), out.data_ptr(), level, thr, mode == "hard", _current_stream(dev))
            else:
                plan.denoise_bands(xk.data_ptr(), out.data_ptr(), level, thr, mode == "hard", _current_stream(dev))
        return self._from_device(out, like_numpy, dev)

    # -- neighbourhood shrinkage (extension; not in the reference): NeighShrink, NeighBlock / NeighCoeff, the local Wiener rule --
    def shrink_neigh(self, y, threshold, radius=1, mode="soft"):
        """Thresholding by the energy of a coefficient's neighbourhood: with S the sum of |c|^2 over the periodic window of 2 radius + 1
        positions per filtered axis around a coefficient -- inside its own band, and its own signal of a batch / item of a stack -- the
        coefficient becomes c * max(1 - t^2 / S, 0) (mode 'hard': c where S > t^2, else 0).  threshold: a scalar for every detail band
        (band 0 kept), or one value per band (0 = the band is kept); neigh_thresholds gives the usual rules.  radius: 1, 2 or 3.
        Returns a new array of the same kind as `y`; `y` is only read."""
        if mode not in ("soft", "hard"):
            raise ValueError("mode must be 'soft' or 'hard'")
        like_numpy = isinstance(y, np.ndarray)
        if y.ndim != len(self._shape) + 1 or list(y.shape[:-1]) != self._shape:
            raise ValueError(f"coefficient array must have shape {self._shape + ['bands']}")
        level = self._level_from_bands(int(y.shape[-1]))
        thr = self._joint_thresholds(threshold, level)
        dev = self._dev(y if isinstance(y, torch.Tensor) else None)
        yk, pitch = self._coef_kernel_order(y, dev)
        if pitch:                                              # the result keeps the pitch of the array it came from
            flat = torch.empty(yk.shape[0] * pitch, dtype=yk.dtype, device=dev)
            out = flat.as_strided(tuple(yk.shape), tuple(yk.stride()))
        else:
            out = torch.empty_like(yk)
        plan = self._plan(yk.is_complex(), level, dev)
        with torch.cuda.device(dev):
            plan.shrink_neigh(yk.data_ptr(), out.data_ptr(), level, thr, int(radius), mode == "hard", _current_stream(dev), band_pitch=pitch)
        return self._from_device(out, like_numpy, dev)

    def denoise_neigh(self, x, level, threshold, radius=1, mode="soft"):
        """rec(shrink_neigh(dec(x, level), threshold, radius)) in one call: the coefficients stay in a scratch array of the plan"""
        if mode not in ("soft", "hard"):
            raise ValueError("mode must be 'soft' or 'hard'")
        level = int(level)
        if level < 1:
            raise ValueError("level must be >= 1")
        thr = self._joint_thresholds(threshold, level)
        like_numpy = isinstance(x, np.ndarray)
        x = self._prep_dec_input(x)
        if list(x.shape) != self._shape:
            raise ValueError(f"input size {list(x.shape)} does not match the object's sizes {self._shape}")
        dev = self._dev(x if isinstance(x, torch.Tensor) else None)
        xk = self._to_device_kernel_order(x, dev, self.NDIM)
        plan = self._plan(xk.is_complex(), level, dev)
        out = torch.empty_like(xk)
        with torch.cuda.device(dev):
            plan.denoise_neigh(xk.data_ptr(), out.data_ptr(), level, thr, int(radius), mode == "hard", _current_stream(dev))
        return self._from_device(out, like_numpy, dev)

    def neigh_thresholds(self, x, level, radius=1, rule="universal"):
        """The thresholds of shrink_neigh / denoise_neigh for the usual rules, one per band, entry 0 (the approximation) 0.  With s_b =
        estimate_sigma(x) * band_gains(level)[b], N = the samples of one item's filtered axes and M = (2 radius + 1)^dimensions:
          'universal'  t_b = s_b sqrt(2 ln N): NeighShrink (Chen, Bui and Krzyzak)
          'wiener'     t_b^2 = M s_b^2: the locally adaptive Wiener estimate c * max(S / M - s_b^2, 0) / (S / M) (Mihcak et al.)
          'block'      t_b^2 = 4.50524 M s_b^2: Cai and Silverman's constant for NeighBlock / NeighCoeff, the root of l - ln l = 3"""
        return neigh_threshold_row(self.estimate_sigma(x), self.band_gains(int(level)), self.sizes, radius, rule)

    def _band_thresholds(self, threshold, level):
        """None for a scalar threshold (today's call), else the sequence as an array of one threshold per band; a [K, bands] array of a
        batch or stack of K > 1 items stays 2-D: a row of thresholds per item (Plan.shrink_bands_items / denoise_bands_items)"""
        if np.ndim(threshold) == 0:
            return None
        if isinstance(threshold, torch.Tensor):
            threshold = threshold.detach().cpu().numpy()
        thr = np.asarray(threshold, dtype=np.float64)
        nb = num_bands(self.NDIM, level)
        if thr.ndim == 2 and self._items > 1 and thr.shape == (self._items, nb):
            return np.ascontiguousarray(thr)
        if thr.size != nb:
            per_item = f", or a [{self._items}, {nb}] array, one row per item" if self._items > 1 else ""
            raise ValueError(f"threshold must be a scalar or {nb} values, one per band of a {level}-level transform{per_item} (got shape {list(thr.shape)})")
        return thr.reshape(-1)

    def _joint_thresholds(self, threshold, level):
        """the thresholds of a joint call, one per band: a scalar for every detail band with band 0 kept, or the sequence; a row per item
        has no meaning there"""
        nb = num_bands(self.NDIM, level)
        if np.ndim(threshold) == 0:
            thr = np.full(nb, float(threshold))
            thr[0] = 0.0
            return thr
        thr = self._band_thresholds(threshold, level)
        if thr.ndim == 2:
            raise ValueError(f"joint=True takes a scalar or {nb} thresholds, one per band: the items of a group share one (got shape {list(thr.shape)})")
        return thr

    @property
    def _items(self):
        """K: the signals of a batch or the items of a stack (1 without either)"""
        return int(self.batch or self.stack or 1)

    def band_gains(self, level):
        """standard deviation of every band for unit-variance white input (ndwt_band_gains): thresholds = k * sigma * band_gains(level)"""
        return L.band_gains(self.sizes, self.wname[: self.NDIM], int(level), self.pres_l2_norm, self.dilation)

    # -- the sigma of thresholds = k * sigma * band_gains(level), estimated on the device (extension; not in the reference) --
    def estimate_sigma(self, x, per_item=False):
        """Standard deviation of white noise in the signal `x` (Donoho and Johnstone): the median of |c| over the finest all-high-pass
        band of a level-1 dec, / 0.6745 and / that band's gain; complex x: / 1.1774, the sigma of each of the real and imaginary parts.
        The band is the whole array (all signals of a batch, all items of a stack).  A float; the call waits for the result.
        per_item=True: one estimate per signal of the batch / item of the stack, a length-K array."""
        x = self._prep_dec_input(x)
        if list(x.shape) != self._shape:
            raise ValueError(f"input size {list(x.shape)} does not match the object's sizes {self._shape}")
        dev = self._dev(x if isinstance(x, torch.Tensor) else None)
        xk = self._to_device_kernel_order(x, dev, self.NDIM)
        plan = self._plan(xk.is_complex(), 1, dev)
        with torch.cuda.device(dev):
            if per_item:
                return plan.estimate_sigma_items(xk.data_ptr(), _current_stream(dev))
            return plan.estimate_sigma(xk.data_ptr(), _current_stream(dev))

    def _coef_for_stats(self, y):
        if y.ndim != len(self._shape) + 1 or list(y.shape[:-1]) != self._shape:
            raise ValueError(f"coefficient array must have shape {self._shape + ['bands']}")
        level = self._level_from_bands(int(y.shape[-1]))
        dev = self._dev(y if isinstance(y, torch.Tensor) else None)
        yk, pitch = self._coef_kernel_order(y, dev)
        return yk, pitch, level, dev, self._plan(yk.is_complex(), level, dev)

    def estimate_sigma_coef(self, y, per_item=False):
        """estimate_sigma from a coefficient array (what dec returns, any level): its last band is the one the estimate reads"""
        yk, pitch, level, dev, plan = self._coef_for_stats(y)
        with torch.cuda.device(dev):
            if per_item:
                return plan.estimate_sigma_coef_items(yk.data_ptr(), level, _current_stream(dev), band_pitch=pitch)
            return plan.estimate_sigma_coef(yk.data_ptr(), level, _current_stream(dev), band_pitch=pitch)

    def band_median(self, y, band, per_item=False):
        """The median of |c| over band `band` of a coefficient array, exactly (an even count: the mean of the two middle order
        statistics, as numpy.median); complex data: of the magnitude the shrink compares.  Computed on the device without a sort.
        per_item=True: the median of every signal of the batch / item of the stack on its own, a length-K array."""
        yk, pitch, level, dev, plan = self._coef_for_stats(y)
        n = int(np.prod(yk.shape[1:]))
        if per_item:
            n //= plan.items
            with torch.cuda.device(dev):
                v = plan.band_select_items(yk.data_ptr(), level, int(band), [(n - 1) // 2] if n % 2 else [n // 2 - 1, n // 2], _current_stream(dev), band_pitch=pitch)
            return v[:, 0].copy() if n % 2 else 0.5 * (v[:, 0] + v[:, 1])
        with torch.cuda.device(dev):
            v = plan.band_select(yk.data_ptr(), level, int(band), [(n - 1) // 2] if n % 2 else [n // 2 - 1, n // 2], _current_stream(dev), band_pitch=pitch)
        return float(v[0]) if n % 2 else 0.5 * float(v[0] + v[1])

    def universal_thresholds(self, x, level, k=None, per_item=False):
        """k * estimate_sigma(x) * band_gains(level) with entry 0 (the approximation) set to 0: one threshold per band, as denoise(x, level,
        thresholds) and shrink(y, thresholds) take them.  k defaults to the universal sqrt(2 ln N), N = the samples of one item's
        filtered axes.  per_item=True: a [K, bands] array, row j from the estimate of item j alone (column 0 zero)."""
        if k is None:
            k = float(np.sqrt(2.0 * np.log(float(np.prod(self.sizes, dtype=np.float64)))))
        if per_item:
            thr = float(k) * np.outer(self.estimate_sigma(x, per_item=True), self.band_gains(level))
            thr[:, 0] = 0.0
            return thr
        thr = float(k) * self.estimate_sigma(x) * self.band_gains(level)
        thr[0] = 0.0
        return thr

    # -- sums over the bands, in one read of the coefficient array on the device (extension; not in the reference) --
    def _band_norms(self, y, per_item):
        """(the [bands, 4] or [K, bands, 4] array of Plan.band_norms / band_norms_items, elements of one block, scalars per element)"""
        yk, pitch, level, dev, plan = self._coef_for_stats(y)
        n = int(np.prod(yk.shape[1:]))
        with torch.cuda.device(dev):
            if per_item:
                return plan.band_norms_items(yk.data_ptr(), level, _current_stream(dev), band_pitch=pitch), n // plan.items, 2 if yk.is_complex() else 1
            return plan.band_norms(yk.data_ptr(), level, _current_stream(dev), band_pitch=pitch), n, 2 if yk.is_complex() else 1

    def band_norms(self, y, per_item=False):
        """The sums of every band of a coefficient array (what dec returns), computed on the device in one read of it: a dict of arrays
        `l1` (sum of |c|), `l2sq` (sum of |c|^2), `max` (the largest |c|) and `nnz` (the count of c != 0), one entry per band, band 0
        included; complex data: |c| is the magnitude the shrink compares.  A band is the whole array (all signals of a batch, all items of
        a stack); per_item=True: [K, bands] arrays, row j from signal / item j alone.  The call waits for the result."""
        v, _, _ = self._band_norms(y, per_item)
        return {"l1": v[..., L.NDWT_NORM_L1].copy(), "l2sq": v[..., L.NDWT_NORM_L2SQ].copy(), "max": v[..., L.NDWT_NORM_MAX].copy(),
                "nnz": v[..., L.NDWT_NORM_NNZ].copy()}

    def l1_norm(self, y, weights=None, per_item=False):
        """sum over the bands of weights[b] * (the sum of |c| over band b): the penalty of an l1-regularised solver.  weights: one per band;
        by default 0 for band 0 and 1 for every other band, the bands `shrink` touches.  A float, or a length-K array with per_item=True."""
        if y.ndim != len(self._shape) + 1 or list(y.shape[:-1]) != self._shape:
            raise ValueError(f"coefficient array must have shape {self._shape + ['bands']}")
        nb = int(y.shape[-1])
        if weights is None:
            w = np.ones(nb)
            w[0] = 0.0
        else:
            w = np.asarray(weights, dtype=np.float64).reshape(-1)
            if w.size != nb:
                raise ValueError(f"{nb} weights expected, one per band of the coefficient array, got {w.size}")
        r = self.band_norms(y, per_item)["l1"] @ w
        return r if per_item else float(r)

    def group_norms(self, y):
        """The sums over the groups of every band of a coefficient array -- a group is the K coefficients at one position across the
        signals of a batch / items of a stack -- in one read of it: a dict of arrays `l1` (the sum of the groups' magnitudes: the l2,1
        norm of the band), `l2sq` (the sum of their squares), `max` (the largest) and `nnz` (the count of groups that are not all zero),
        one entry per band, band 0 included.  Without a batch or stack the group is the element.  The call waits for the result."""
        yk, pitch, level, dev, plan = self._coef_for_stats(y)
        with torch.cuda.device(dev):
            v = plan.group_norms(yk.data_ptr(), level, _current_stream(dev), band_pitch=pitch)
        return {"l1": v[:, L.NDWT_NORM_L1].copy(), "l2sq": v[:, L.NDWT_NORM_L2SQ].copy(), "max": v[:, L.NDWT_NORM_MAX].copy(),
                "nnz": v[:, L.NDWT_NORM_NNZ].copy()}

    def l21_norm(self, y, weights=None):
        """sum over the bands of weights[b] * (the l2,1 norm of band b): the penalty whose prox shrink(.., joint=True) is.  weights: one per
        band; by default 0 for band 0 and 1 for every other band.  A float."""
        if y.ndim != len(self._shape) + 1 or list(y.shape[:-1]) != self._shape:
            raise ValueError(f"coefficient array must have shape {self._shape + ['bands']}")
        nb = int(y.shape[-1])
        if weights is None:
            w = np.ones(nb)
            w[0] = 0.0
        else:
            w = np.asarray(weights, dtype=np.float64).reshape(-1)
            if w.size != nb:
                raise ValueError(f"{nb} weights expected, one per band of the coefficient array, got {w.size}")
        return float(self.group_norms(y)["l1"] @ w)

    def sparsity(self, y, per_item=False):
        """the fraction of coefficients that are not zero, over all bands: a float, or a length-K array with per_item=True"""
        v, n, _ = self._band_norms(y, per_item)
        r = v[..., L.NDWT_NORM_NNZ].sum(axis=-1) / (float(n) * v.shape[-2])
        return r if per_item else float(r)

    def bayes_thresholds(self, x, level, per_item=False):
        """BayesShrink thresholds for this frame (Chang, Yu and Vetterli), one per band, as denoise(x, level, thresholds) and shrink(y,
        thresholds) take them.  With s_b = estimate_sigma(x) * band_gains(level)[b], the noise in band b, and v_b = max(l2sq_b / (elements *
        parts) - s_b^2, 0), the signal variance of each part (1 for real, 2 for complex data) of a coefficient of dec(x, level):
        t_b = s_b^2 / sqrt(v_b), and where v_b = 0 -- a band of noise alone -- t_b = the band's largest magnitude, so the band goes to zero.
        Entry 0 (the approximation) is 0.  per_item=True: a [K, bands] array, row j from signal / item j alone."""
        level = int(level)
        s = np.multiply.outer(np.asarray(self.estimate_sigma(x, per_item=per_item), dtype=np.float64), self.band_gains(level))
        v, n, comp = self._band_norms(self.dec(x, level), per_item)
        var = np.maximum(v[..., L.NDWT_NORM_L2SQ] / (float(n) * comp) - s * s, 0.0)
        thr = np.where(var > 0.0, s * s / np.sqrt(np.where(var > 0.0, var, 1.0)), v[..., L.NDWT_NORM_MAX])
        thr[..., 0] = 0.0
        return thr

    def band_risk(self, y, thresholds, per_item=False):
        """What Stein's unbiased risk estimate of a soft threshold needs of every band of a coefficient array (what dec returns), at up
        to 8 candidate thresholds per band in one read of the array: a dict of arrays `count` (the elements with |c| <= t, those a shrink at
        t sets to zero), `energy` (the sum of |c|^2 over them) and `invsum` (complex data: the sum of 1 / |c| over the others; real data:
        0), shaped like `thresholds`: [bands, nc], or with per_item=True [K, bands, nc], row j from signal / item j alone.  A row of
        thresholds that begins with a negative entry skips its band: zeros.  The call waits for the result."""
        yk, pitch, level, dev, plan = self._coef_for_stats(y)
        if isinstance(thresholds, torch.Tensor):
            thresholds = thresholds.detach().cpu().numpy()
        with torch.cuda.device(dev):
            if per_item:
                v = plan.band_risk_items(yk.data_ptr(), level, thresholds, _current_stream(dev), band_pitch=pitch)
            else:
                v = plan.band_risk(yk.data_ptr(), level, thresholds, _current_stream(dev), band_pitch=pitch)
        return {"count": v[..., L.NDWT_RISK_COUNT].copy(), "energy": v[..., L.NDWT_RISK_ENERGY].copy(), "invsum": v[..., L.NDWT_RISK_INVSUM].copy()}

    def sure_thresholds(self, x, level, per_item=False, hybrid=True, rounds=3):
        """SureShrink thresholds for this frame (Donoho and Johnstone), one per band, as denoise(x, level, thresholds) and shrink(y,
        thresholds) take them: with s_b = estimate_sigma(x) * band_gains(level)[b], the soft threshold in [0, s_b sqrt(2 ln N)] that
        minimises Stein's unbiased estimate of the risk over band b of dec(x, level), searched on the device in `rounds` reads of the
        detail bands (3: to 1/128 of the interval).  hybrid=True: a band too sparse for the estimate -- (l2sq_b / s_b^2 - d N) / (d N) <=
        log2(N)^1.5 / sqrt(N), d = 1 for real and 2 for complex data, N = the samples of one item's filtered axes -- gets the universal
        s_b sqrt(2 ln N).  Entry 0 (the approximation) is 0.  per_item=True: a [K, bands] array, row j from signal / item j alone."""
        level = int(level)
        sigma = self.estimate_sigma(x, per_item=per_item)
        y = self.dec(x, level)
        yk, pitch, _, dev, plan = self._coef_for_stats(y)
        with torch.cuda.device(dev):
            if per_item:
                thr, _ = plan.sure_thresholds_items(yk.data_ptr(), level, sigma, rounds, _current_stream(dev), band_pitch=pitch)
            else:
                thr, _ = plan.sure_thresholds(yk.data_ptr(), level, sigma, rounds, _current_stream(dev), band_pitch=pitch)
        if hybrid:
            N = float(np.prod(self.sizes, dtype=np.float64))
            s = np.multiply.outer(np.asarray(sigma, dtype=np.float64), self.band_gains(level))
            v, n, comp = self._band_norms(y, per_item)
            dn = float(n) * comp
            with np.errstate(divide="ignore", invalid="ignore"):
                sparse = (v[..., L.NDWT_NORM_L2SQ] / (s * s) - dn) / dn <= np.log2(N) ** 1.5 / np.sqrt(N)
            thr = np.where(sparse, s * np.sqrt(2.0 * np.log(N)), thr)
        thr[..., 0] = 0.0
        return thr

    def _prep_dec_input(self, x):
        return x

    def _multi(self, a, level, direction):
        """host array through the single-process multi-device plan (the 'devices' option)"""
        like_numpy = isinstance(a, np.ndarray)
        an = a if like_numpy else a.cpu().numpy()
        cplx = np.iscomplexobj(an)
        single = self.precision.lower() == "single"
        cdt = (np.complex64 if single else np.complex128) if cplx else (np.float32 if single else np.float64)
        ak = np.ascontiguousarray(np.transpose(an)).astype(cdt, copy=False)
        key = ("multi", cplx)
        mp = self._plans.get(key)
        if mp is None or mp.max_level < level:
            mp = MultiPlan(self.sizes, self.wname[: self.NDIM], torch.float32 if single else torch.float64, self.devices, cplx,
                           self.pres_l2_norm, self.dilation, max_level=max(level, 3))
            self._plans[key] = mp
        out = np.transpose(mp.rec(ak) if direction == "rec" else mp.dec(ak, level))
        return out if like_numpy else torch.from_numpy(np.ascontiguousarray(out))


class nd_dwt_1D(_NdDwtBase):
    """Functions/nd_dwt_1D.m -- 1-D signal of length n; coefficients [n, 1+level].
    nd_dwt_1D(wname, n, 'batch', K): K signals per call -- dec takes [n, K] (column k = signal k) and returns [n, K, 1+level]; rec, shrink
    and denoise likewise.  In memory that is (K, n) contiguous: a device tensor laid out so is used where it lies."""
    NDIM = 1

    def _check_sizes(self, sizes):
        if len(sizes) != 1:
            raise ValueError("1D array length must be a scalar")          # nd_dwt_1D.m:88

    def _check_wname(self, wname):
        if not isinstance(wname, str):
            raise ValueError("Wavelet Name Must be a string")             # nd_dwt_1D.m:84
        return [wname, wname]

    def _level_from_bands(self, n):
        return int(np.ceil(n - 1))                                        # nd_dwt_1D.m:213

    def _prep_dec_input(self, x):
        # row vectors are transposed (nd_dwt_1D.m:151-153); accept [n], [n,1] and [1,n]; a batched object takes [n, batch] as it is
        if self.batch is None and self.inner is None and x.ndim == 2 and 1 in x.shape:
            x = x.reshape(-1)
        return x


class nd_dwt_2D(_NdDwtBase):
    """Functions/nd_dwt_2D.m -- coefficients [n1, n2, 4+3(level-1)].
    nd_dwt_2D(wname, [n1, n2], 'stack', K): K images per call -- dec takes [n1, n2, K] and returns [n1, n2, K, bands], image j transformed
    on its own; rec, shrink and denoise likewise.  In memory that is (K, n2, n1) contiguous."""
    NDIM = 2

    def _check_sizes(self, sizes):
        if len(sizes) != 2:
            raise ValueError("The sizes vector must be length 2")

    def _check_wname(self, wname):
        if isinstance(wname, str):
            return [wname, wname]
        if len(wname) != 2:
            raise ValueError("You must specify two filter names in a cell array of length 2, or a single string for the "
                             "same filter to be used in all dimensions")
        return list(wname)

    def _level_from_bands(self, n):
        return int(1 + (n - 4) / 3)                                       # nd_dwt_2D.m:215


class nd_dwt_3D(_NdDwtBase):
    """Functions/nd_dwt_3D.m -- coefficients [n1, n2, n3, 8+7(level-1)].
    nd_dwt_3D(wname, [n1, n2, n3], 'stack', K): K volumes per call -- dec takes [n1, n2, n3, K] and returns [n1, n2, n3, K, bands]."""
    NDIM = 3

    def _check_sizes(self, sizes):
        if len(sizes) != 3:
            raise ValueError("The sizes vector must be length 3")          # nd_dwt_3D.m:83

    def _check_wname(self, wname):
        if isinstance(wname, str):
            return [wname, wname, wname]
        if len(wname) != 3:                                               # nd_dwt_3D.m:94-96
            raise ValueError("You must specify three filter names in a cell arrayof length 3, or a single string for "
                             "the same filter to be used in all dimensions")
        return list(wname)

    def _level_from_bands(self, n):
        return int(np.ceil(n / 8))                                        # nd_dwt_3D.m:217 (breaks for level >= 9, as there)


class nd_dwt_4D(_NdDwtBase):
    """Functions/nd_dwt_4D.m ('fft' method semantics) -- coefficients [n1, n2, n3, n4, 16+15(level-1)]."""
    NDIM = 4

    def _check_sizes(self, sizes):
        if len(sizes) != 4:
            raise ValueError("The sizes vector must be length 4")

    def _check_wname(self, wname):
        if isinstance(wname, str):
            return [wname] * 4
        if len(wname) != 4:
            raise ValueError("You must specify four filter names in a cell array of length 4, or a single string for "
                             "the same filter to be used in all dimensions")
        return list(wname)

    def _level_from_bands(self, n):
        return int(1 + (n - 16) / 15)                                     # nd_dwt_4D.m:213
