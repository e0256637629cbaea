"""ctypes binding of libndwt_hip.so (the C ABI declared in include/ndwt.h).

The library is built in-tree by `make -C csrc` (hipcc, gfx950).  There is no CPU fallback: if the
shared object is missing, or no HIP device is usable, the calls raise.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# NDWT_LIB_VARIANT=<name> loads libndwt_hip_<name>.so (diagnostic / tuning builds of tools/, `make VARIANT=<name>`)
LIB_PATH = os.path.join(_HERE, "libndwt_hip" + ("_" + os.environ["NDWT_LIB_VARIANT"] if os.environ.get("NDWT_LIB_VARIANT") else "") + ".so")

# status codes / enums of include/ndwt.h
NDWT_OK = 0
NDWT_F32, NDWT_F64 = 0, 1
NDWT_REAL, NDWT_COMPLEX_INTERLEAVED = 0, 1
NDWT_DILATION_REFERENCE, NDWT_DILATION_ATROUS = 0, 1
NDWT_PATH_AUTO, NDWT_PATH_GENERIC = 0, 1
NDWT_NORM_L1, NDWT_NORM_L2SQ, NDWT_NORM_MAX, NDWT_NORM_NNZ, NDWT_NORM_COUNT = 0, 1, 2, 3, 4
NDWT_RISK_COUNT, NDWT_RISK_ENERGY, NDWT_RISK_INVSUM, NDWT_RISK_STATS = 0, 1, 2, 3
NDWT_RISK_MAX_CAND = 8

EXPORTS = [
    "ndwt_wave_filters", "ndwt_num_bands", "ndwt_level_from_bands", "ndwt_plan_create", "ndwt_plan_create_slab", "ndwt_plan_destroy",
    "ndwt_plan_set_path", "ndwt_plan_describe", "ndwt_plan_set_tuning", "ndwt_plan_set_variant", "ndwt_plan_set_fused_level1", "ndwt_plan_set_profiling", "ndwt_plan_get_profile", "ndwt_dec", "ndwt_rec", "ndwt_dec_host",
    "ndwt_rec_host", "ndwt_shrink", "ndwt_denoise", "ndwt_denoise_host", "ndwt_dec_split", "ndwt_rec_split", "ndwt_dec_split_host", "ndwt_rec_split_host", "ndwt_slab_halo", "ndwt_analysis_level_slab", "ndwt_synthesis_level_slab",
    "ndwt_analysis_level_slab_split", "ndwt_synthesis_level_slab_ext", "ndwt_analysis_level_slab_part",
    "ndwt_synthesis_level_slab_part", "ndwt_analysis_level_slab_runs", "ndwt_synthesis_level_slab_runs", "ndwt_last_error",
    "ndwt_version", "ndwt_mplan_create", "ndwt_mplan_destroy", "ndwt_mplan_num_slabs", "ndwt_mplan_slab", "ndwt_mdec_host",
    "ndwt_mrec_host", "ndwt_mplan_last_error", "ndwt_mdec", "ndwt_mrec", "ndwt_mplan_set_exchange", "ndwt_mplan_describe", "ndwt_plan_slab_fast", "ndwt_dec_pitched", "ndwt_rec_pitched", "ndwt_shrink_pitched", "ndwt_band_pitch", "ndwt_slab_segments",
    "ndwt_plan_release_staging", "ndwt_mplan_set_overlap", "ndwt_mplan_last_enqueue_us", "ndwt_mplan_set_threads", "ndwt_comm_unique_id", "ndwt_comm_create", "ndwt_comm_destroy", "ndwt_comm_exchange",
    "ndwt_comm_last_error", "ndwt_coef_create", "ndwt_coef_release", "ndwt_coef_info", "ndwt_coef_dec_host", "ndwt_coef_rec_host",
    "ndwt_coef_shrink", "ndwt_coef_get_host", "ndwt_coef_put_host", "ndwt_plan_create_slab_axis", "ndwt_slab_segments_strided",
    "ndwt_mplan_create_axis", "ndwt_trace_enable", "ndwt_trace_get", "ndwt_plan_create_many", "ndwt_plan_create_axes",
    "ndwt_plan_create_interleaved", "ndwt_band_gains", "ndwt_shrink_bands", "ndwt_denoise_bands", "ndwt_band_select",
    "ndwt_estimate_sigma_coef", "ndwt_estimate_sigma", "ndwt_band_select_items", "ndwt_estimate_sigma_coef_items", "ndwt_estimate_sigma_items",
    "ndwt_shrink_bands_items", "ndwt_denoise_bands_items", "ndwt_band_norms", "ndwt_band_norms_items", "ndwt_band_norms_dev",
    "ndwt_band_risk", "ndwt_band_risk_items", "ndwt_sure_from_risk", "ndwt_sure_thresholds", "ndwt_sure_thresholds_items",
    "ndwt_shrink_joint", "ndwt_denoise_joint", "ndwt_group_norms", "ndwt_group_norms_dev",
    "ndwt_shrink_neigh", "ndwt_denoise_neigh",
]


class NdwtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ndwt error {code}: {msg}")
        self.code = code
        self.message = msg


def build(verbose: bool = False) -> str:
    """Compile the HIP extension in-tree (hipcc --offload-arch=gfx950)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j", str(min(8, os.cpu_count() or 1))]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout)
    if r.returncode != 0:
        raise RuntimeError("building libndwt_hip.so failed")
    return LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension must be built first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C non-decimated_wavelets_amd/csrc). "
            "This engine has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    c_void_pp = ctypes.POINTER(ctypes.c_void_p)
    L.ndwt_wave_filters.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(ctypes.c_int)]
    L.ndwt_num_bands.argtypes = [ctypes.c_int, ctypes.c_int]
    L.ndwt_num_bands.restype = ctypes.c_int64
    L.ndwt_level_from_bands.argtypes = [ctypes.c_int, ctypes.c_int64]
    L.ndwt_plan_create.argtypes = [c_void_pp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_char_p),
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ndwt_plan_create_many.argtypes = [c_void_pp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.POINTER(ctypes.c_char_p),
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ndwt_plan_create_axes.argtypes = [c_void_pp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_uint, ctypes.POINTER(ctypes.c_char_p),
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ndwt_plan_create_interleaved.argtypes = [c_void_pp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_int64,
                                               ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int]
    L.ndwt_plan_create_slab.argtypes = [c_void_pp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.POINTER(ctypes.c_char_p),
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ndwt_plan_create_slab_axis.argtypes = [c_void_pp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int64,
                                             ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int]
    L.ndwt_plan_destroy.argtypes = [ctypes.c_void_p]
    L.ndwt_plan_set_path.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndwt_plan_set_tuning.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.ndwt_plan_set_variant.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5
    L.ndwt_plan_set_fused_level1.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndwt_plan_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndwt_plan_get_profile.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]
    L.ndwt_plan_describe.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    for f in (L.ndwt_dec, L.ndwt_rec):
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    for f in (L.ndwt_dec_host, L.ndwt_rec_host):
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.ndwt_shrink.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
    L.ndwt_dec_pitched.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    L.ndwt_rec_pitched.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.ndwt_shrink_pitched.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
    L.ndwt_band_pitch.argtypes = [ctypes.c_void_p]
    L.ndwt_band_pitch.restype = ctypes.c_int64
    L.ndwt_denoise.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                               ctypes.c_void_p]
    L.ndwt_band_gains.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_double)]
    L.ndwt_shrink_bands.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                    ctypes.c_void_p]
    L.ndwt_denoise_bands.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                     ctypes.c_void_p]
    L.ndwt_band_select.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p]
    L.ndwt_estimate_sigma_coef.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                           ctypes.c_void_p]
    L.ndwt_estimate_sigma.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p]
    # the per-item forms: the signatures of their band-wide namesakes (the host arrays are longer)
    L.ndwt_band_select_items.argtypes = L.ndwt_band_select.argtypes
    L.ndwt_estimate_sigma_coef_items.argtypes = L.ndwt_estimate_sigma_coef.argtypes
    L.ndwt_estimate_sigma_items.argtypes = L.ndwt_estimate_sigma.argtypes
    L.ndwt_shrink_bands_items.argtypes = L.ndwt_shrink_bands.argtypes
    L.ndwt_denoise_bands_items.argtypes = L.ndwt_denoise_bands.argtypes
    # the band norms: host results [nb][4] / [items][nb][4], or the same on the device (per_item chooses the layout)
    L.ndwt_band_norms.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p]
    L.ndwt_band_norms_items.argtypes = L.ndwt_band_norms.argtypes
    L.ndwt_band_norms_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    # the SURE statistics: candidates [nb][nc] / [items][nb][nc] and results [..][nc][3] on the host; the estimate (host only); the search
    c_double_p = ctypes.POINTER(ctypes.c_double)
    L.ndwt_band_risk.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_void_p]
    L.ndwt_band_risk_items.argtypes = L.ndwt_band_risk.argtypes
    L.ndwt_sure_from_risk.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_double_p, c_double_p, c_double_p]
    L.ndwt_sure_thresholds.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_int, c_double_p, c_double_p,
                                       ctypes.c_void_p]
    L.ndwt_sure_thresholds_items.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p,
                                             ctypes.c_void_p]
    # joint shrinkage across the items and the group norms: thresholds [nb] on the host; results [nb][4] on the host or on the device
    L.ndwt_shrink_joint.argtypes = L.ndwt_shrink_bands.argtypes
    L.ndwt_denoise_joint.argtypes = L.ndwt_denoise_bands.argtypes
    L.ndwt_group_norms.argtypes = L.ndwt_band_norms.argtypes
    L.ndwt_group_norms_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    # neighbourhood shrinkage: out of place, a radius, thresholds [nb] on the host
    L.ndwt_shrink_neigh.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int,
                                    ctypes.c_void_p]
    L.ndwt_denoise_neigh.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, ctypes.c_void_p]
    L.ndwt_denoise_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int]
    for f in (L.ndwt_dec_split, L.ndwt_rec_split):
        f.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p]
    for f in (L.ndwt_dec_split_host, L.ndwt_rec_split_host):
        f.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 4 + [ctypes.c_int]
    L.ndwt_slab_halo.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int64)] * 4
    L.ndwt_analysis_level_slab.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_void_pp, ctypes.c_int, ctypes.c_void_p]
    L.ndwt_synthesis_level_slab.argtypes = [ctypes.c_void_p, c_void_pp, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.ndwt_analysis_level_slab_split.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_void_pp,
                                                 ctypes.c_int, ctypes.c_void_p]
    L.ndwt_synthesis_level_slab_ext.argtypes = [ctypes.c_void_p, c_void_pp, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.ndwt_analysis_level_slab_part.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_void_pp,
                                                ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    L.ndwt_synthesis_level_slab_part.argtypes = [ctypes.c_void_p, c_void_pp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                 ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.ndwt_analysis_level_slab_runs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_void_pp, ctypes.c_int, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    L.ndwt_synthesis_level_slab_runs.argtypes = [ctypes.c_void_p, c_void_pp] + [ctypes.c_int64] * 5 + [ctypes.c_void_p, ctypes.c_int,
                                                                                                    ctypes.c_void_p]
    L.ndwt_mplan_create.argtypes = [c_void_pp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_char_p), ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.ndwt_mplan_create_axis.argtypes = L.ndwt_mplan_create.argtypes + [ctypes.c_int]
    L.ndwt_mplan_destroy.argtypes = [ctypes.c_void_p]
    L.ndwt_mplan_num_slabs.argtypes = [ctypes.c_void_p]
    L.ndwt_mplan_slab.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64),
                                  ctypes.POINTER(ctypes.c_int64)]
    for f in (L.ndwt_mdec_host, L.ndwt_mrec_host):
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.ndwt_mplan_last_error.restype = ctypes.c_char_p
    for f in (L.ndwt_mdec, L.ndwt_mrec):
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    L.ndwt_mplan_set_exchange.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndwt_mplan_set_overlap.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndwt_mplan_set_threads.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndwt_mplan_last_enqueue_us.argtypes = [ctypes.c_void_p]
    L.ndwt_mplan_last_enqueue_us.restype = ctypes.c_double
    L.ndwt_mplan_describe.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    L.ndwt_trace_enable.argtypes = [ctypes.c_int]
    L.ndwt_trace_get.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.ndwt_plan_slab_fast.argtypes = [ctypes.c_void_p]
    L.ndwt_plan_release_staging.argtypes = [ctypes.c_void_p]
    L.ndwt_comm_unique_id.argtypes = [ctypes.c_void_p]
    L.ndwt_comm_create.argtypes = [c_void_pp, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ndwt_comm_destroy.argtypes = [ctypes.c_void_p]
    L.ndwt_comm_exchange.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), c_void_pp, ctypes.POINTER(ctypes.c_int64),
                                     ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
    L.ndwt_comm_last_error.restype = ctypes.c_char_p
    L.ndwt_coef_create.argtypes = [ctypes.c_void_p, ctypes.c_int, c_void_pp]
    L.ndwt_coef_release.argtypes = [ctypes.c_void_p]
    L.ndwt_coef_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), c_void_pp]
    L.ndwt_coef_dec_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, c_void_pp]
    L.ndwt_coef_rec_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.ndwt_coef_shrink.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int]
    L.ndwt_coef_get_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.ndwt_coef_put_host.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, c_void_pp]
    L.ndwt_slab_segments.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_void_pp, c_void_pp, ctypes.POINTER(ctypes.c_int64),
                                     ctypes.c_void_p]
    L.ndwt_slab_segments_strided.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_void_pp, c_void_pp, ctypes.POINTER(ctypes.c_int64),
                                             ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    L.ndwt_last_error.restype = ctypes.c_char_p
    L.ndwt_version.restype = ctypes.c_char_p
    _lib = L
    return L


def check(rc: int):
    if rc != NDWT_OK:
        raise NdwtError(rc, lib().ndwt_last_error().decode())


def mcheck(rc: int):
    if rc != NDWT_OK:
        raise NdwtError(rc, lib().ndwt_mplan_last_error().decode())


def wave_filters(wname: str):
    """(LO_D, HI_D) as lists -- Functions/wave_filters.m through the C ABI."""
    lo = (ctypes.c_double * 20)()
    hi = (ctypes.c_double * 20)()
    n = ctypes.c_int(0)
    check(lib().ndwt_wave_filters(wname.encode(), lo, hi, ctypes.byref(n)))
    return list(lo[: n.value]), list(hi[: n.value])


def band_gains(dims, wnames, level, pres_l2_norm=0, dilation="reference"):
    """Standard deviation of every band of a `level`-level transform of unit-variance white noise on an array of `dims` (the filtered
    axes of one item), as a numpy array of ndwt_num_bands(len(dims), level) doubles -- include/ndwt.h: ndwt_band_gains.  Host only: no
    device is needed.  wnames: one name for every axis, or a name per axis.  thresholds[b] = k * sigma * gains[b]."""
    import numpy as np
    dims = [int(d) for d in np.atleast_1d(dims)]
    names = [wnames] * len(dims) if isinstance(wnames, str) else list(wnames)
    if len(names) != len(dims):
        raise ValueError(f"{len(dims)} axes need {len(dims)} wavelet names (or one for all), got {len(names)}")
    if dilation not in ("reference", "atrous"):
        raise ValueError("dilation must be 'reference' or 'atrous'")
    nb = int(lib().ndwt_num_bands(len(dims), int(level)))
    out = np.zeros(max(nb, 1))
    c_dims = (ctypes.c_int64 * len(dims))(*dims)
    c_names = (ctypes.c_char_p * len(dims))(*[None if w is None else str(w).encode() for w in names])
    check(lib().ndwt_band_gains(len(dims), c_dims, c_names, int(bool(pres_l2_norm)), NDWT_DILATION_ATROUS if dilation == "atrous" else NDWT_DILATION_REFERENCE,
                                int(level), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out[:nb]


def sure_from_risk(comp, n, s, cand, risk):
    """Stein's unbiased estimate of the risk of a soft threshold at every candidate of ONE block, from the statistics of band_risk --
    include/ndwt.h: ndwt_sure_from_risk.  comp: 1 real, 2 complex data; n: the elements of the block; s: the standard deviation of the
    noise in each real part of a coefficient of the band; cand: nc thresholds; risk: [nc, 3] (count, energy, invsum).  A length-nc
    numpy array.  Host only: no device is needed."""
    import numpy as np
    c = np.ascontiguousarray(np.asarray(cand, dtype=np.float64).reshape(-1))
    r = np.ascontiguousarray(np.asarray(risk, dtype=np.float64))
    if r.shape != (c.size, NDWT_RISK_STATS):
        raise ValueError(f"risk must be a [{c.size}, {NDWT_RISK_STATS}] array, one row per candidate, got {list(r.shape)}")
    out = np.zeros(max(c.size, 1))
    dp = ctypes.POINTER(ctypes.c_double)
    check(lib().ndwt_sure_from_risk(int(comp), float(n), float(s), int(c.size), c.ctypes.data_as(dp), r.ctypes.data_as(dp), out.ctypes.data_as(dp)))
    return out[:c.size]
