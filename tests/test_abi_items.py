"""The per-item calls without a GPU: the five exports (ndwt_band_select_items, ndwt_estimate_sigma_coef_items, ndwt_estimate_sigma_items,
ndwt_shrink_bands_items, ndwt_denoise_bands_items), their declarations in include/ndwt.h and their bindings, the refusals that need no
plan, the methods and options the classes gained, and the trace parser's table of the two new kernel families.  (The refusals that need
a plan -- item and band of a bad threshold, ranks outside one item -- are in tests/test_gpu_items.py: a plan needs a device.)
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import ndwt_amd as ndwt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndwt_band_select_items", "ndwt_estimate_sigma_coef_items", "ndwt_estimate_sigma_items", "ndwt_shrink_bands_items", "ndwt_denoise_bands_items")
# the documented signatures: those of the band-wide namesakes
SIGNATURES = {
    "ndwt_band_select_items": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, int64_t band, int nk, const int64_t* k, double* values, void* stream",
    "ndwt_estimate_sigma_coef_items": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* sigma, void* stream",
    "ndwt_estimate_sigma_items": "ndwt_plan* plan, const void* x_dev, double* sigma, void* stream",
    "ndwt_shrink_bands_items": "ndwt_plan* plan, void* y_dev, int64_t band_pitch, int level, const double* thresholds, int mode, void* stream",
    "ndwt_denoise_bands_items": "ndwt_plan* plan, const void* x_dev, void* out_dev, int level, const double* thresholds, int mode, void* stream",
}


def test_the_five_symbols_are_exported_declared_and_bound():
    lib = ndwt.lib()
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    for name in NEW:
        assert name in ndwt._lib.EXPORTS
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
        assert f"int {name}({SIGNATURES[name]});" in hdr, name
        assert len(getattr(lib, name).argtypes) == SIGNATURES[name].count(",") + 1
    assert "a statistic per item is not offered" not in hdr


def test_the_calls_refuse_a_null_plan_and_write_nothing():
    lib = ndwt.lib()
    buf = ctypes.create_string_buffer(64)
    k = (ctypes.c_int64 * 4)(0, 0, 0, 0)
    v = (ctypes.c_double * 4)()
    s = (ctypes.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    t = (ctypes.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    err = lambda: lib.ndwt_last_error().decode()
    assert lib.ndwt_band_select_items(None, buf, 0, 1, 0, 1, k, v, None) == 1 and "null plan" in err()
    assert lib.ndwt_estimate_sigma_coef_items(None, buf, 0, 1, s, None) == 1 and "null plan" in err()
    assert lib.ndwt_estimate_sigma_items(None, buf, s, None) == 1 and "null plan" in err()
    assert lib.ndwt_shrink_bands_items(None, buf, 0, 1, t, 0, None) == 1 and "null plan" in err()
    assert lib.ndwt_denoise_bands_items(None, buf, buf, 1, t, 0, None) == 1 and "null plan" in err()
    assert list(s) == [-1.0] * 4 and list(v) == [0.0] * 4 and buf.raw == b"\0" * 64


def test_the_methods_and_options_exist():
    for name in ("band_select_items", "estimate_sigma_items", "estimate_sigma_coef_items", "shrink_bands_items", "denoise_bands_items"):
        assert callable(getattr(ndwt.Plan, name)), name
    assert isinstance(ndwt.Plan.items, property)
    for cls in (ndwt.nd_dwt_1D, ndwt.nd_dwt_2D, ndwt.nd_dwt_3D, ndwt.nd_dwt_4D):
        for name in ("estimate_sigma", "estimate_sigma_coef", "band_median", "universal_thresholds"):
            p = inspect.signature(getattr(cls, name)).parameters
            assert "per_item" in p and p["per_item"].default is False, (cls.__name__, name)


def test_the_classes_take_a_row_of_thresholds_per_item_and_refuse_other_shapes():
    """_band_thresholds needs no device: [K, bands] stays 2-D for a batch or stack of K > 1; a scalar, a length-bands sequence and
    [1, bands] with K = 1 are what they were; any other shape raises"""
    w = ndwt.nd_dwt_1D("db2", 64, "batch", 5)
    nb = ndwt.num_bands(1, 2)
    t = np.arange(5 * nb, dtype=np.float64).reshape(5, nb)
    got = w._band_thresholds(t, 2)
    assert got.shape == (5, nb) and got.flags.c_contiguous and np.array_equal(got, t)
    assert w._band_thresholds(t[:, ::-1], 2).flags.c_contiguous
    assert w._band_thresholds(0.5, 2) is None
    assert w._band_thresholds([0.0, 1.0, 2.0], 2).shape == (nb,)
    for bad in (np.zeros((6, nb)), np.zeros((4, nb)), np.zeros((5, nb + 1)), np.zeros((nb, 5)), np.zeros((1, 5, nb))):
        with pytest.raises(ValueError, match=f"{nb} values, one per band of a 2-level transform"):
            w._band_thresholds(bad, 2)
    one = ndwt.nd_dwt_1D("db2", 64)
    assert one._band_thresholds(np.zeros((1, nb)), 2).shape == (nb,)           # K = 1: the 1-D form, as before
    with pytest.raises(ValueError):
        one._band_thresholds(np.zeros((2, nb)), 2)
    st = ndwt.nd_dwt_2D("db1", [8, 8], "stack", 4)
    assert st._band_thresholds(np.zeros((4, ndwt.num_bands(2, 1))), 1).shape == (4, 4)


def test_the_trace_parser_knows_the_two_families():
    r = ndwt.trace.parse_record("ndwt::ItemSelect<float, 1, true> grid=(5,1,1) block=(256,1,1)")
    assert r.family == "ItemSelect" and r.params == {"T": "float", "COMP": 1, "VEC": True, "AGG": 2} and r.grid == (5, 1, 1)
    r = ndwt.trace.parse_record("ndwt::ShrinkItems<double, 2, false> grid=(24,1,1) block=(256,1,1)")
    assert r.family == "ShrinkItems" and r.params == {"T": "double", "COMP": 2, "VEC": False}
    assert set(ndwt.trace.FAMILY_PARAMS_ITEMS) == {"ItemSelect", "ShrinkItems"}


def test_the_table_of_the_parser_matches_the_declarations():
    """FAMILY_PARAMS_ITEMS against the template heads of csrc/ndwt_device_items.h, as FAMILY_PARAMS is held to ndwt_device.h"""
    txt = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", "ndwt_device_items.h")).read()
    for fam, table in ndwt.trace.FAMILY_PARAMS_ITEMS.items():
        m = re.search(r"template <([^>]*)> struct " + fam + r" \{", txt)
        assert m, fam
        params = []
        for p in m.group(1).split(","):
            decl, _, default = p.strip().partition("=")
            name = decl.split()[-1].rstrip("_")
            d = default.strip()
            params.append((name, None if not d else (d == "true") if d in ("true", "false") else int(d)))
        assert params == table, (fam, params)
