"""The band norms without a GPU: the three exports (ndwt_band_norms, ndwt_band_norms_items, ndwt_band_norms_dev), their declarations in
include/ndwt.h and their bindings, the refusal that needs no plan, the enum, the methods the classes gained with their argument errors,
and the trace parser's table of the two new kernel families.  (The refusals that need a plan are in tests/test_gpu_norms.py: a plan needs
a device.)
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import ndwt_amd as ndwt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "ndwt_band_norms": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* norms, void* stream",
    "ndwt_band_norms_items": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* norms, void* stream",
    "ndwt_band_norms_dev": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, int per_item, double* norms_dev, void* stream",
}


def test_the_three_symbols_are_exported_declared_and_bound():
    lib = ndwt.lib()
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    for name, sig in SIGNATURES.items():
        assert name in ndwt._lib.EXPORTS
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
        assert f"int {name}({sig});" in hdr, name
        assert len(getattr(lib, name).argtypes) == sig.count(",") + 1
    assert lib.ndwt_band_norms_dev.argtypes[4] is ctypes.c_int and lib.ndwt_band_norms.argtypes[2] is ctypes.c_int64


def test_the_enum_values():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    assert "enum { NDWT_NORM_L1 = 0, NDWT_NORM_L2SQ = 1, NDWT_NORM_MAX = 2, NDWT_NORM_NNZ = 3, NDWT_NORM_COUNT = 4 };" in hdr
    L = ndwt._lib
    assert (L.NDWT_NORM_L1, L.NDWT_NORM_L2SQ, L.NDWT_NORM_MAX, L.NDWT_NORM_NNZ, L.NDWT_NORM_COUNT) == (0, 1, 2, 3, 4)


def test_the_calls_refuse_a_null_plan_and_write_nothing():
    lib = ndwt.lib()
    buf = ctypes.create_string_buffer(64)
    v = (ctypes.c_double * 8)(*([-1.0] * 8))
    err = lambda: lib.ndwt_last_error().decode()
    assert lib.ndwt_band_norms(None, buf, 0, 1, v, None) == 1 and "null plan" in err()
    assert lib.ndwt_band_norms_items(None, buf, 0, 1, v, None) == 1 and "null plan" in err()
    assert lib.ndwt_band_norms_dev(None, buf, 0, 1, 0, buf, None) == 1 and "null plan" in err()
    assert lib.ndwt_band_norms_dev(None, buf, 0, 1, 1, buf, None) == 1 and "null plan" in err()
    assert list(v) == [-1.0] * 8 and buf.raw == b"\0" * 64


def test_the_methods_exist():
    for name in ("band_norms", "band_norms_items", "band_norms_dev"):
        assert callable(getattr(ndwt.Plan, name)), name
    p = inspect.signature(ndwt.Plan.band_norms_dev).parameters
    assert list(p) == ["self", "y_ptr", "level", "out_ptr", "per_item", "stream", "band_pitch"] and p["per_item"].default is False
    assert list(inspect.signature(ndwt.Plan.band_norms).parameters) == ["self", "y_ptr", "level", "stream", "band_pitch"]
    for cls in (ndwt.nd_dwt_1D, ndwt.nd_dwt_2D, ndwt.nd_dwt_3D, ndwt.nd_dwt_4D):
        for name in ("band_norms", "l1_norm", "sparsity", "bayes_thresholds"):
            p = inspect.signature(getattr(cls, name)).parameters
            assert "per_item" in p and p["per_item"].default is False, (cls.__name__, name)
        assert inspect.signature(cls.l1_norm).parameters["weights"].default is None


def test_the_classes_refuse_a_wrong_weight_count_and_a_wrong_coefficient_shape():
    """both are decided before a device is asked for"""
    w = ndwt.nd_dwt_1D("db2", 64, "batch", 5)
    nb = ndwt.num_bands(1, 2)
    y = np.zeros((64, 5, nb))
    for bad in ([1.0] * (nb + 1), [1.0] * (nb - 1), np.ones((2, nb)), 1.0):
        with pytest.raises(ValueError, match=f"{nb} weights expected, one per band"):
            w.l1_norm(y, weights=bad)
    for f in (w.band_norms, w.l1_norm, w.sparsity):
        for bad in (np.zeros((64, 5)), np.zeros((63, 5, nb)), np.zeros((64, 4, nb)), np.zeros((64, 5, nb, 1))):
            with pytest.raises(ValueError, match="coefficient array must have shape"):
                f(bad)
    st = ndwt.nd_dwt_2D("db1", [8, 8], "stack", 4)
    with pytest.raises(ValueError, match="coefficient array must have shape"):
        st.band_norms(np.zeros((8, 8, 4)), per_item=True)
    with pytest.raises(ValueError, match="4 weights expected"):
        st.l1_norm(np.zeros((8, 8, 4, 4)), weights=[0, 1, 1])


def test_the_trace_parser_knows_the_two_families():
    r = ndwt.trace.parse_record("ndwt::BandNorms<float, 1, true> grid=(20,1,1) block=(256,1,1)")
    assert r.family == "BandNorms" and r.params == {"T": "float", "COMP": 1, "VEC": True} and r.grid == (20, 1, 1)
    r = ndwt.trace.parse_record("ndwt::BandNorms<double, 2, false> grid=(7,1,1) block=(256,1,1)")
    assert r.params == {"T": "double", "COMP": 2, "VEC": False}
    for text in ("ndwt::NormsFinish<> grid=(4,1,1) block=(64,1,1)", "ndwt::NormsFinish<64> grid=(4,1,1) block=(64,1,1)"):
        r = ndwt.trace.parse_record(text)
        assert r.family == "NormsFinish" and r.params == {"NT": 64} and r.block == (64, 1, 1)
    assert set(ndwt.trace.FAMILY_PARAMS_NORMS) == {"BandNorms", "NormsFinish"}


def test_the_table_of_the_parser_matches_the_declarations():
    """FAMILY_PARAMS_NORMS against the template heads of csrc/ndwt_device_norms.h, as test_abi_items.py holds its table to its header"""
    txt = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", "ndwt_device_norms.h")).read()
    for fam, table in ndwt.trace.FAMILY_PARAMS_NORMS.items():
        m = re.search(r"template <([^>]*)> struct " + fam + r" \{", txt)
        assert m, fam
        params = []
        for p in m.group(1).split(","):
            decl, _, default = p.strip().partition("=")
            name = decl.split()[-1].rstrip("_")
            d = default.strip()
            params.append((name, None if not d else (d == "true") if d in ("true", "false") else int(d)))
        assert params == table, (fam, params)
    # every struct of the header with a kernel body is in the table
    heads = re.findall(r"template <[^>]*> struct (\w+) \{(?:(?!\ntemplate <).)*?static NDWT_DEV void block\(", txt, re.S)
    assert set(heads) == set(ndwt.trace.FAMILY_PARAMS_NORMS), heads
