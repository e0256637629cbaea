"""The joint shrinkage and the group norms without a GPU: the four exports (ndwt_shrink_joint, ndwt_denoise_joint, ndwt_group_norms,
ndwt_group_norms_dev), their declarations in include/ndwt.h and their bindings, the refusal that needs no plan, the methods and arguments
the classes gained with their argument errors, and the trace parser's table of the two new kernel families.  (The refusals that need a
plan are in tests/test_gpu_joint.py: a plan needs a device.)
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
    "ndwt_shrink_joint": "ndwt_plan* plan, void* y_dev, int64_t band_pitch, int level, const double* thresholds, int mode, void* stream",
    "ndwt_denoise_joint": "ndwt_plan* plan, const void* x_dev, void* out_dev, int level, const double* thresholds, int mode, void* stream",
    "ndwt_group_norms": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* norms, void* stream",
    "ndwt_group_norms_dev": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double* norms_dev, void* stream",
}


def test_the_four_symbols_are_exported_declared_and_bound():
    lib = ndwt.lib()
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    for name, sig in SIGNATURES.items():
        assert name in ndwt._lib.EXPORTS
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
        assert f"int {name}({sig});" in hdr, name
        assert len(getattr(lib, name).argtypes) == sig.count(",") + 1
    assert lib.ndwt_shrink_joint.argtypes[2] is ctypes.c_int64 and lib.ndwt_group_norms_dev.argtypes[2] is ctypes.c_int64
    assert list(lib.ndwt_shrink_joint.argtypes) == list(lib.ndwt_shrink_bands.argtypes)
    assert list(lib.ndwt_denoise_joint.argtypes) == list(lib.ndwt_denoise_bands.argtypes)


def test_the_header_says_what_is_not_built_and_what_a_nan_becomes():
    hdr = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    part = hdr[hdr.index("joint shrinkage across the items of a plan"):hdr.index("int ndwt_shrink_joint(")]
    for words in ("Not built:", "Den1C", "`inner` axis", "per-item weights", "a norm fused into the shrink", "MATLAB gateway", "a NaN", "explicit zero",
                  "hipEventSynchronize", "captured into a graph"):
        assert words in part, words


def test_the_calls_refuse_a_null_plan_and_write_nothing():
    lib = ndwt.lib()
    buf = ctypes.create_string_buffer(64)
    v = (ctypes.c_double * 8)(*([-1.0] * 8))
    thr = (ctypes.c_double * 8)(*([1.0] * 8))
    err = lambda: lib.ndwt_last_error().decode()
    assert lib.ndwt_shrink_joint(None, buf, 0, 1, thr, 0, None) == 1 and "null plan" in err()
    assert lib.ndwt_denoise_joint(None, buf, buf, 1, thr, 0, None) == 1 and "null plan" in err()
    assert lib.ndwt_group_norms(None, buf, 0, 1, v, None) == 1 and "null plan" in err()
    assert lib.ndwt_group_norms_dev(None, buf, 0, 1, buf, None) == 1 and "null plan" in err()
    assert list(v) == [-1.0] * 8 and buf.raw == b"\0" * 64


def test_the_methods_and_the_new_argument_exist():
    for name in ("shrink_joint", "denoise_joint", "group_norms", "group_norms_dev"):
        assert callable(getattr(ndwt.Plan, name)), name
    assert list(inspect.signature(ndwt.Plan.shrink_joint).parameters) == list(inspect.signature(ndwt.Plan.shrink_bands).parameters)
    assert list(inspect.signature(ndwt.Plan.denoise_joint).parameters) == list(inspect.signature(ndwt.Plan.denoise_bands).parameters)
    assert list(inspect.signature(ndwt.Plan.group_norms).parameters) == ["self", "y_ptr", "level", "stream", "band_pitch"]
    assert list(inspect.signature(ndwt.Plan.group_norms_dev).parameters) == ["self", "y_ptr", "level", "out_ptr", "stream", "band_pitch"]
    for cls in (ndwt.nd_dwt_1D, ndwt.nd_dwt_2D, ndwt.nd_dwt_3D, ndwt.nd_dwt_4D):
        p = inspect.signature(cls.shrink).parameters
        assert list(p) == ["self", "y", "threshold", "mode", "joint"] and p["joint"].default is False and p["mode"].default == "soft"
        p = inspect.signature(cls.denoise).parameters
        assert list(p) == ["self", "x", "level", "threshold", "mode", "joint"] and p["joint"].default is False
        assert list(inspect.signature(cls.group_norms).parameters) == ["self", "y"]
        assert inspect.signature(cls.l21_norm).parameters["weights"].default is None


def test_the_classes_refuse_a_row_per_item_a_wrong_count_and_a_wrong_shape():
    """all decided before a device is asked for"""
    w = ndwt.nd_dwt_1D("db2", 64, "batch", 5)
    level = 2
    nb = ndwt.num_bands(1, level)
    y = np.zeros((64, 5, nb))
    with pytest.raises(ValueError, match="joint=True takes a scalar or 3 thresholds"):
        w.shrink(y, np.ones((5, nb)), joint=True)
    with pytest.raises(ValueError, match="joint=True takes a scalar or 3 thresholds"):
        w.denoise(np.zeros((64, 5)), level, np.ones((5, nb)), joint=True)
    for bad in ([1.0] * (nb + 1), [1.0] * (nb - 1), np.ones((2, nb))):
        with pytest.raises(ValueError, match="threshold must be a scalar or 3 values"):
            w.shrink(y, bad, joint=True)
    with pytest.raises(ValueError, match="mode must be"):
        w.shrink(y, 1.0, "firm", joint=True)
    for bad in ([1.0] * (nb + 1), [1.0] * (nb - 1), np.ones((2, nb)), 1.0):
        with pytest.raises(ValueError, match=f"{nb} weights expected, one per band"):
            w.l21_norm(y, weights=bad)
    for f in (w.group_norms, w.l21_norm, lambda a: w.shrink(a, 1.0, joint=True)):
        for bad in (np.zeros((64, 5)), np.zeros((63, 5, nb)), np.zeros((64, 4, nb)), np.zeros((64, 5, nb, 1))):
            with pytest.raises(ValueError, match="coefficient array must have shape"):
                f(bad)


def test_a_scalar_means_every_detail_band():
    w = ndwt.nd_dwt_2D("db1", [8, 8], "stack", 4)
    assert w._joint_thresholds(0.5, 2).tolist() == [0.0] + [0.5] * 6
    assert w._joint_thresholds([3, 0, 1, 2, 0, 0, 7], 2).tolist() == [3, 0, 1, 2, 0, 0, 7]


def test_the_trace_parser_knows_the_two_families():
    r = ndwt.trace.parse_record("ndwt::JointShrink<float, 1, true, true> grid=(20,1,1) block=(256,1,1)")
    assert r.family == "JointShrink" and r.params == {"T": "float", "COMP": 1, "VEC": True, "REG": True} and r.grid == (20, 1, 1)
    r = ndwt.trace.parse_record("ndwt::JointShrink<double, 2, false, false> grid=(7,1,1) block=(256,1,1)")
    assert r.params == {"T": "double", "COMP": 2, "VEC": False, "REG": False}
    r = ndwt.trace.parse_record("ndwt::GroupNorms<double, 2, true> grid=(4,1,1) block=(256,1,1)")
    assert r.family == "GroupNorms" and r.params == {"T": "double", "COMP": 2, "VEC": True} and r.block == (256, 1, 1)
    assert set(ndwt.trace.FAMILY_PARAMS_JOINT) == {"JointShrink", "GroupNorms"}


def test_the_table_of_the_parser_matches_the_declarations():
    """FAMILY_PARAMS_JOINT against the template heads of csrc/ndwt_device_joint.h, as test_abi_norms.py holds its table to its header"""
    txt = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", "ndwt_device_joint.h")).read()
    for fam, table in ndwt.trace.FAMILY_PARAMS_JOINT.items():
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
    assert set(heads) == set(ndwt.trace.FAMILY_PARAMS_JOINT), heads
