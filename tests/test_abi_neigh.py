"""Neighbourhood shrinkage without a GPU: the two exports (ndwt_shrink_neigh, ndwt_denoise_neigh), their declarations in include/ndwt.h and
their bindings, what the header says is not built and which overlap is allowed, the refusal that needs no plan, the methods the classes
gained, the formulas of neigh_thresholds on a hand-computed case, and the trace parser's table of the new kernel family.  (The refusals
that need a plan are in tests/test_gpu_neigh.py: a plan needs a device.)
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
    "ndwt_shrink_neigh": "ndwt_plan* plan, const void* y_dev, void* out_dev, int64_t band_pitch, int level, int radius, const double* thresholds, int mode, "
                         "void* stream",
    "ndwt_denoise_neigh": "ndwt_plan* plan, const void* x_dev, void* out_dev, int level, int radius, const double* thresholds, int mode, void* stream",
}


def test_the_two_symbols_are_exported_declared_and_bound():
    lib = ndwt.lib()
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    for name, sig in SIGNATURES.items():
        assert name in ndwt._lib.EXPORTS
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
        assert f"int {name}({sig});" in hdr, name
        assert len(getattr(lib, name).argtypes) == sig.count(",") + 1
    assert lib.ndwt_shrink_neigh.argtypes[3] is ctypes.c_int64
    assert lib.ndwt_shrink_neigh.argtypes[6] is lib.ndwt_denoise_neigh.argtypes[5] is ctypes.POINTER(ctypes.c_double)


def test_the_header_says_what_is_not_built_and_which_overlap_is_allowed():
    hdr = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    part = hdr[hdr.index("neighbourhood shrinkage: the energy of a small window"):hdr.index("int ndwt_shrink_neigh(")]
    assert part.rstrip(" /").endswith("MATLAB gateway.")         # the block ends with "Not built:"
    tail = part[part.index("Not built:"):]
    for words in ("interleaved plans", "four filtered axes", "a threshold row per item", "a window across levels (parent and child)",
                  "the window sum as an output of its own", "a statistic fused in", "the handles, the slab entry points and the MATLAB gateway"):
        assert words in tail, words
    for words in ("out_dev == y_dev - band_pitch", "out_dev overlaps y_dev", "never writes y_dev", "never writes the scalars between the bands",
                  "one launch per band in stream order", "one device-to-device copy", "nb + 1 band slots", "items_table_upload", "hipEventSynchronize",
                  "captured into a graph", "explicit zero", "a NaN", "no running sum", "formed on the host", "4.50524", "count an element twice",
                  "`inner` elements apart"):
        assert words in part, words


def test_the_calls_refuse_a_null_plan_and_write_nothing():
    lib = ndwt.lib()
    buf, out = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    thr = (ctypes.c_double * 8)(*([1.0] * 8))
    err = lambda: lib.ndwt_last_error().decode()
    assert lib.ndwt_shrink_neigh(None, buf, out, 0, 1, 1, thr, 0, None) == 1 and "null plan" in err()
    assert lib.ndwt_denoise_neigh(None, buf, out, 1, 1, thr, 0, None) == 1 and "null plan" in err()
    assert buf.raw == b"\0" * 64 and out.raw == b"\0" * 64 and list(thr) == [1.0] * 8


def test_the_methods_exist_and_the_old_signatures_stay():
    assert list(inspect.signature(ndwt.Plan.shrink_neigh).parameters) == ["self", "y_ptr", "out_ptr", "level", "thresholds", "radius", "hard", "stream", "band_pitch"]
    assert list(inspect.signature(ndwt.Plan.denoise_neigh).parameters) == ["self", "x_ptr", "out_ptr", "level", "thresholds", "radius", "hard", "stream"]
    for f in (ndwt.Plan.shrink_neigh, ndwt.Plan.denoise_neigh):
        p = inspect.signature(f).parameters
        assert p["radius"].default == 1 and p["hard"].default is False and p["stream"].default == 0
    assert inspect.signature(ndwt.Plan.shrink_neigh).parameters["band_pitch"].default == 0
    for cls in (ndwt.nd_dwt_1D, ndwt.nd_dwt_2D, ndwt.nd_dwt_3D, ndwt.nd_dwt_4D):
        p = inspect.signature(cls.shrink_neigh).parameters
        assert list(p) == ["self", "y", "threshold", "radius", "mode"] and p["radius"].default == 1 and p["mode"].default == "soft"
        p = inspect.signature(cls.denoise_neigh).parameters
        assert list(p) == ["self", "x", "level", "threshold", "radius", "mode"] and p["radius"].default == 1 and p["mode"].default == "soft"
        p = inspect.signature(cls.neigh_thresholds).parameters
        assert list(p) == ["self", "x", "level", "radius", "rule"] and p["radius"].default == 1 and p["rule"].default == "universal"
        # no argument was added to shrink or denoise
        assert list(inspect.signature(cls.shrink).parameters) == ["self", "y", "threshold", "mode", "joint"]
        assert list(inspect.signature(cls.denoise).parameters) == ["self", "x", "level", "threshold", "mode", "joint"]


def test_the_classes_refuse_a_wrong_mode_count_and_shape_before_a_device_is_asked_for():
    w = ndwt.nd_dwt_1D("db2", 64, "batch", 5)
    nb = ndwt.num_bands(1, 2)
    y = np.zeros((64, 5, nb))
    with pytest.raises(ValueError, match="mode must be"):
        w.shrink_neigh(y, 1.0, 1, "firm")
    with pytest.raises(ValueError, match="mode must be"):
        w.denoise_neigh(np.zeros((64, 5)), 2, 1.0, 1, "firm")
    for bad in ([1.0] * (nb + 1), [1.0] * (nb - 1), np.ones((2, nb))):
        with pytest.raises(ValueError, match="threshold must be a scalar or 3 values"):
            w.shrink_neigh(y, bad)
    with pytest.raises(ValueError, match="takes a scalar or 3 thresholds"):
        w.shrink_neigh(y, np.ones((5, nb)))                      # a row per item: not built
    for bad in (np.zeros((64, 5)), np.zeros((63, 5, nb)), np.zeros((64, 5, nb, 1))):
        with pytest.raises(ValueError, match="coefficient array must have shape"):
            w.shrink_neigh(bad, 1.0)


def test_the_three_rules_on_a_hand_computed_case():
    """sigma = 2, gains 1, 0.5, 0.25, a 16 x 16 item (N = 256, ln N = 8 ln 2), radius 1: M = 9"""
    f = ndwt.api.neigh_threshold_row
    gains = [1.0, 0.5, 0.25]
    s = np.array([0.0, 1.0, 0.5])                                # sigma * gain, entry 0 dropped
    assert np.allclose(f(2.0, gains, [16, 16], 1, "universal"), s * np.sqrt(16 * np.log(2.0)), rtol=1e-15)
    assert f(2.0, gains, [16, 16], 1, "wiener").tolist() == [0.0, 3.0, 1.5]                 # t^2 = 9 s^2
    assert np.allclose(f(2.0, gains, [16, 16], 1, "block") ** 2, 4.50524 * 9 * s * s, rtol=1e-15)
    assert f(2.0, gains, [16, 16], 2, "wiener").tolist() == [0.0, 5.0, 2.5]                 # M = 25
    assert f(2.0, gains, [16], 3, "wiener").tolist() == [0.0, np.sqrt(7.0), np.sqrt(7.0) / 2]   # one axis: M = 7
    assert f(2.0, gains, [4, 4, 4], 1, "wiener").tolist() == [0.0, np.sqrt(27.0), np.sqrt(27.0) / 2]
    lam = 4.50524
    assert abs(lam - np.log(lam) - 3.0) < 1e-5                   # Cai and Silverman's constant: the root of lambda - ln lambda = 3
    with pytest.raises(ValueError, match="rule must be"):
        f(2.0, gains, [16, 16], 1, "sure")
    with pytest.raises(ValueError, match="radius must be"):
        f(2.0, gains, [16, 16], 4, "wiener")


def test_the_trace_parser_knows_the_family():
    r = ndwt.trace.parse_record("ndwt::NeighShrink<float, 1, 3, 2> grid=(2048,1,1) block=(256,1,1)")
    assert r.family == "NeighShrink" and r.params == {"T": "float", "COMP": 1, "ND": 3, "R": 2} and r.grid == (2048, 1, 1) and r.block == (256, 1, 1)
    r = ndwt.trace.parse_record("ndwt::NeighShrink<double, 2, 1, 3> grid=(7,1,1) block=(256,1,1)")
    assert r.params == {"T": "double", "COMP": 2, "ND": 1, "R": 3}
    assert set(ndwt.trace.FAMILY_PARAMS_NEIGH) == {"NeighShrink"}


def test_the_table_of_the_parser_matches_the_declaration():
    """FAMILY_PARAMS_NEIGH against the template heads of csrc/ndwt_device_neigh.h, as test_abi_joint.py holds its table to its header"""
    txt = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", "ndwt_device_neigh.h")).read()
    for fam, table in ndwt.trace.FAMILY_PARAMS_NEIGH.items():
        m = re.search(r"template <([^>]*)> struct " + fam + r" \{", txt)
        assert m, fam
        params = [(p.strip().split()[-1].rstrip("_"), None) for p in m.group(1).split(",")]
        assert params == table, (fam, params)
    heads = re.findall(r"template <[^>]*> struct (\w+) \{(?:(?!\ntemplate <).)*?static NDWT_DEV void block\(", txt, re.S)
    assert set(heads) == set(ndwt.trace.FAMILY_PARAMS_NEIGH), heads
    # the launch units instantiate all 36
    for unit, T in (("ndwt_neigh_f32.hip", "float"), ("ndwt_neigh_f64.hip", "double")):
        src = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", unit)).read()
        assert sorted(re.findall(r"NDWT_LAUNCH_NEIGH_R\(" + T + r", (\d), (\d)\)", src)) == [(c, d) for c in "12" for d in "123"], unit
    mk = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", "Makefile")).read()
    assert "ndwt_neigh_f32.hip" in mk and "ndwt_neigh_f64.hip" in mk and "ndwt_device_neigh.h" in mk
