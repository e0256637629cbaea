"""The SURE statistics and thresholds without a GPU: the five exports (ndwt_band_risk, ndwt_band_risk_items, ndwt_sure_from_risk,
ndwt_sure_thresholds, ndwt_sure_thresholds_items), their declarations in include/ndwt.h and their bindings, the enum and the
NDWT_RISK_MAX_CAND define, the refusals that need no plan, the methods the classes gained, the trace parser's table of the two new
kernel families, and ndwt_sure_from_risk -- host only -- against the formula.  (The refusals that need a plan are in
tests/test_gpu_risk.py: a plan needs a device.)
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import ndwt_amd as ndwt
from risk_cases import sure as sure_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "ndwt_band_risk": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, int nc, const double* cand, double* risk, void* stream",
    "ndwt_band_risk_items": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, int nc, const double* cand, double* risk, void* stream",
    "ndwt_sure_from_risk": "int comp, double n, double s, int nc, const double* cand, const double* risk, double* sure",
    "ndwt_sure_thresholds": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, double sigma, int rounds, double* thresholds, double* sure, "
                            "void* stream",
    "ndwt_sure_thresholds_items": "ndwt_plan* plan, const void* y_dev, int64_t band_pitch, int level, const double* sigma, int rounds, double* thresholds, "
                                  "double* sure, void* stream",
}
DP = ctypes.POINTER(ctypes.c_double)


def test_the_five_symbols_are_exported_declared_and_bound():
    lib = ndwt.lib()
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    for name, sig in SIGNATURES.items():
        assert name in ndwt._lib.EXPORTS
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
        assert f"int {name}({sig});" in hdr, name
        assert len(getattr(lib, name).argtypes) == sig.count(",") + 1
    assert lib.ndwt_band_risk.argtypes[2] is ctypes.c_int64 and lib.ndwt_band_risk.argtypes[4] is ctypes.c_int
    assert lib.ndwt_sure_thresholds.argtypes[4] is ctypes.c_double and lib.ndwt_sure_thresholds_items.argtypes[4] is DP
    assert lib.ndwt_sure_from_risk.argtypes[1] is ctypes.c_double


def test_the_enum_and_the_define():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    assert "enum { NDWT_RISK_COUNT = 0, NDWT_RISK_ENERGY = 1, NDWT_RISK_INVSUM = 2, NDWT_RISK_STATS = 3 };" in hdr
    assert "#define NDWT_RISK_MAX_CAND 8 " in hdr
    L = ndwt._lib
    assert (L.NDWT_RISK_COUNT, L.NDWT_RISK_ENERGY, L.NDWT_RISK_INVSUM, L.NDWT_RISK_STATS, L.NDWT_RISK_MAX_CAND) == (0, 1, 2, 3, 8)
    txt = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", "ndwt_device_risk.h")).read()
    assert re.search(r"constexpr int kRiskMaxCand = 8;", txt)    # the kernels are compiled for the same count


def test_the_calls_refuse_a_null_plan_and_write_nothing():
    lib = ndwt.lib()
    buf = ctypes.create_string_buffer(64)
    cand = (ctypes.c_double * 8)(*([0.5] * 8))
    v = (ctypes.c_double * 24)(*([-1.0] * 24))
    w = (ctypes.c_double * 8)(*([-2.0] * 8))
    err = lambda: lib.ndwt_last_error().decode()
    assert lib.ndwt_band_risk(None, buf, 0, 1, 8, cand, v, None) == 1 and "null plan" in err()
    assert lib.ndwt_band_risk_items(None, buf, 0, 1, 8, cand, v, None) == 1 and "null plan" in err()
    assert lib.ndwt_sure_thresholds(None, buf, 0, 1, 1.0, 3, w, v, None) == 1 and "null plan" in err()
    assert lib.ndwt_sure_thresholds_items(None, buf, 0, 1, cand, 3, w, v, None) == 1 and "null plan" in err()
    assert list(v) == [-1.0] * 24 and list(w) == [-2.0] * 8 and buf.raw == b"\0" * 64 and list(cand) == [0.5] * 8


def test_the_methods_exist():
    P = ndwt.Plan
    assert list(inspect.signature(P.band_risk).parameters) == ["self", "y_ptr", "level", "cand", "stream", "band_pitch"]
    assert list(inspect.signature(P.band_risk_items).parameters) == ["self", "y_ptr", "level", "cand", "stream", "band_pitch"]
    for name in ("sure_thresholds", "sure_thresholds_items"):
        p = inspect.signature(getattr(P, name)).parameters
        assert list(p) == ["self", "y_ptr", "level", "sigma", "rounds", "stream", "band_pitch"] and p["rounds"].default == 3, name
    assert callable(ndwt.sure_from_risk) and "sure_from_risk" in ndwt.__all__
    for cls in (ndwt.nd_dwt_1D, ndwt.nd_dwt_2D, ndwt.nd_dwt_3D, ndwt.nd_dwt_4D):
        p = inspect.signature(cls.band_risk).parameters
        assert list(p) == ["self", "y", "thresholds", "per_item"] and p["per_item"].default is False, cls.__name__
        p = inspect.signature(cls.sure_thresholds).parameters
        assert list(p) == ["self", "x", "level", "per_item", "hybrid", "rounds"], cls.__name__
        assert (p["per_item"].default, p["hybrid"].default, p["rounds"].default) == (False, True, 3)


def test_the_classes_refuse_a_wrong_coefficient_shape():
    """decided before a device is asked for"""
    w = ndwt.nd_dwt_1D("db2", 64, "batch", 5)
    nb = ndwt.num_bands(1, 2)
    for bad in (np.zeros((64, 5)), np.zeros((63, 5, nb)), np.zeros((64, 4, nb))):
        with pytest.raises(ValueError, match="coefficient array must have shape"):
            w.band_risk(bad, np.zeros((nb, 2)))


def test_the_trace_parser_knows_the_two_families():
    r = ndwt.trace.parse_record("ndwt::BandRisk<float, 1, true> grid=(20,1,1) block=(256,1,1)")
    assert r.family == "BandRisk" and r.params == {"T": "float", "COMP": 1, "VEC": True} and r.grid == (20, 1, 1)
    r = ndwt.trace.parse_record("ndwt::BandRisk<double, 2, false> grid=(7,1,1) block=(256,1,1)")
    assert r.params == {"T": "double", "COMP": 2, "VEC": False}
    for text in ("ndwt::RiskFinish<> grid=(4,1,1) block=(64,1,1)", "ndwt::RiskFinish<64> grid=(4,1,1) block=(64,1,1)"):
        r = ndwt.trace.parse_record(text)
        assert r.family == "RiskFinish" and r.params == {"NT": 64} and r.block == (64, 1, 1)
    assert set(ndwt.trace.FAMILY_PARAMS_RISK) == {"BandRisk", "RiskFinish"}


def test_the_table_of_the_parser_matches_the_declarations():
    """FAMILY_PARAMS_RISK against the template heads of csrc/ndwt_device_risk.h, as test_abi_norms.py holds its table to its header"""
    txt = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", "ndwt_device_risk.h")).read()
    for fam, table in ndwt.trace.FAMILY_PARAMS_RISK.items():
        m = re.search(r"template <([^>]*)> struct " + fam + r" \{", txt)
        assert m, fam
        params = []
        for p in m.group(1).split(","):
            decl, _, default = p.strip().partition("=")
            name = decl.split()[-1].rstrip("_")
            d = default.strip()
            params.append((name, None if not d else (d == "true") if d in ("true", "false") else int(d)))
        assert params == table, (fam, params)
    heads = re.findall(r"template <[^>]*> struct (\w+) \{(?:(?!\ntemplate <).)*?static NDWT_DEV void block\(", txt, re.S)
    assert set(heads) == set(ndwt.trace.FAMILY_PARAMS_RISK), heads


def test_the_units_are_built_and_no_kernel_is_declared_outside_the_wrapper():
    mk = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", "Makefile")).read()
    assert " ndwt_risk_f32.hip " in mk and " ndwt_risk_f64.hip " in mk and " ndwt_device_risk.h " in mk
    for f in ("ndwt_device_risk.h", "ndwt_risk_f32.hip", "ndwt_risk_f64.hip"):
        txt = open(os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", f)).read()
        assert "__global__" not in txt and "atomic" not in txt.replace("No floating-point atomics", ""), f


@pytest.mark.parametrize("comp", [1, 2])
def test_sure_from_risk_is_the_formula(comp):
    """n d s^2 + E + t^2 (n - C) - 2 s^2 (d C + (d - 1) t I), written out here; eight roundings of doubles of one sign pattern each: 1e-14"""
    rng = np.random.default_rng(5 + comp)
    n, s = 4096.0, 0.37
    t = np.sort(rng.uniform(0.0, 1.5, 8))
    C = np.sort(rng.integers(0, 4097, 8)).astype(np.float64)
    E = C * 0.05 * t
    I = (n - C) * 1.3 if comp == 2 else np.zeros(8)
    stats = np.stack([C, E, I], axis=1)
    got = ndwt.sure_from_risk(comp, n, s, t, stats)
    d = float(comp)
    want = [n * d * s * s + E[i] + t[i] * t[i] * (n - C[i]) - 2 * s * s * (d * C[i] + (d - 1) * t[i] * I[i]) for i in range(8)]
    scale = n * d * s * s + E + t * t * n + 2 * s * s * (d * n + t * I)
    assert np.all(np.abs(got - np.array(want)) <= 1e-14 * scale), (got, want)
    assert np.all(np.abs(got - sure_numpy(comp, n, s, t, stats)) <= 1e-14 * scale)
    # at t = 0 with no zeros in the block the estimate is n d s^2; at t = +inf (everything below) it is E - n d s^2
    assert ndwt.sure_from_risk(comp, n, s, [0.0], [[0.0, 0.0, 55.0]])[0] == n * d * s * s
    assert ndwt.sure_from_risk(comp, n, s, [np.inf], [[n, 700.0, 0.0]])[0] == n * d * s * s + 700.0 - 2 * s * s * d * n


def test_sure_from_risk_refuses_bad_arguments():
    lib = ndwt.lib()
    c = (ctypes.c_double * 2)(0.1, 0.2)
    r = (ctypes.c_double * 6)(*([1.0] * 6))
    out = (ctypes.c_double * 2)(-1.0, -1.0)
    err = lambda: lib.ndwt_last_error().decode()
    assert lib.ndwt_sure_from_risk(3, 10.0, 1.0, 2, c, r, out) == 1 and "comp" in err()
    assert lib.ndwt_sure_from_risk(0, 10.0, 1.0, 2, c, r, out) == 1 and "comp" in err()
    assert lib.ndwt_sure_from_risk(1, -1.0, 1.0, 2, c, r, out) == 1 and "n must" in err()
    assert lib.ndwt_sure_from_risk(1, float("nan"), 1.0, 2, c, r, out) == 1 and "n must" in err()
    assert lib.ndwt_sure_from_risk(1, 10.0, -0.5, 2, c, r, out) == 1 and "s must" in err()
    assert lib.ndwt_sure_from_risk(1, 10.0, float("inf"), 2, c, r, out) == 1 and "s must" in err()
    assert lib.ndwt_sure_from_risk(1, 10.0, 1.0, 0, c, r, out) == 1 and "nc" in err()
    assert lib.ndwt_sure_from_risk(1, 10.0, 1.0, 2, None, r, out) == 1 and "cand" in err()
    assert lib.ndwt_sure_from_risk(1, 10.0, 1.0, 2, c, None, out) == 1 and "risk" in err()
    assert lib.ndwt_sure_from_risk(1, 10.0, 1.0, 2, c, r, None) == 1 and "sure" in err()
    assert list(out) == [-1.0, -1.0]
    with pytest.raises(ValueError, match=r"risk must be a \[2, 3\] array"):
        ndwt.sure_from_risk(1, 10.0, 1.0, [0.1, 0.2], np.zeros((3, 3)))
