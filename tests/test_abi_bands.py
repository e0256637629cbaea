"""Per-band thresholds without a GPU: the three exports (ndwt_band_gains, ndwt_shrink_bands, ndwt_denoise_bands), ndwt_band_gains against
the numpy oracle -- the l2 norm of every band of spatial_dec(unit impulse), relative error <= 1e-12 -- every argument refusal of
ndwt_band_gains with its message, the plan calls on a null plan, and the classes' check of a threshold sequence's length.
"""
import ctypes

import numpy as np
import pytest

import helpers
import ndwt_amd as ndwt
import ndwt_oracle as orc

NEW = ("ndwt_band_gains", "ndwt_shrink_bands", "ndwt_denoise_bands")


def test_the_three_symbols_are_exported_and_bound():
    lib = ndwt.lib()
    for name in NEW:
        assert name in ndwt._lib.EXPORTS
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name


def _oracle_gains(dims, wnames, level, l2, dilation="reference"):
    e = np.zeros(dims)
    e[(0,) * len(dims)] = 1.0
    y = orc.spatial_dec(e, wnames, level, l2, dilation)
    return np.sqrt((y ** 2).reshape(-1, y.shape[-1]).sum(axis=0))


# (id, dims, wavelet per axis, levels, pres_l2_norm, dilation)
GAIN_CASES = [
    ("1d-db4-l4", [256], ["db4"], 4, 0, "reference"),
    ("1d-db4-l4-l2norm", [256], ["db4"], 4, 1, "reference"),
    ("1d-n8-db4-l3-wraps", [8], ["db4"], 3, 1, "reference"),          # the equivalent filter (22 taps) is longer than the axis
    ("2d-32x32-db2-db3-l2", [32, 32], ["db2", "db3"], 2, 1, "reference"),
    ("3d-16-db1", [16, 16, 16], ["db1"] * 3, 2, 0, "reference"),
    ("1d-atrous-n64-db2-l3", [64], ["db2"], 3, 1, "atrous"),
    # a-trous on axes shorter than the dilated filter: it goes round the axis more than once, two taps land on one sample
    ("1d-atrous-n8-db4-l3-wraps", [8], ["db4"], 3, 1, "atrous"),
    ("1d-atrous-n10-db5-l4-wraps", [10], ["db5"], 4, 0, "atrous"),
    ("3d-atrous-8-db4-l3-wraps", [8, 8, 8], ["db4"] * 3, 3, 1, "atrous"),
    ("2d-atrous-12x6-db3-l4-wraps", [12, 6], ["db3", "db3"], 4, 1, "atrous"),
]


@pytest.mark.parametrize("cid,dims,wn,level,l2,dil", GAIN_CASES, ids=[c[0] for c in GAIN_CASES])
def test_band_gains_are_the_band_norms_of_the_oracles_impulse_response(cid, dims, wn, level, l2, dil):
    got = ndwt.band_gains(dims, wn, level, pres_l2_norm=l2, dilation=dil)
    want = _oracle_gains(dims, wn, level, l2, dil)
    assert got.shape == want.shape == (orc.num_bands(len(dims), level),)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{cid}: gains {np.array2string(got, precision=4)}, relative error {err:.3g}")
    assert np.abs(got / want - 1).max() <= 1e-12


# a tap stride that is a multiple of an axis: every tap lands on one sample, the high-pass taps sum to zero, and the bands that are
# high-pass on that axis are identically zero in exact arithmetic (helpers.zero_bands).  Both sides return rounding noise there: those
# bands are compared absolutely, against the largest gain, the others relatively as above
ZERO_GAIN_CASES = [
    ("1d-atrous-n8-db4-l5", [8], ["db4"], 5, 1, 2),                               # the details of levels 4 and 5
    ("4d-atrous-6x4x5x4-l3", [6, 4, 5, 4], ["db3", "db2", "db2", "db1"], 3, 0, 12),   # level 3 (stride 4): high-pass on y or t
]


@pytest.mark.parametrize("cid,dims,wn,level,l2,nzero", ZERO_GAIN_CASES, ids=[c[0] for c in ZERO_GAIN_CASES])
def test_band_gains_where_the_tap_stride_is_a_multiple_of_an_axis(cid, dims, wn, level, l2, nzero):
    got = ndwt.band_gains(dims, wn, level, pres_l2_norm=l2, dilation="atrous")
    want = _oracle_gains(dims, wn, level, l2, "atrous")
    zero = helpers.zero_bands(dims, level, "atrous")
    assert got.shape == want.shape == zero.shape and int(zero.sum()) == nzero
    print(f"{cid}: zero bands: got {np.abs(got[zero]).max():.3g}, oracle {np.abs(want[zero]).max():.3g}; "
          f"the others: relative error {np.abs(got[~zero] / want[~zero] - 1).max():.3g}")
    assert np.abs(want[zero]).max() <= 1e-12 * want.max()                             # the oracle agrees that they are zero
    assert np.abs(got[zero] - want[zero]).max() <= 1e-12 * want.max()
    assert np.abs(got[~zero] / want[~zero] - 1).max() <= 1e-12


def test_the_figures_users_are_told():
    """what include/ndwt.h quotes: db4, 4 levels, pres_l2_norm -- a factor of 5 between the level-4 and the level-1 details"""
    g = ndwt.band_gains([4096], "db4", 4, pres_l2_norm=1)
    assert np.allclose(g, [0.620, 0.143, 0.178, 0.252, 0.707], atol=5e-4)
    g2 = ndwt.band_gains([64, 64], "db2", 2, pres_l2_norm=1)
    assert abs(g2.max() - 0.5) < 1e-12 and abs(g2.min() - 0.090) < 5e-4


def _gains_raw(ndim, dims, names, l2=0, dil=0, level=2, out=True):
    lib = ndwt.lib()
    g = (ctypes.c_double * 64)()
    d = None if dims is None else (ctypes.c_int64 * len(dims))(*dims)
    n = None if names is None else (ctypes.c_char_p * len(names))(*[None if w is None else w.encode() for w in names])
    rc = lib.ndwt_band_gains(ndim, d, n, l2, dil, level, g if out else None)
    return rc, lib.ndwt_last_error().decode()


def test_every_argument_refusal_of_band_gains_with_its_message():
    assert _gains_raw(1, [64], ["db2"]) [0] == 0
    for ndim in (0, 5, -1):
        assert _gains_raw(ndim, [64] * 5, ["db2"] * 5) == (1, "ndim must be 1..4")
    assert _gains_raw(1, None, ["db2"]) == (1, "null dims/wnames")
    assert _gains_raw(1, [64], None) == (1, "null dims/wnames")
    assert _gains_raw(1, [64], ["db2"], out=False) == (1, "null output pointer")
    assert _gains_raw(1, [64], ["db2"], dil=2) == (1, "bad dilation mode")
    for level in (0, -3, 31):
        assert _gains_raw(1, [64], ["db2"], level=level) == (1, "level must be 1..30")
    assert _gains_raw(2, [64, 0], ["db2", "db2"]) == (1, "dims[1] must be >= 1")
    assert _gains_raw(1, [64], ["coif2"]) == (2, "Unknown Wavelet Name")
    assert _gains_raw(2, [64, 64], ["db2", None]) == (2, "Unknown Wavelet Name")
    assert _gains_raw(1, [6], ["db4"]) == (3, "First Dimension of Data is shorter than the wavelet filter being used")
    assert _gains_raw(3, [16, 16, 3], ["db1", "db1", "db2"]) == (3, "Third Dimension of Data is shorter than the wavelet filter being used")
    with pytest.raises(ValueError, match="wavelet names"):
        ndwt.band_gains([64, 64], ["db2"], 2)
    with pytest.raises(ndwt.NdwtError, match="Unknown Wavelet Name"):
        ndwt.band_gains([64], "sym4", 2)


def test_the_plan_calls_refuse_a_null_plan():
    lib = ndwt.lib()
    thr = (ctypes.c_double * 8)(*[0.1] * 8)
    buf = ctypes.create_string_buffer(64)
    assert lib.ndwt_shrink_bands(None, buf, 0, 1, thr, 0, None) == 1 and "null plan" in lib.ndwt_last_error().decode()
    assert lib.ndwt_denoise_bands(None, buf, buf, 1, thr, 0, None) == 1 and "null plan" in lib.ndwt_last_error().decode()


def test_the_classes_check_the_length_of_a_threshold_sequence_before_any_gpu_work():
    w = ndwt.nd_dwt_1D("db2", 64, "batch", 3, "compute", "hip_off")
    with pytest.raises(ValueError, match="4 values, one per band of a 3-level transform"):
        w.denoise(np.zeros((64, 3)), 3, [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="4 values, one per band of a 3-level transform"):
        w.shrink(np.zeros((64, 3, 4)), np.full(5, 0.1))
    w2 = ndwt.nd_dwt_2D("db1", [8, 8], "compute", "hip_off")
    with pytest.raises(ValueError, match="7 values, one per band of a 2-level transform"):
        w2.denoise(np.zeros((8, 8)), 2, [0.1] * 4)
    g = w2.band_gains(2)
    assert g.shape == (7,) and np.allclose(g, _oracle_gains([8, 8], ["db1", "db1"], 2, 0))
    assert np.allclose(w.band_gains(3), _oracle_gains([64], ["db2"], 3, 0))
