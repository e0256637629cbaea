"""ndwt_plan_create_many and the 'batch' option of nd_dwt_1D, without a GPU: the export, the argument checks that come before any device
call, and -- on a machine without a GPU -- the loud failure instead of a fallback.
"""
import ctypes

import pytest

import ndwt_amd as ndwt


def _create_many(dims, howmany, names, dtype=0, cplx=0, l2=0, dil=0, maxlev=2, dev=0):
    lib = ndwt.lib()
    h = ctypes.c_void_p(None)
    d = len(dims)
    rc = lib.ndwt_plan_create_many(ctypes.byref(h), d, (ctypes.c_int64 * d)(*dims), howmany, (ctypes.c_char_p * d)(*[n.encode() for n in names]),
                                   dtype, cplx, l2, dil, maxlev, dev)
    return rc, lib.ndwt_last_error().decode(), h


def test_plan_create_many_is_exported_and_bound():
    assert "ndwt_plan_create_many" in ndwt._lib.EXPORTS
    assert hasattr(ndwt.lib(), "ndwt_plan_create_many") and ndwt.lib().ndwt_plan_create_many.argtypes is not None


@pytest.mark.parametrize("howmany", [0, -1, -(1 << 40)])
def test_howmany_below_one_is_an_invalid_argument(howmany):
    rc, msg, h = _create_many([64], howmany, ["db2"])
    assert rc == 1 and "howmany" in msg and not h.value


@pytest.mark.parametrize("ndim", [2, 3, 4])
def test_more_than_one_dimension_is_unsupported_and_says_so(ndim):
    rc, msg, h = _create_many([64] * ndim, 3, ["db2"] * ndim)
    assert rc == 7 and "1-D" in msg and f"ndim = {ndim}" in msg and not h.value


def test_the_other_argument_checks_are_those_of_a_plan():
    assert _create_many([64] * 5, 3, ["db2"] * 5)[0] == 1
    rc, msg, _ = _create_many([6], 3, ["db4"])
    assert rc == 3 and msg == "First Dimension of Data is shorter than the wavelet filter being used"
    assert _create_many([64], 3, ["coif2"])[0] == 2
    assert _create_many([64], 3, ["db2"], dtype=7)[0] == 1


def test_no_gpu_means_a_loud_failure_not_a_fallback():
    import torch
    rc, msg, h = _create_many([64], 3, ["db2"])
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        assert ndwt.lib().ndwt_plan_destroy(h) == 0
    else:
        assert rc == 4 and "no CPU path" in msg and not h.value


def test_the_class_checks_the_batch_option_before_any_gpu_work():
    import numpy as np
    with pytest.raises(ValueError, match="'batch' is an option of nd_dwt_1D"):
        ndwt.nd_dwt_2D("db1", [8, 8], "batch", 3)
    with pytest.raises(ValueError, match="'batch' is an option of nd_dwt_1D"):
        ndwt.nd_dwt_3D("db1", [8, 8, 8], "batch", 3)
    with pytest.raises(ValueError, match="devices"):
        ndwt.nd_dwt_1D("db1", 64, "batch", 3, "compute", "hip_off", "devices", [0, 1])
    with pytest.raises(ValueError, match="'batch' must be a number of signals >= 1"):
        ndwt.nd_dwt_1D("db1", 64, "batch", 0)
    w = ndwt.nd_dwt_1D("db2", 64, "batch", 3, "compute", "hip_off")
    for bad in (np.zeros(64), np.zeros((64, 2)), np.zeros((3, 64)), np.zeros((64, 3, 1))):
        with pytest.raises(ValueError, match="does not match the object's sizes"):
            w.dec(bad, 2)
    with pytest.raises(ValueError, match="coefficient array must have shape"):
        w.rec(np.zeros((64, 3)))
    with pytest.raises(ValueError, match="coefficient array must have shape"):
        w.rec(np.zeros((64, 2, 3)))
    plain = ndwt.nd_dwt_1D("db2", 64, "compute", "hip_off")           # without 'batch' nothing changes: [n], [n, 1], [1, n]
    assert plain.batch is None and plain._shape == [64]
    for ok in (np.zeros(64), np.zeros((64, 1)), np.zeros((1, 64))):
        assert list(plain._prep_dec_input(ok).shape) == [64]
