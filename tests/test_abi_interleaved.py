"""ndwt_plan_create_interleaved, Plan(inner=...) / Plan(axes=(a, ..)) with a > 0 and the 'inner' option of nd_dwt_1D / 2D / 3D, without
a GPU: the export and its binding, every refusal of an argument -- with its code, a message that names the argument and a null handle
--, the reference's length checks on `dims` only, and, on a machine without a GPU, the loud failure that comes after the checks.
"""
import ctypes

import numpy as np
import pytest

import ndwt_amd as ndwt

INVALID_ARG, UNKNOWN_WAVELET, FILTER_TOO_LONG, NO_DEVICE, UNSUPPORTED = 1, 2, 3, 4, 7


def _create(dims, inner, howmany, names, dtype=0, cplx=0, l2=0, dil=0, maxlev=2, dev=0, ndim=None, null_dims=False, null_names=False):
    lib = ndwt.lib()
    h = ctypes.c_void_p(0xdead)                               # whatever was there: a refusal leaves a null handle
    d = len(dims)
    dims_c = None if null_dims else (ctypes.c_int64 * d)(*dims)
    names_c = None if null_names else (ctypes.c_char_p * d)(*[None if n is None else n.encode() for n in names])
    rc = lib.ndwt_plan_create_interleaved(ctypes.byref(h), d if ndim is None else ndim, dims_c, inner, howmany, names_c, dtype, cplx, l2, dil,
                                          maxlev, dev)
    return rc, lib.ndwt_last_error().decode(), h


def _after_the_checks(rc, msg, h):
    """the arguments passed every check: a plan where there is a GPU, else the loud NDWT_ERR_NO_DEVICE"""
    import torch
    if torch.cuda.is_available():
        assert rc == 0 and h.value, msg
        assert ndwt.lib().ndwt_plan_destroy(h) == 0
    else:
        assert rc == NO_DEVICE and "no CPU path" in msg and not h.value


def test_plan_create_interleaved_is_exported_and_bound():
    assert "ndwt_plan_create_interleaved" in ndwt._lib.EXPORTS
    f = ndwt.lib().ndwt_plan_create_interleaved
    assert f.argtypes is not None and len(f.argtypes) == 12
    assert f.argtypes[3] is ctypes.c_int64 and f.argtypes[4] is ctypes.c_int64      # inner, howmany


@pytest.mark.parametrize("inner", [0, -1, -(1 << 40)])
def test_inner_below_one_is_an_invalid_argument(inner):
    rc, msg, h = _create([64], inner, 3, ["db2"])
    assert rc == INVALID_ARG and "inner" in msg and str(inner) in msg and not h.value


@pytest.mark.parametrize("howmany", [0, -1])
def test_howmany_below_one_is_an_invalid_argument(howmany):
    rc, msg, h = _create([64], 4, howmany, ["db2"])
    assert rc == INVALID_ARG and "howmany" in msg and str(howmany) in msg and not h.value


@pytest.mark.parametrize("ndim", [0, 5, -1])
def test_ndim_outside_one_to_four_is_an_invalid_argument(ndim):
    rc, msg, h = _create([64] * 5, 4, 3, ["db2"] * 5, ndim=ndim)
    assert rc == INVALID_ARG and "ndim" in msg and not h.value


def test_the_other_arguments_are_checked_as_for_every_plan():
    assert _create([64], 4, 3, ["db2"], null_dims=True)[0] == INVALID_ARG
    assert _create([64], 4, 3, ["db2"], null_names=True)[0] == INVALID_ARG
    assert _create([64], 4, 3, ["db2"], dtype=7)[0] == INVALID_ARG
    assert _create([64], 4, 3, ["db2"], cplx=5)[0] == INVALID_ARG
    assert _create([64], 4, 3, ["db2"], dil=9)[0] == INVALID_ARG
    assert _create([64], 4, 3, ["db2"], maxlev=0)[0] == INVALID_ARG
    rc, msg, h = _create([64, 0], 4, 3, ["db2", "db2"])
    assert rc == INVALID_ARG and "dims[1]" in msg and not h.value
    rc, msg, h = _create([64], 4, 3, ["coif2"])
    assert rc == UNKNOWN_WAVELET and msg == "Unknown Wavelet Name" and not h.value
    lib = ndwt.lib()
    assert lib.ndwt_plan_create_interleaved(None, 1, (ctypes.c_int64 * 1)(64), 4, 3, (ctypes.c_char_p * 1)(b"db2"), 0, 0, 0, 0, 2, 0) == INVALID_ARG


def test_the_length_checks_are_the_references_and_apply_to_dims_only():
    _after_the_checks(*_create([8], 2, 1, ["db4"]))                                      # inner = 2 and one item: neither is an axis
    _after_the_checks(*_create([8, 9], 3, 2, ["db4", "db4"]))
    for a, word in enumerate(["First", "Second", "Third", "Fourth"]):
        dims = [16] * 4
        dims[a] = 7                                                                      # 7 < 8 taps
        rc, msg, h = _create(dims, 64, 64, ["db4"] * 4)
        assert rc == FILTER_TOO_LONG and msg == f"{word} Dimension of Data is shorter than the wavelet filter being used" and not h.value


def test_no_gpu_means_a_loud_failure_after_the_checks():
    _after_the_checks(*_create([19], 8, 6, ["db2"]))
    _after_the_checks(*_create([24, 20], 3, 2, ["db2", "db4"], cplx=1, dtype=1))
    _after_the_checks(*_create([12, 10, 9], 4, 2, ["db2"] * 3, dil=1))
    _after_the_checks(*_create([8, 8, 8, 8], 2, 1, ["db1"] * 4))
    _after_the_checks(*_create([64, 40], 1, 3, ["db2", "db2"]))                           # inner = 1: the stack plan


def _plan_outcome(make):
    """Plan(...) on this machine: the handle's plan where there is a GPU, else NDWT_ERR_NO_DEVICE -- either way the checks passed"""
    import torch
    if torch.cuda.is_available():
        return make()
    with pytest.raises(ndwt._lib.NdwtError, match="no CPU path") as e:
        make()
    assert e.value.code == NO_DEVICE
    return None


def test_plan_axes_that_do_not_start_at_zero_reach_the_new_entry_point():
    import torch
    # time only of a dynamic series [nx, ny, nt]: the names of the axes left alone are ignored, their lengths are not checked
    p = _plan_outcome(lambda: ndwt.Plan([6, 5, 19], [None, "nonsense", "db4"], torch.float32, axes=(2,)))
    if p is not None:
        assert (p.inner, p.howmany) == (30, 1) and p.describe().startswith("interleaved")
    p = _plan_outcome(lambda: ndwt.Plan([3, 24, 20], [None, "db2", "db4"], torch.float32, axes=(1, 2)))
    if p is not None:
        assert (p.inner, p.howmany) == (3, 1)
    p = _plan_outcome(lambda: ndwt.Plan([4, 24, 20, 5], [None, "db2", "db4", None], torch.float64, axes=(2, 1)))
    if p is not None:
        assert (p.inner, p.howmany) == (4, 5)
    with pytest.raises(ndwt._lib.NdwtError, match="Second Dimension of Data is shorter") as e:      # of the ITEM: whole axis 2
        ndwt.Plan([3, 24, 6], [None, "db2", "db4"], torch.float32, axes=(1, 2))
    assert e.value.code == FILTER_TOO_LONG
    with pytest.raises(ndwt._lib.NdwtError, match="leading axes only") as e:                        # the pinned refusal stays
        ndwt.Plan([64, 40, 3], ["db2", "db2", "db2"], torch.float32, axes=(0, 2))
    assert e.value.code == UNSUPPORTED and "0x5" in e.value.message
    with pytest.raises(ndwt._lib.NdwtError, match="leading axes only"):                             # not adjacent: no run of axes
        ndwt.Plan([8, 8, 8, 8], ["db1"] * 4, torch.float32, axes=(1, 3))
    with pytest.raises(ndwt._lib.NdwtError) as e:                                                   # an axis beyond the array
        ndwt.Plan([64, 40], ["db2", "db2"], torch.float32, axes=(2,))
    assert e.value.code == INVALID_ARG


def test_plan_inner_calls_the_new_entry_point_and_not_with_axes():
    import torch
    with pytest.raises(ValueError, match="'axes' and 'inner'"):
        ndwt.Plan([64, 40, 3], ["db2", "db2", None], torch.float32, axes=(0, 1), inner=2)
    with pytest.raises(ValueError, match="not a slab plan"):
        ndwt.Plan([64, 40], ["db2", "db2"], torch.float32, inner=2, global_outer=80)
    with pytest.raises(ndwt._lib.NdwtError, match="inner must be >= 1") as e:
        ndwt.Plan([64], ["db2"], torch.float32, inner=0, howmany=3)
    assert e.value.code == INVALID_ARG
    with pytest.raises(ndwt._lib.NdwtError, match="howmany must be >= 1"):
        ndwt.Plan([64], ["db2"], torch.float32, inner=4, howmany=0)
    p = _plan_outcome(lambda: ndwt.Plan([19], ["db2"], torch.float32, inner=8, howmany=6))
    if p is not None:
        assert (p.inner, p.howmany) == (8, 6)


def test_the_classes_check_the_inner_option_before_any_gpu_work():
    with pytest.raises(ValueError, match="'inner' is an option of nd_dwt_1D, nd_dwt_2D and nd_dwt_3D"):
        ndwt.nd_dwt_4D("db1", [8, 8, 8, 8], "inner", 3)
    with pytest.raises(ValueError, match="'inner' and 'devices'"):
        ndwt.nd_dwt_2D("db1", [8, 8], "inner", 3, "compute", "hip_off", "devices", [0, 1])
    for bad in (0, -2, [4, 0], []):
        with pytest.raises(ValueError, match="'inner' must be a number of elements >= 1"):
            ndwt.nd_dwt_1D("db1", 8, "inner", bad)
        with pytest.raises(ValueError, match="'inner' must be a number of elements >= 1"):
            ndwt.nd_dwt_3D("db1", [8, 8, 8], "inner", bad)
    w = ndwt.nd_dwt_1D("db2", 19, "inner", [4, 2], "batch", 3, "compute", "hip_off")
    assert w.inner == [4, 2] and w._shape == [4, 2, 19, 3]
    w = ndwt.nd_dwt_1D("db2", 19, "inner", 8, "compute", "hip_off")
    assert w._shape == [8, 19]
    for bad in (np.zeros(19), np.zeros((19, 8)), np.zeros((8, 19, 1)), np.zeros((1, 19))):
        with pytest.raises(ValueError, match="does not match the object's sizes"):
            w.dec(bad, 2)
        with pytest.raises(ValueError, match="does not match the object's sizes"):
            w.denoise(bad, 2, 0.1)
    for bad in (np.zeros((8, 19)), np.zeros((19, 8, 3)), np.zeros((8, 19, 3, 1))):
        with pytest.raises(ValueError, match="coefficient array must have shape"):
            w.rec(bad)
        with pytest.raises(ValueError, match="coefficient array must have shape"):
            w.shrink(bad, 0.1)
    v = ndwt.nd_dwt_2D("db2", [24, 20], "inner", 3, "stack", 2, "compute", "hip_off")
    assert v._shape == [3, 24, 20, 2]
    with pytest.raises(ValueError, match="First Dimension of Data is shorter"):          # the length check: the filtered axes, as ever
        ndwt.nd_dwt_2D("db4", [6, 64], "inner", 300)
    plain = ndwt.nd_dwt_1D("db2", 19, "compute", "hip_off")                              # without 'inner' nothing changes
    assert plain.inner is None and plain._shape == [19]
