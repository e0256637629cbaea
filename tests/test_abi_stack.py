"""ndwt_plan_create_axes and the 'stack' option of nd_dwt_2D / nd_dwt_3D, without a GPU: the export, every refusal of a mask -- with its
code, a message that names the mask and a null handle --, the length check on the filtered axes only, and, on a machine without a GPU,
the loud failure that comes after the checks have passed.
"""
import ctypes

import numpy as np
import pytest

import ndwt_amd as ndwt

INVALID_ARG, UNKNOWN_WAVELET, FILTER_TOO_LONG, NO_DEVICE, UNSUPPORTED = 1, 2, 3, 4, 7


def _create_axes(dims, axes, names, dtype=0, cplx=0, l2=0, dil=0, maxlev=2, dev=0, ndim=None):
    lib = ndwt.lib()
    h = ctypes.c_void_p(0xdead)                               # whatever was there: a refusal leaves a null handle
    d = len(dims)
    rc = lib.ndwt_plan_create_axes(ctypes.byref(h), d if ndim is None else ndim, (ctypes.c_int64 * d)(*dims), axes,
                                   (ctypes.c_char_p * d)(*[None if n is None else n.encode() for n in names]), dtype, cplx, l2, dil, maxlev, dev)
    return rc, lib.ndwt_last_error().decode(), h


def _create(dims, names, maxlev=2):
    lib = ndwt.lib()
    h = ctypes.c_void_p(None)
    d = len(dims)
    rc = lib.ndwt_plan_create(ctypes.byref(h), d, (ctypes.c_int64 * d)(*dims), (ctypes.c_char_p * d)(*[n.encode() for n in names]), 0, 0, 0, 0, maxlev, 0)
    return rc, lib.ndwt_last_error().decode(), h


def _after_the_checks(rc, msg, h):
    """the arguments passed every check: a plan where there is a GPU, else the loud NDWT_ERR_NO_DEVICE"""
    import torch
    if torch.cuda.is_available():
        assert rc == 0 and h.value, msg
        assert ndwt.lib().ndwt_plan_destroy(h) == 0
    else:
        assert rc == NO_DEVICE and "no CPU path" in msg and not h.value


def test_plan_create_axes_is_exported_and_bound():
    assert "ndwt_plan_create_axes" in ndwt._lib.EXPORTS
    assert hasattr(ndwt.lib(), "ndwt_plan_create_axes") and ndwt.lib().ndwt_plan_create_axes.argtypes is not None
    assert len(ndwt.lib().ndwt_plan_create_axes.argtypes) == 11


@pytest.mark.parametrize("ndim,axes", [(3, 0), (3, 0b1000), (3, 0b1011), (2, 0b100), (1, 0b10), (4, 0b10000), (4, 1 << 31)])
def test_an_empty_mask_or_a_bit_beyond_the_axes_is_an_invalid_argument(ndim, axes):
    rc, msg, h = _create_axes([64] * ndim, axes, ["db2"] * ndim)
    assert rc == INVALID_ARG and f"0x{axes:x}" in msg and not h.value


@pytest.mark.parametrize("ndim", [0, 5, -1])
def test_ndim_outside_one_to_four_is_an_invalid_argument(ndim):
    rc, msg, h = _create_axes([64] * 5, 1, ["db2"] * 5, ndim=ndim)
    assert rc == INVALID_ARG and "ndim" in msg and not h.value


@pytest.mark.parametrize("ndim,axes", [(3, 0b101), (3, 0b010), (3, 0b110), (3, 0b100), (2, 0b10), (4, 0b1000), (4, 0b1011), (4, 0b0110)])
def test_a_mask_that_is_not_leading_axes_is_unsupported_and_says_so(ndim, axes):
    rc, msg, h = _create_axes([64] * ndim, axes, ["db2"] * ndim)
    assert rc == UNSUPPORTED and f"0x{axes:x}" in msg and "leading axes only" in msg and not h.value


def test_the_length_check_applies_to_filtered_axes_only():
    _after_the_checks(*_create_axes([64, 64, 3], 0b011, ["db4", "db4", "db4"]))          # 3 < 8 taps: the axis is left alone
    _after_the_checks(*_create_axes([64, 64, 3], 0b011, ["db4", "db4", None]))           # ... and its name is never read
    _after_the_checks(*_create_axes([64, 64, 1, 1], 0b0011, ["db4", "db4", None, None]))
    rc, msg, h = _create_axes([64, 6, 3], 0b011, ["db4", "db4", None])
    assert rc == FILTER_TOO_LONG and msg == "Second Dimension of Data is shorter than the wavelet filter being used" and not h.value
    rc, msg, h = _create_axes([6, 64, 3], 0b011, ["db4", "db4", None])
    assert rc == FILTER_TOO_LONG and msg == "First Dimension of Data is shorter than the wavelet filter being used" and not h.value
    rc, msg, h = _create_axes([64, 64, 0], 0b011, ["db4", "db4", None])                  # an axis left alone needs length >= 1
    assert rc == INVALID_ARG and "dims[2]" in msg and not h.value
    rc, msg, h = _create_axes([64, 64, 3], 0b011, ["db4", "coif2", None])
    assert rc == UNKNOWN_WAVELET and not h.value
    assert _create_axes([64, 64, 3], 0b011, ["db4", "db4", None], dtype=7)[0] == INVALID_ARG


def test_every_axis_filtered_is_plan_create():
    for dims, names in (([64, 64, 3], ["db4", "db4", "db4"]), ([64, 6, 30], ["db4", "db4", "db4"]), ([64, 64, 30], ["db4", "db4", "coif2"])):
        rc, msg, h = _create_axes(dims, 0b111, names)
        rc0, msg0, h0 = _create(dims, names)
        assert rc == rc0 and (rc == 0 or msg == msg0), (dims, rc, rc0, msg, msg0)
        for hh in (h, h0):
            if rc == 0:
                assert ndwt.lib().ndwt_plan_destroy(hh) == 0
            else:
                assert not hh.value
    rc, msg, _ = _create_axes([64, 64, 3], 0b111, ["db4", "db4", "db4"])
    assert rc == FILTER_TOO_LONG and msg == "Third Dimension of Data is shorter than the wavelet filter being used"


def test_no_gpu_means_a_loud_failure_after_the_checks():
    _after_the_checks(*_create_axes([64, 40, 3], 0b011, ["db2", "db2", None]))
    _after_the_checks(*_create_axes([24, 20, 18, 3], 0b0111, ["db2"] * 4))
    _after_the_checks(*_create_axes([64, 3], 0b01, ["db2", None]))                       # k = 1: the batched 1-D plan


def test_the_plan_wrapper_takes_axes_as_a_tuple_and_not_with_howmany():
    import torch
    with pytest.raises(ValueError, match="'axes' and 'howmany'"):
        ndwt.Plan([64, 40, 3], ["db2", "db2", None], torch.float32, axes=(0, 1), howmany=3)
    with pytest.raises(ValueError, match="distinct axis numbers"):
        ndwt.Plan([64, 40, 3], ["db2", "db2", None], torch.float32, axes=(0, 0))
    with pytest.raises(ndwt._lib.NdwtError, match="leading axes only") as e:
        ndwt.Plan([64, 40, 3], ["db2", "db2", "db2"], torch.float32, axes=(0, 2))
    assert e.value.code == UNSUPPORTED and "0x5" in e.value.message


def test_the_class_checks_the_stack_option_before_any_gpu_work():
    with pytest.raises(ValueError, match="'batch'"):
        ndwt.nd_dwt_1D("db1", 64, "stack", 3)
    with pytest.raises(ValueError, match="'stack' is an option of nd_dwt_2D and nd_dwt_3D"):
        ndwt.nd_dwt_4D("db1", [8, 8, 8, 8], "stack", 3)
    with pytest.raises(ValueError, match="'stack' and 'devices'"):
        ndwt.nd_dwt_2D("db1", [8, 8], "stack", 3, "compute", "hip_off", "devices", [0, 1])
    for k in (0, -2):
        with pytest.raises(ValueError, match="'stack' must be a number of items >= 1"):
            ndwt.nd_dwt_2D("db1", [8, 8], "stack", k)
        with pytest.raises(ValueError, match="'stack' must be a number of items >= 1"):
            ndwt.nd_dwt_3D("db1", [8, 8, 8], "stack", k)
    w = ndwt.nd_dwt_2D("db2", [64, 40], "stack", 3, "compute", "hip_off")
    assert w.stack == 3 and w.batch is None and w._shape == [64, 40, 3]
    for bad in (np.zeros((64, 40)), np.zeros((64, 40, 2)), np.zeros((3, 40, 64)), np.zeros((64, 40, 3, 1))):
        with pytest.raises(ValueError, match="does not match the object's sizes"):
            w.dec(bad, 2)
        with pytest.raises(ValueError, match="does not match the object's sizes"):
            w.denoise(bad, 2, 0.1)
    for bad in (np.zeros((64, 40, 3)), np.zeros((64, 40, 7)), np.zeros((64, 40, 2, 7)), np.zeros((64, 40, 7, 3))):
        with pytest.raises(ValueError, match="coefficient array must have shape"):
            w.rec(bad)
        with pytest.raises(ValueError, match="coefficient array must have shape"):
            w.shrink(bad, 0.1)
    v = ndwt.nd_dwt_3D("db2", [24, 20, 18], "stack", 2, "compute", "hip_off")
    assert v._shape == [24, 20, 18, 2]
    with pytest.raises(ValueError, match="does not match the object's sizes"):
        v.dec(np.zeros((24, 20, 18)), 1)
    with pytest.raises(ValueError, match="Second Dimension of Data is shorter"):          # the length check: filtered axes, as ever
        ndwt.nd_dwt_2D("db4", [64, 6], "stack", 3)
    plain = ndwt.nd_dwt_2D("db2", [64, 40], "compute", "hip_off")                        # without 'stack' nothing changes
    assert plain.stack is None and plain._shape == [64, 40]


def test_batch_on_the_other_classes_keeps_its_pinned_message():
    with pytest.raises(ValueError, match="'batch' is an option of nd_dwt_1D: the other classes transform one array per call"):
        ndwt.nd_dwt_2D("db1", [8, 8], "batch", 3)
    with pytest.raises(ValueError, match="'batch' is an option of nd_dwt_1D: the other classes transform one array per call"):
        ndwt.nd_dwt_3D("db1", [8, 8, 8], "batch", 3)
