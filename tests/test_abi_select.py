"""Order statistics of a band and the noise estimate without a GPU: the three exports (ndwt_band_select, ndwt_estimate_sigma_coef,
ndwt_estimate_sigma) and their bindings, the refusals that need no plan, the methods the classes gained, and the host-side decisions of
csrc/ndwt_select.h (asked through tests/select/bandselect_shim.cpp) on both sides of every condition: passes and digits per data kind,
the 4-scalar or the element-wise form, the grid with and without target_blocks, the 2^32 refusal.  (The refusals that need a plan --
band, nk, k[i] out of range -- are in tests/test_gpu_select.py: a plan needs a device.)
"""
import ctypes

import pytest

import ndwt_amd as ndwt
from select_cases import build_shim

NEW = ("ndwt_band_select", "ndwt_estimate_sigma_coef", "ndwt_estimate_sigma")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory)


def test_the_three_symbols_are_exported_and_bound():
    lib = ndwt.lib()
    for name in NEW:
        assert name in ndwt._lib.EXPORTS
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert len(lib.ndwt_band_select.argtypes) == 9
    assert len(lib.ndwt_estimate_sigma_coef.argtypes) == 6 and len(lib.ndwt_estimate_sigma.argtypes) == 4


def test_the_calls_refuse_a_null_plan():
    lib = ndwt.lib()
    buf = ctypes.create_string_buffer(64)
    k = (ctypes.c_int64 * 4)(0, 0, 0, 0)
    v = (ctypes.c_double * 4)()
    s = ctypes.c_double(-1.0)
    assert lib.ndwt_band_select(None, buf, 0, 1, 0, 1, k, v, None) == 1 and "null plan" in lib.ndwt_last_error().decode()
    assert lib.ndwt_estimate_sigma_coef(None, buf, 0, 1, ctypes.byref(s), None) == 1 and "null plan" in lib.ndwt_last_error().decode()
    assert lib.ndwt_estimate_sigma(None, buf, ctypes.byref(s), None) == 1 and "null plan" in lib.ndwt_last_error().decode()
    assert s.value == -1.0 and list(v) == [0.0] * 4                      # nothing was written


def test_the_methods_exist_on_the_plan_and_on_every_class():
    for name in ("band_select", "estimate_sigma", "estimate_sigma_coef"):
        assert callable(getattr(ndwt.Plan, name))
    for cls in (ndwt.nd_dwt_1D, ndwt.nd_dwt_2D, ndwt.nd_dwt_3D, ndwt.nd_dwt_4D):
        for name in ("estimate_sigma", "estimate_sigma_coef", "band_median", "universal_thresholds"):
            assert callable(getattr(cls, name)), (cls.__name__, name)


def test_the_trace_parser_knows_the_two_families():
    r = ndwt.trace.parse_record("ndwt::BandHist<float, 1, true> grid=(16,1,1) block=(256,1,1)")
    assert r.family == "BandHist" and r.params == {"T": "float", "COMP": 1, "VEC": True, "AGG": 2}
    r = ndwt.trace.parse_record("ndwt::BandHist<double, 2, false, 0> grid=(3,1,1) block=(256,1,1)")
    assert r.params == {"T": "double", "COMP": 2, "VEC": False, "AGG": 0} and r.grid == (3, 1, 1)
    r = ndwt.trace.parse_record("ndwt::BandPick<double> grid=(1,1,1) block=(256,1,1)")
    assert r.family == "BandPick" and r.params == {"T": "double"}


def test_passes_and_digits_per_data_kind(shim):
    """11-bit digits from the top of the key, the last one what is left: float 11 + 11 + 10 in 3 passes, double 5 x 11 + 9 in 6"""
    assert shim.sel_select_consts(0) == 11 and shim.sel_select_consts(1) == 2048 and shim.sel_select_consts(2) == 4
    for f64, keybits, passes, widths in ((0, 32, 3, [11, 11, 10]), (1, 64, 6, [11, 11, 11, 11, 11, 9])):
        assert shim.sel_select_key_bits(f64) == keybits
        assert shim.sel_select_passes(f64) == passes
        got = [(shim.sel_select_digit_shift(f64, p), shim.sel_select_digit_bits(f64, p)) for p in range(passes)]
        assert [b for _, b in got] == widths
        # the digits tile the key without a gap or an overlap, most significant first
        top = keybits
        for shift, bits in got:
            assert shift + bits == top and 1 <= bits <= 11
            top = shift
        assert top == 0


def test_the_four_scalar_form_needs_an_aligned_band_of_whole_groups(shim):
    for sb in (4, 8):
        assert shim.sel_select_vec(4096, 4096, sb) == 1
        assert shim.sel_select_vec(4096 + 4 * sb, 4096, sb) == 1
        for off in (sb, 2 * sb, 3 * sb):                                 # off the 16- / 32-byte groups by one .. three scalars
            assert shim.sel_select_vec(4096 + off, 4096, sb) == 0
        for n in (37, 4097, 4098, 4099):                                 # not whole groups of 4
            assert shim.sel_select_vec(4096, n, sb) == 0
        assert shim.sel_select_vec(4096, 4, sb) == 1
    assert shim.sel_select_vec(4096 + 16, 4096, 8) == 0                  # 16-byte alignment is not enough for 4 doubles
    assert shim.sel_select_vec(4096 + 16, 4096, 4) == 1


def test_the_grid_with_and_without_target_blocks(shim):
    g = shim.sel_select_grid
    cus, cap = 256, 256 * 16
    per = 256 * 8                                                        # kSelectTurns turns of 256 threads
    assert g(37, 1, 0, cus, 0) == 1                                      # below one workgroup
    assert g(per, 1, 0, cus, 0) == 1 and g(per + 1, 1, 0, cus, 0) == 2   # one element per thread and step
    assert g(4 * per, 1, 1, cus, 0) == 1 and g(4 * per + 4, 1, 1, cus, 0) == 2   # 4 scalars per thread and step
    assert g(2 * per, 2, 0, cus, 0) == 1 and g(2 * per + 2, 2, 0, cus, 0) == 2   # complex, element-wise: one pair per thread
    assert g(4 * per * cap, 1, 1, cus, 0) == cap                         # the cap of shrink_run: num_cus * 16
    assert g(4 * per * cap + 4, 1, 1, cus, 0) == cap
    assert g(4 * per * (cap - 1), 1, 1, cus, 0) == cap - 1
    assert g(1 << 32, 1, 1, 8, 0) == 128
    # target_blocks is an upper bound, not a size
    assert g(40000, 1, 1, cus, 0) == 5                                   # 10000 groups of 4 are 4.9 x 2048
    assert g(40000, 1, 1, cus, 3) == 3
    assert g(40000, 1, 1, cus, 5) == 5 and g(40000, 1, 1, cus, 4) == 4
    assert g(40000, 1, 1, cus, 6) == 5
    assert g(37, 1, 0, cus, 3) == 1
    assert g(1 << 40, 1, 1, cus, cap + 5) == cap


def test_bands_of_two_to_the_32_elements_are_refused(shim):
    assert shim.sel_select_fits((1 << 32) - 1) == 1
    assert shim.sel_select_fits(1 << 32) == 0 and shim.sel_select_fits((1 << 32) + 1) == 0
    assert shim.sel_select_fits(1) == 1 and shim.sel_select_fits(0) == 0


def test_the_ab_switch_of_the_wave_wide_combining(shim):
    assert shim.sel_select_agg(0) == 2 and shim.sel_select_agg(9) == 0 and shim.sel_select_agg(11) == 2
