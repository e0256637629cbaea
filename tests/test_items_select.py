"""The host-side decisions of the per-item calls (csrc/ndwt_select.h: select_items_route, shrink_items_chunks), without a device:
functions of integers, asked through tests/select/items_shim.cpp.

  * select_items_route: at least as many items as compute units take the one launch; variant 11 forces it and variant 9 forces the loop,
    whatever the sizes; with fewer items the one launch is taken only where it was measured to win (up to 2^14 scalars
    from 8 items on, up to 2^18 scalars from 64 items on), and the constants of the predicate are the documented ones;
  * shrink_items_chunks: at least one workgroup per (band, item) block, no more than the block has steps of 256 threads, all blocks
    together within shrink_run's cap of num_cus * 16 wherever bands * items is below it;
  * the answers of cascade_route / denoise1_levels are those of before: tests/test_denoise1_select.py and tests/test_dispatch_select.py
    run unchanged on the same header; here the grid of the former is asked once more through its own shim with the new header in place.
"""
import ctypes
import os
import re

import pytest

from items_cases import build_items_shim, build_named_shim

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "non-decimated_wavelets_amd", "csrc")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_items_shim(tmp_path_factory)


def test_as_many_items_as_compute_units_take_the_one_launch(shim):
    for cus in (8, 256, 304):
        for n in (4, 4096, 1 << 22):
            assert shim.sel_items_one_launch(n, cus, cus, 0) == 1
            assert shim.sel_items_one_launch(n, cus + 1, cus, 0) == 1 and shim.sel_items_one_launch(n, 1 << 20, cus, 0) == 1
        for n in ((1 << 22) + 4, 1 << 24, 1 << 31):               # beyond the largest item measured: the loop, whatever the item count
            assert shim.sel_items_one_launch(n, cus, cus, 0) == 0 and shim.sel_items_one_launch(n, 1 << 20, cus, 0) == 0
            assert shim.sel_items_one_launch(n, cus, cus, 11) == 1


def test_the_variants_force_their_route(shim):
    for n, items in ((4, 1), (1 << 22, 8), (4096, 4096), (1 << 14, 255)):
        assert shim.sel_items_one_launch(n, items, 256, 11) == 1
        assert shim.sel_items_one_launch(n, items, 256, 9) == 0
    for v in (1, 2, 4, 10, 12):                                   # numbers the column does not name: the default
        assert shim.sel_items_one_launch(4096, 4096, 256, v) == 1 and shim.sel_items_one_launch(1 << 22, 8, 256, v) == 0
        assert shim.sel_items_one_launch(4096, 8, 256, v) == 1


def test_fewer_items_than_compute_units_take_what_was_measured_to_win(shim):
    """the constants of the predicate are those its comment and DESIGN.md 4.3f document: the measured table supports exactly them"""
    few, small, many, large = (shim.sel_items_route_const(i) for i in range(4))
    assert (few, small, many, large) == (8, 1 << 14, 64, 1 << 18)
    hdr = open(os.path.join(CSRC, "ndwt_select.h")).read()
    assert re.search(r"kItemsFewFrom = 8, kItemsOneLaunchMaxScalars = 1LL << 14;", hdr)
    assert re.search(r"kItemsManyFrom = 64, kItemsOneLaunchMaxScalarsMany = 1LL << 18;", hdr)
    design = open(os.path.join(os.path.dirname(HERE), "DESIGN.md")).read()
    for word in ("4.3f", "kItemsOneLaunchMaxScalars", "kItemsOneLaunchMaxScalarsMany", "kItemsFewFrom", "kItemsManyFrom"):
        assert word in design, word
    one = lambda n, items: shim.sel_items_one_launch(n, items, 256, 0)
    for n in (4, 4096, 1 << 14):                                  # measured to win at 8 and at 64 items
        assert one(n, 8) == 1 and one(n, 9) == 1 and one(n, 64) == 1 and one(n, 255) == 1
        assert one(n, 7) == 0 and one(n, 1) == 0                  # fewer items than were measured: the loop
    for n in ((1 << 14) + 1, 1 << 16, 1 << 18):                   # won at 64 items, lost at 8, not measured in between
        assert one(n, 8) == 0 and one(n, 32) == 0 and one(n, 63) == 0
        assert one(n, 64) == 1 and one(n, 255) == 1
    for n in ((1 << 18) + 1, 1 << 22, 1 << 30):                   # lost wherever it was measured
        assert one(n, 1) == 0 and one(n, 8) == 0 and one(n, 64) == 0 and one(n, 255) == 0 and one(n, 256) == int(n <= 1 << 22)
    assert shim.sel_items_route_const(4) == 1 << 22 and "kItemsOneLaunchMaxScalarsFull" in design


def test_the_workgroups_of_a_block_of_shrink_items(shim):
    c = shim.sel_shrink_items_chunks
    cus, cap = 256, 256 * 16
    assert c(37, 1, 0, 5, 5, cus) == 1                            # below one step of 256 threads
    assert c(1024, 1, 1, 1, 1, cus) == 1 and c(1028, 1, 1, 1, 1, cus) == 2   # 4 scalars per thread and step
    assert c(256, 1, 0, 1, 1, cus) == 1 and c(257, 1, 0, 1, 1, cus) == 2     # one element per thread and step
    assert c(512, 2, 0, 1, 1, cus) == 1 and c(514, 2, 0, 1, 1, cus) == 2     # complex, element-wise: one pair per thread
    assert c(1 << 30, 1, 1, 1, 1, cus) == cap                     # one block: the whole cap of shrink_run
    assert c(1 << 30, 1, 1, 4, 8, cus) == cap // 32               # ... shared among the blocks
    assert c(1 << 30, 1, 1, 5, 4096, cus) == 1                    # more blocks than the cap: one workgroup each
    assert c(1 << 30, 1, 1, 3, 1000, cus) == 1 and c(1 << 30, 1, 1, 1, 1000, cus) == 4
    for bands, items in ((1, 1), (4, 8), (5, 100), (8, 511)):     # within the cap wherever bands * items is
        assert bands * items * c(1 << 30, 1, 1, bands, items, cus) <= cap


def test_the_row_threshold_instances_are_the_uniform_ones_less_what_was_dropped(shim):
    """NDWT_LIST_*_DEN1R against NDWT_LIST_*_DEN1: the same (T, EW, L, NLEV); no ROWTHR instance spilled where its twin does not, so
    none was dropped (DESIGN.md 4.3f has the audit)"""
    dropped = set()
    n = 0
    for f64 in (0, 1):
        for ew in (1, 2):
            for L in (2, 3, 4, 6, 8, 10):
                for nlev in (0, 1, 2, 3, 4, 5):
                    uni, row = shim.sel_den1_listed_too(f64, ew, L, nlev), shim.sel_den1r_listed(f64, ew, L, nlev)
                    assert row == (uni and (f64, ew, L, nlev) not in dropped), (f64, ew, L, nlev)
                    n += row
    assert n == 61                                                # 64 less the three complex128 instances that left both tables


def test_the_one_launch_denoise_of_a_batch_answers_as_before(tmp_path_factory):
    """the grid of tests/test_denoise1_select.py: the whole depth or nothing, and the variants that switch it"""
    lib = build_named_shim(tmp_path_factory, "denoise1_shim")
    lib.sel_denoise1_levels.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int]
    spill = {(1, 2, 6, 4), (1, 2, 8, 3), (1, 2, 8, 4)}

    def plan(n, L, f64, cplx, vf=0, vi=0):
        v = [1, 2 if cplx else 1, f64, not cplx, True, False, 1] + [n, 1, 1, 1] + [L, 2, 2, 2] + [vf, vi]
        return (ctypes.c_int * len(v))(*[int(x) for x in v])
    for f64 in (0, 1):
        for cplx in (0, 1):
            for L in (2, 4, 6, 8):
                for level in (1, 2, 3, 4, 5):
                    want = 0 if level == 5 or (f64, 2 if cplx else 1, L, level) in spill else level
                    assert lib.sel_denoise1_levels(plan(512, L, f64, cplx), 3, 1, level) == want
                assert lib.sel_denoise1_levels(plan(512, L, f64, cplx, vf=9), 3, 1, 2) == 0
                assert lib.sel_denoise1_levels(plan(512, L, f64, cplx, vi=9), 3, 1, 2) == 0
