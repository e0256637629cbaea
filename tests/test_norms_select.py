"""The grid rule of the band norms (csrc/ndwt_select.h: norms_chunks, norms_per_band) without a GPU, through tests/select/norms_shim.cpp:
both sides of every condition.

  turns          a block gets a further chunk only while every one of a workgroup's 256 threads keeps kSelectTurns turns of its loop
  cap            all blocks together stay within num_cus * 16 wherever bands * items is below that cap; above it every block has one chunk
  target_blocks  an upper bound on all blocks on top of that (0: none)
  per band       past 2^31 - 1 (band, item) blocks: one launch per band
"""
import ctypes

import pytest

from items_cases import build_named_shim

CUS = 256


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_named_shim(tmp_path_factory, "norms_shim")
    lib.sel_norms_chunks.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_norms_chunks.restype = ctypes.c_longlong
    lib.sel_norms_per_band.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
    return lib


def test_a_further_chunk_only_while_every_thread_keeps_its_turns(shim):
    turns = shim.sel_norms_turns()
    assert turns == 8
    per_chunk = 256 * turns                                       # steps of one chunk
    for comp, vec, scalars_per_step in ((1, 1, 4), (2, 1, 4), (1, 0, 1), (2, 0, 2)):
        s = per_chunk * scalars_per_step
        assert shim.sel_norms_chunks(s - scalars_per_step, comp, vec, 1, 1, CUS, 0) == 1      # fewer than kSelectTurns turns: one chunk
        assert shim.sel_norms_chunks(s, comp, vec, 1, 1, CUS, 0) == 1
        assert shim.sel_norms_chunks(2 * s - scalars_per_step, comp, vec, 1, 1, CUS, 0) == 1  # two chunks would leave the threads 7.99 turns
        assert shim.sel_norms_chunks(2 * s, comp, vec, 1, 1, CUS, 0) == 2
        assert shim.sel_norms_chunks(5 * s + 3 * scalars_per_step, comp, vec, 1, 1, CUS, 0) == 5
    assert shim.sel_norms_chunks(4, 1, 1, 3, 5, CUS, 0) == 1 and shim.sel_norms_chunks(1, 1, 0, 1, 1, CUS, 0) == 1   # at least one
    assert shim.sel_norms_chunks(20000, 1, 1, 2, 2, CUS, 0) == 2                                # (tests/test_gpu_norms.py: 2 x 20000, level 1)
    assert shim.sel_norms_chunks(20000, 1, 0, 2, 2, CUS, 0) == 9


def test_the_cap_on_all_blocks(shim):
    big = 1 << 30
    cap = CUS * 16
    assert shim.sel_norms_chunks(big, 1, 1, 1, 1, CUS, 0) == cap
    assert shim.sel_norms_chunks(big, 1, 1, 8, 1, CUS, 0) == cap // 8
    assert shim.sel_norms_chunks(big, 1, 1, 5, 3, CUS, 0) == cap // 15                          # rounded down: within the cap
    assert shim.sel_norms_chunks(big, 1, 1, 5, 3, 64, 0) == 64 * 16 // 15                       # the cap is the device's
    assert shim.sel_norms_chunks(big, 1, 1, cap // 2, 1, CUS, 0) == 2
    assert shim.sel_norms_chunks(big, 1, 1, cap // 2 + 1, 1, CUS, 0) == 1
    assert shim.sel_norms_chunks(big, 1, 1, cap, 1, CUS, 0) == 1
    assert shim.sel_norms_chunks(big, 1, 1, 5, cap, CUS, 0) == 1                                # bands * items above the cap: one chunk each
    assert shim.sel_norms_chunks(big, 1, 1, 1, 1 << 31, CUS, 0) == 1


def test_target_blocks_is_an_upper_bound_on_top(shim):
    big = 1 << 30
    assert shim.sel_norms_chunks(big, 1, 1, 2, 2, CUS, 40) == 10
    assert shim.sel_norms_chunks(big, 1, 1, 2, 2, CUS, 1) == 1                                  # below bands * items: still one each
    assert shim.sel_norms_chunks(big, 1, 1, 2, 2, CUS, 1 << 20) == CUS * 16 // 4                # above the cap: the cap holds
    assert shim.sel_norms_chunks(20000, 1, 1, 2, 2, CUS, 40) == 2                               # above what the turns give: they hold
    assert shim.sel_norms_chunks(20000, 1, 1, 2, 2, CUS, 1) == 1
    assert shim.sel_norms_chunks(20000, 1, 1, 2, 2, CUS, 0) == shim.sel_norms_chunks(20000, 1, 1, 2, 2, CUS, -3) == 2   # none


def test_one_launch_per_band_past_what_a_launch_can_number(shim):
    lim = (1 << 31) - 1
    assert shim.sel_norms_per_band(1, lim) == 0 and shim.sel_norms_per_band(lim, 1) == 0
    assert shim.sel_norms_per_band(2, lim) == 1 and shim.sel_norms_per_band(1, lim + 1) == 1
    assert shim.sel_norms_per_band(8, lim // 8) == 0 and shim.sel_norms_per_band(8, lim // 8 + 1) == 1
    # a band alone (what the fallback launches) has one chunk per item at such a count, so its grid is the items: below 2^31
    assert shim.sel_norms_chunks(1 << 20, 1, 1, 1, lim, CUS, 0) == 1
