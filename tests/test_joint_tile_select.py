"""The route of the joint shrinkage and the group norms (csrc/ndwt_select.h: joint_route, joint_tile_strips) without a GPU, through
tests/select/joint_tile_shim.cpp: both sides of every condition.

  hook       variant_inv 11 takes the tile form whatever the plan, 9 never does, anything else is the default
  items      fewer than 64 items never take it unasked
  default    the measured rule: the 4-scalar form only; from 64 items on bands of up to 4096 steps, from 256 items on of up to 16384
  strips     ceil(steps / SW): one strip, two strips, a ragged last one; a step is 4 scalars or one element
  grid       bands x strips beyond 2^31 - 1 workgroups: the launch cannot number them, and not even 11 takes the tile form
"""
import ctypes

import pytest

from items_cases import build_named_shim

CUS = 256
TILE, CHUNKS = 1, 0


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_named_shim(tmp_path_factory, "joint_tile_shim")
    lib.sel_joint_route.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_joint_tile_strips.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_joint_tile_strips.restype = ctypes.c_longlong
    lib.sel_joint_tile_from.restype = ctypes.c_longlong
    return lib


def test_the_tile_is_whole_passes(shim):
    SW, J = shim.sel_joint_tile_sw(), shim.sel_joint_tile_j()
    assert SW >= 1 and 256 % SW == 0 and J >= 256 // SW and J % (256 // SW) == 0
    assert shim.sel_joint_tile_from() == 64


def test_the_strips_of_a_band(shim):
    SW = shim.sel_joint_tile_sw()
    for comp, vec, per_step in ((1, 1, 4), (2, 1, 4), (1, 0, 1), (2, 0, 2)):
        s = SW * per_step                                          # the scalars of one full strip
        assert shim.sel_joint_tile_strips(per_step, comp, vec) == 1                 # one step: one (ragged) strip
        assert shim.sel_joint_tile_strips(s - per_step, comp, vec) == 1
        assert shim.sel_joint_tile_strips(s, comp, vec) == 1                        # one strip exactly
        assert shim.sel_joint_tile_strips(s + per_step, comp, vec) == 2             # two strips, the second of one step
        assert shim.sel_joint_tile_strips(2 * s, comp, vec) == 2
        assert shim.sel_joint_tile_strips(5 * s + 3 * per_step, comp, vec) == 6     # a ragged last strip
    # (tests/test_gpu_joint_tile.py: 96 scalars in the 4-scalar form are 24 steps, 100 are 25, 37 complex elements are 37)
    assert shim.sel_joint_tile_strips(96, 1, 1) == -(-24 // SW) and shim.sel_joint_tile_strips(100, 1, 1) == -(-25 // SW)
    assert shim.sel_joint_tile_strips(74, 2, 0) == -(-37 // SW)


def test_the_hook_forces_and_forbids(shim):
    for n, comp, vec, bands, items in ((96, 1, 1, 3, 5), (37, 1, 0, 3, 1), (74, 2, 0, 7, 70), (4096, 1, 1, 2, 4096), (1 << 22, 1, 1, 8, 8)):
        assert shim.sel_joint_route(n, comp, vec, bands, items, CUS, 11) == TILE, (n, items)
        assert shim.sel_joint_route(n, comp, vec, bands, items, CUS, 9) == CHUNKS, (n, items)
    # any other number is the default
    assert shim.sel_joint_route(4096, 1, 1, 2, 4096, CUS, 3) == shim.sel_joint_route(4096, 1, 1, 2, 4096, CUS, 0) == TILE
    assert shim.sel_joint_route(96, 1, 1, 3, 5, CUS, 12) == shim.sel_joint_route(96, 1, 1, 3, 5, CUS, 0) == CHUNKS


def test_fewer_than_64_items_never_take_it_unasked(shim):
    for n in (4, 96, 1024, 4096, 16384, 65536, 1 << 22):
        for bands in (1, 2, 5, 8):
            for items in (1, 8, 9, 40, 63):
                assert shim.sel_joint_route(n, 1, 1, bands, items, CUS, 0) == CHUNKS, (n, bands, items)
    assert shim.sel_joint_route(4096, 1, 1, 2, 63, CUS, 0) == CHUNKS and shim.sel_joint_route(4096, 1, 1, 2, 64, CUS, 0) == TILE


def test_the_measured_default(shim):
    route = lambda n, items, comp=1, vec=1, bands=2: shim.sel_joint_route(n, comp, vec, bands, items, CUS, 0)   # noqa: E731
    # from 64 items on: bands of up to 4096 steps (16384 scalars in the 4-scalar form)
    assert route(16384, 64) == TILE and route(16384 + 4, 64) == CHUNKS and route(16384, 63) == CHUNKS
    assert route(16384 + 4, 255) == CHUNKS and route(65536, 64) == CHUNKS
    # from 256 items on: of up to 16384 steps
    assert route(65536, 256) == TILE and route(16384 + 4, 256) == TILE and route(65536 + 4, 256) == CHUNKS and route(65536, 255) == CHUNKS
    assert route(65536 + 4, 1 << 20) == CHUNKS                    # longer items were not measured, however many
    assert route(4096, 4096) == TILE and route(1024, 1 << 20) == TILE and route(4, 64) == TILE
    # the bands do not enter, the device does not
    for bands in (1, 2, 5, 8, 15):
        assert route(4096, 4096, bands=bands) == TILE and route(65536, 64, bands=bands) == CHUNKS
    assert shim.sel_joint_route(4096, 1, 1, 2, 4096, 64, 0) == TILE
    # the element-wise form is on request only; complex data count their steps like real data
    assert route(4096, 4096, vec=0) == CHUNKS and route(74, 70, comp=2, vec=0) == CHUNKS
    assert route(16384, 64, comp=2) == TILE and route(16384 + 4, 64, comp=2) == CHUNKS


def test_a_grid_the_launch_cannot_number(shim):
    SW = shim.sel_joint_tile_sw()
    limit = 0x7fffffff
    n = 4 * SW * 1024                                              # 1024 strips a band in the 4-scalar form
    assert shim.sel_joint_tile_strips(n, 1, 1) == 1024
    fits, over = limit // 1024, limit // 1024 + 1
    assert shim.sel_joint_route(n, 1, 1, fits, 4096, CUS, 11) == TILE and shim.sel_joint_route(n, 1, 1, over, 4096, CUS, 11) == CHUNKS
    assert shim.sel_joint_route(n, 1, 1, fits, 4096, CUS, 0) == TILE and shim.sel_joint_route(n, 1, 1, over, 4096, CUS, 0) == CHUNKS
    # one band of more than 2^31 - 1 strips (element-wise: a strip is SW elements)
    assert shim.sel_joint_route((limit + 1) * SW, 1, 0, 1, 4096, CUS, 11) == CHUNKS
    assert shim.sel_joint_route(limit * SW, 1, 0, 1, 4096, CUS, 11) == TILE
    assert shim.sel_joint_route(4096, 1, 1, 0, 4096, CUS, 11) == CHUNKS                          # no band: nothing to tile
