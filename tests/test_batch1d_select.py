"""cascade1_levels (csrc/ndwt_select.h) and the instance table of the 1-D cascade (csrc/ndwt_fused_list.h: NDWT_LIST_*1C), without a
device: functions of integers, asked through tests/select/cascade1_shim.cpp.

  * how a level count splits into launches: the largest of 4, 3, 2 levels that is left, then one launch per level;
  * every condition that takes the cascade off, one at a time: a plan that is not batched, a-trous dilation, rows that are not whole
    groups of 4 scalars, rows shorter than 8 L scalars, 10 taps, variant 9 per direction -- and a few more (the generic path, rows of
    2^30 scalars, a 2-D plan);
  * the host's tile width against the rule written down here, and the table against the one written down here: 96 instances.
"""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# the table: {float, double} x EW {1, 2} x L {2, 4, 6, 8} x NLEV {2, 3, 4} x {analysis, synthesis}
TABLE = {(inv, f64, ew, L, nlev) for inv in (0, 1) for f64 in (0, 1) for ew in (1, 2) for L in (2, 4, 6, 8) for nlev in (2, 3, 4)}
NONE, ROWS1 = 0, 1                                                                # CascadeKind of csrc/ndwt_select.h
KINDS = {"f32": (False, False), "c64": (False, True), "f64": (True, False), "c128": (True, True)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++ to compile tests/select/cascade1_shim.cpp")
    out = str(tmp_path_factory.mktemp("select_batch1d") / "libcascade1_shim.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "select", "cascade1_shim.cpp"), "-o", out],
                   check=True)
    lib = ctypes.CDLL(out)
    lib.sel_cascade1_levels.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.sel_cascade1_levels_n.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_cascade_route.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return lib


def _plan(n, L, f64=False, cplx=False, atrous=False, vf=0, vi=0, ndim=1, path_auto=True):
    dims = [n] + [64] * (ndim - 1)
    v = [ndim, 2 if cplx else 1, f64, not cplx, path_auto, atrous, 1] + (dims + [1] * 4)[:4] + [L] * ndim + [2] * (4 - ndim) + [vf, vi]
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _levels(shim, plan, howmany, inverse, left):
    L = ctypes.c_int(-1)
    n = shim.sel_cascade1_levels(plan, howmany, int(inverse), int(left), ctypes.byref(L))
    return n, L.value


def _launches(shim, plan, howmany, inverse, level):
    """the walk of dec_impl / rec_impl: cascade_route (csrc/ndwt_select.h) asked once per launch, for the levels still to do"""
    out, left = [], level
    while left:
        nlev = ctypes.c_int(-1)
        kind = shim.sel_cascade_route(plan, howmany, int(inverse), int(left), ctypes.byref(nlev))
        n = _levels(shim, plan, howmany, inverse, left)[0]
        assert kind == (ROWS1 if n else NONE) and nlev.value == n
        out.append(nlev.value if kind != NONE else 1)
        left -= out[-1]
    return out


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_level_count_splits_into_launches_of_four_three_two(shim, kind):
    f64, cplx = KINDS[kind]
    want = {1: [1], 2: [2], 3: [3], 4: [4], 5: [4, 1], 6: [4, 2], 7: [4, 3], 8: [4, 4], 9: [4, 4, 1]}
    for inverse in (False, True):
        for L in (2, 4, 6, 8):
            plan = _plan(512, L, f64, cplx)
            for level, split in want.items():
                assert _launches(shim, plan, 3, inverse, level) == split, (kind, inverse, L, level)
            assert _levels(shim, plan, 3, inverse, 4) == (4, L)                   # the tap length comes back with the count
    assert _launches(shim, _plan(512, 8, f64, cplx), 1, False, 5) == [4, 1]       # one signal is a batch too


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_condition_that_takes_the_cascade_off(shim, kind):
    f64, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    for inverse in (False, True):
        def ask(n=512, L=8, howmany=3, **kw):
            return _levels(shim, _plan(n, L, f64, cplx, **kw), howmany, inverse, 4)[0]
        assert ask() == 4
        assert ask(howmany=0) == 0                                                # not a batched plan
        assert ask(atrous=True) == 0
        n_odd = 511 if not cplx else 255                                          # 511 / 510 scalars: not whole groups of 4
        assert (n_odd * comp) % 4 != 0 and ask(n=n_odd) == 0
        if cplx:
            assert ask(n=258) == 4                                                # an even number of pairs IS whole groups of 4
        for L in (2, 4, 6, 8):                                                    # n comp >= 8 L, the floor of the per-level kernel
            n_min = 8 * L // comp
            assert ask(n=n_min, L=L) == 4 and ask(n=n_min - 4 // comp, L=L) == 0, (L, n_min)
        assert ask(L=10) == 0 and ask(L=12) == 0 and ask(L=20) == 0               # db5 and longer
        assert ask(path_auto=False) == 0                                          # the generic path was asked for
        assert ask(ndim=2) == 0
        assert shim.sel_cascade1_levels_n(_plan(512, 8, f64, cplx), (1 << 30) // comp, 3, int(inverse), 4) == 0
        assert shim.sel_cascade1_levels_n(_plan(512, 8, f64, cplx), (1 << 30) // comp - 4, 3, int(inverse), 4) == 4
        # variant 9, per direction
        assert ask(vf=9) == (4 if inverse else 0)
        assert ask(vi=9) == (0 if inverse else 4)
        assert ask(vf=9, vi=9) == 0
        assert ask(vf=11, vi=11) == 4                                             # the other numbers mean nothing here
        assert _levels(shim, _plan(512, 8, f64, cplx), 3, inverse, 1)[0] == 0     # one level left: nothing to cascade


def _tile_width(inverse, f64, ew, L, nlev):
    LH, RH = (L // 2, L // 2 - 1) if inverse else (L // 2 - 1, L // 2)
    GL, GR = (LH * ew + 3) // 4, (RH * ew + 3) // 4
    LPL = 32 // (8 if f64 else 4)
    return 4 * ((64 - nlev * (GL + GR)) // LPL * LPL)


def test_tile_width_of_every_instance_is_the_window_valid_at_every_level_in_whole_lines(shim):
    assert len(TABLE) == 96
    for k in sorted(TABLE):
        w = shim.sel_cascade1_tile_width(*k)
        assert w == _tile_width(*k) and w > 0 and (w * (8 if k[1] else 4)) % 128 == 0, (k, w)
    assert shim.sel_cascade1_tile_width(0, 0, 1, 8, 4) == 224 and shim.sel_cascade1_tile_width(1, 1, 2, 8, 4) == 192   # 56 and 48 lanes
    assert shim.sel_cascade1_tile_width(0, 0, 1, 2, 2) == 224 and shim.sel_cascade1_tile_width(0, 1, 1, 2, 2) == 240


def test_the_instance_table_is_the_one_written_down_here(shim):
    asked = set(itertools.product((0, 1), (0, 1), (1, 2, 4), range(0, 13), range(0, 7)))
    listed = {k for k in asked if shim.sel_cascade1_listed(*k)}
    assert listed == TABLE
