"""denoise1_levels (csrc/ndwt_select.h) and the instance table of the one-launch denoise of a batched 1-D plan (csrc/ndwt_fused_list.h:
NDWT_LIST_*DEN1), without a device: functions of integers, asked through tests/select/denoise1_shim.cpp.

  * the whole depth or nothing: 1 .. 4 levels answer themselves, 5 answers 0;
  * every condition that takes the launch off, one at a time: a plan that is not batched, a 2-D plan, interleaved samples, a-trous
    dilation, the generic path, rows that are not whole groups of 4 scalars, rows shorter than 8 L scalars, 10 taps, variant 9 in
    either slot -- and rows of 2^30 scalars;
  * who asks: variant 11 / 11, or the data kind's default;
  * the host's tile width against the rule written down here, and the table against the one written down here: 64 less the 3 that spill.
"""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# the table: {float, double} x EW {1, 2} x L {2, 4, 6, 8} x NLEV {1, 2, 3, 4}, less the three complex128 instances that spill registers
# at 4 waves per SIMD (they left the table: csrc/ndwt_fused_list.h)
SPILL = {(1, 2, 6, 4), (1, 2, 8, 3), (1, 2, 8, 4)}
TABLE = {(f64, ew, L, nlev) for f64 in (0, 1) for ew in (1, 2) for L in (2, 4, 6, 8) for nlev in (1, 2, 3, 4)} - SPILL
KINDS = {"f32": (False, False), "c64": (False, True), "f64": (True, False), "c128": (True, True)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++ to compile tests/select/denoise1_shim.cpp")
    out = str(tmp_path_factory.mktemp("select_denoise1") / "libdenoise1_shim.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "select", "denoise1_shim.cpp"), "-o", out],
                   check=True)
    lib = ctypes.CDLL(out)
    lib.sel_denoise1_levels.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int]
    lib.sel_denoise1_levels_n.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int]
    return lib


def _plan(n, L, f64=False, cplx=False, atrous=False, vf=0, vi=0, ndim=1, path_auto=True):
    dims = [n] + [64] * (ndim - 1)
    v = [ndim, 2 if cplx else 1, f64, not cplx, path_auto, atrous, 1] + (dims + [1] * 4)[:4] + [L] * ndim + [2] * (4 - ndim) + [vf, vi]
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_whole_depth_or_nothing(shim, kind):
    f64, cplx = KINDS[kind]
    for L in (2, 4, 6, 8):
        plan = _plan(512, L, f64, cplx)
        for level in (1, 2, 3, 4):
            want = 0 if (int(f64), 2 if cplx else 1, L, level) in SPILL else level      # an instance that left the table: the general route
            assert shim.sel_denoise1_levels(plan, 3, 1, level) == want, (kind, L, level)
        for level in (5, 6, 9, 0, -1):
            assert shim.sel_denoise1_levels(plan, 3, 1, level) == 0, (kind, L, level)
    assert shim.sel_denoise1_levels(_plan(512, 4, f64, cplx), 1, 1, 4) == 4          # one signal is a batch too


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_condition_that_takes_the_launch_off(shim, kind):
    f64, cplx = KINDS[kind]
    comp = 2 if cplx else 1

    def ask(n=512, L=4, howmany=3, inner=1, level=4, **kw):
        return shim.sel_denoise1_levels(_plan(n, L, f64, cplx, **kw), howmany, inner, level)
    assert ask() == 4
    assert ask(howmany=0) == 0                                                # not a batched plan
    assert ask(ndim=2) == 0                                                   # a stack of images
    assert ask(inner=4) == 0 and ask(inner=2) == 0                            # interleaved samples
    assert ask(atrous=True) == 0
    assert ask(path_auto=False) == 0                                          # the generic path was asked for
    n_odd = 511 if not cplx else 255                                          # 511 / 510 scalars: not whole groups of 4
    assert (n_odd * comp) % 4 != 0 and ask(n=n_odd) == 0
    if cplx:
        assert ask(n=258) == 4                                                # an even number of pairs IS whole groups of 4
    for L in (2, 4, 6, 8):                                                    # n comp >= 8 L, the floor of the per-level kernel
        n_min = 8 * L // comp
        assert ask(n=n_min, L=L, level=2) == 2 and ask(n=n_min - 4 // comp, L=L, level=2) == 0, (L, n_min)
    assert ask(L=10) == 0 and ask(L=12) == 0 and ask(L=20) == 0               # db5 and longer
    assert shim.sel_denoise1_levels_n(_plan(512, 4, f64, cplx), (1 << 30) // comp, 3, 4) == 0
    assert shim.sel_denoise1_levels_n(_plan(512, 4, f64, cplx), (1 << 30) // comp - 4, 3, 4) == 4
    # variant 9 in either slot (the A/B switch); the other numbers do not take it off
    assert ask(vf=9) == 0 and ask(vi=9) == 0 and ask(vf=9, vi=9) == 0
    assert ask(vf=11, vi=11) == 4 and ask(vf=11) == 4 and ask(vi=11) == 4 and ask(vf=2, vi=5) == 4


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_who_asks_for_the_launch(shim, kind):
    """variant 11 in BOTH slots asks for it; otherwise the data kind's default decides"""
    f64, cplx = KINDS[kind]
    default = shim.sel_denoise1_default(int(f64), 2 if cplx else 1)
    assert default in (0, 1)
    assert shim.sel_denoise1_wanted(_plan(512, 8, f64, cplx, vf=11, vi=11)) == 1
    for vf, vi in ((0, 0), (11, 0), (0, 11), (10, 12)):
        assert shim.sel_denoise1_wanted(_plan(512, 8, f64, cplx, vf=vf, vi=vi)) == default, (vf, vi)


def _tile_width(L, ew, f64, nlev):
    GLa, GRa = ((L // 2 - 1) * ew + 3) // 4, ((L // 2) * ew + 3) // 4         # analysis: L/2 - 1 taps to the left, L/2 to the right
    GLs, GRs = ((L // 2) * ew + 3) // 4, ((L // 2 - 1) * ew + 3) // 4         # synthesis: the other way round
    lpl = 32 // (8 if f64 else 4)
    return 4 * ((64 - nlev * (GLa + GRa + GLs + GRs)) // lpl * lpl)


def test_tile_width_of_every_instance_is_the_window_valid_after_both_cascades_in_whole_lines(shim):
    assert len(TABLE) == 61
    for f64, ew, L, nlev in sorted(TABLE):
        w = shim.sel_den1_tile_width(L, ew, f64, nlev)
        assert w == _tile_width(L, ew, f64, nlev) and w > 0 and (w * (8 if f64 else 4)) % 128 == 0, ((f64, ew, L, nlev), w)
    assert shim.sel_den1_tile_width(8, 1, 0, 4) == 192                        # float db4 at 4 levels: 48 of 64 lanes
    assert shim.sel_den1_tile_width(8, 2, 0, 4) == 128 and shim.sel_den1_tile_width(8, 2, 1, 4) == 128   # the narrowest: 32 lanes
    assert shim.sel_den1_tile_width(2, 1, 0, 1) == 224 and shim.sel_den1_tile_width(2, 1, 1, 1) == 240  # db1, one level: 62 lanes -> 56 / 60


def test_the_instance_table_is_the_one_written_down_here(shim):
    asked = set(itertools.product((0, 1), (1, 2, 4), range(0, 13), range(0, 7)))
    listed = {k for k in asked if shim.sel_den1_listed(*k)}
    assert listed == TABLE
