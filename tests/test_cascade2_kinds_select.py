"""cascade2_levels (csrc/ndwt_select.h) for double and interleaved complex images, without a device: the selector is a function of
integers, asked through tests/select/select_shim.cpp as tests/test_dispatch_select.py does.

  * on request (variant 11) it returns the level count of the instance table -- written down here from csrc/ndwt_fused_list.h
    (NDWT_LIST_*2C) -- wherever an instance exists, and 0 everywhere else: 10 taps and longer, rows that are not whole groups of 4
    scalars, images shorter than 3 (Lp - 1) rows, a-trous plans, variant 9;
  * by default it does so from the kind's and direction's size in BYTES on (cascade2_min_bytes) and not one row below it;
  * a float real plan gets what it always got: a literal table written down from the rule it had (<= 8 taps: 3 levels when 3 are left,
    else 2; 12 taps: the analysis, 2 levels; beyond 2048^2 = 6 Mi elements or on request).
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# kind -> (f64, complex).  MAX_NLEV[kind][inverse][Lp]: the most levels one launch takes (an instance of 3 levels has one of 2 beside it)
KINDS = {"f64": (True, False), "c64": (False, True), "c128": (True, True)}
MAX_NLEV = {
    "c64": ({2: 3, 4: 3, 6: 3, 8: 3}, {2: 3, 4: 3, 6: 3, 8: 3}),
    "f64": ({2: 3, 4: 3, 6: 3, 8: 3}, {2: 3, 4: 3, 6: 3, 8: 3}),
    "c128": ({2: 3, 4: 3, 6: 3, 8: 3}, {2: 3, 4: 3, 6: 3, 8: 2}),      # (complex128 synthesis, 8 taps x 3 levels: scratch even at one wave per SIMD)
}
# bytes of the smallest image that takes the cascade by default, (analysis, synthesis): DESIGN.md 4.3 -- 2048^2 complex64, 2048^2 / 4096^2
# double, 2048^2 complex128
MIN_BYTES = {"c64": (32 << 20, 32 << 20), "f64": (32 << 20, 128 << 20), "c128": (64 << 20, 64 << 20)}
ESIZE = {"f32": 4, "c64": 8, "f64": 8, "c128": 16}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++ to compile tests/select/select_shim.cpp")
    out = str(tmp_path_factory.mktemp("select_kinds") / "libselect_shim.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "select", "select_shim.cpp"), "-o", out],
                   check=True)
    return ctypes.CDLL(out)


def _plan(dims, Lp, f64=False, cplx=False, atrous=False, vf=0, vi=0, lens=None):
    lens = lens or [Lp, Lp]
    v = [len(dims), 2 if cplx else 1, f64, not cplx, 1, atrous, 1] + (list(dims) + [1] * 4)[:4] + (list(lens) + [2] * 4)[:4] + [vf, vi]
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _levels(shim, plan, inverse, left):
    return shim.sel_cascade2_levels(plan, int(inverse), int(left))


def _want(kind, inverse, Lp, left):
    top = MAX_NLEV[kind][1 if inverse else 0].get(Lp, 0)
    return 0 if left < 2 or not top else min(3 if left >= 3 else 2, top)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_on_request_the_selector_follows_the_instance_table(shim, kind):
    f64, cplx = KINDS[kind]
    for inverse in (False, True):
        for Lp in range(2, 21, 2):
            for left in range(1, 6):
                got = _levels(shim, _plan([128, 64], Lp, f64, cplx, vf=11, vi=11), inverse, left)
                assert got == _want(kind, inverse, Lp, left), (kind, inverse, Lp, left, got)
    # a mixed pair of wavelets runs at the longer length
    assert _levels(shim, _plan([128, 64], 6, f64, cplx, vf=11, vi=11, lens=[4, 6]), False, 3) == _want(kind, False, 6, 3) == 3
    assert _levels(shim, _plan([128, 64], 12, f64, cplx, vf=11, vi=11), False, 3) == 0           # 12 taps: float real only


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_on_request_it_refuses_what_the_kernels_do_not_take(shim, kind):
    f64, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    ok = _plan([128, 64], 8, f64, cplx, vf=11, vi=11)
    assert _levels(shim, ok, False, 3) == 3 and _levels(shim, ok, True, 2) == 2
    for inverse in (False, True):
        n1 = 65 if cplx else 66                                # 130 / 66 scalars: not whole groups of 4
        assert (n1 * comp) % 4 != 0
        assert _levels(shim, _plan([n1, 64], 8, f64, cplx, vf=11, vi=11), inverse, 3) == 0
        assert _levels(shim, _plan([128, 20], 8, f64, cplx, vf=11, vi=11), inverse, 3) == 0       # n2 = 20 < 3 (8 - 1)
        assert _levels(shim, _plan([128, 21], 8, f64, cplx, vf=11, vi=11), inverse, 3) == _want(kind, inverse, 8, 3)
        assert _levels(shim, _plan([128, 64], 8, f64, cplx, atrous=True, vf=11, vi=11), inverse, 3) == 0
        assert _levels(shim, _plan([128, 64], 8, f64, cplx, vf=9, vi=11), inverse, 3) == 0        # variant 9: analysis AND synthesis
        assert _levels(shim, _plan([128, 64, 32], 8, f64, cplx, vf=11, vi=11), inverse, 3) == 0   # a volume
    assert _levels(shim, _plan([128, 64], 8, f64, cplx, vf=0, vi=9), True, 3) == 0
    assert _levels(shim, _plan([128, 64], 8, f64, cplx, vf=0, vi=0), False, 3) == 0               # small and not asked for
    if cplx:                                                   # an odd number of complex elements whose scalars are whole groups of 4
        assert _levels(shim, _plan([66, 64], 8, f64, cplx, vf=11, vi=11), False, 3) == 3
    assert _levels(shim, _plan([128, 64], 8, f64, cplx, vf=10, vi=12), False, 3) == 3             # variants 10 / 12 ask as 11 does
    assert _levels(shim, _plan([128, 64], 8, f64, cplx, vf=10, vi=12), True, 3) == _want(kind, True, 8, 3)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_default_on_both_sides_of_the_kind_threshold(shim, kind):
    f64, cplx = KINDS[kind]
    n1 = 2048
    for inverse in (False, True):
        n2 = MIN_BYTES[kind][inverse] // (n1 * ESIZE[kind])
        assert n1 * n2 * ESIZE[kind] == MIN_BYTES[kind][inverse]
        assert _levels(shim, _plan([n1, n2], 8, f64, cplx), inverse, 3) == _want(kind, inverse, 8, 3)           # the smallest image that takes it
        assert _levels(shim, _plan([n1, n2 - 1], 8, f64, cplx), inverse, 3) == 0                          # one row fewer
        assert _levels(shim, _plan([n2, n1], 8, f64, cplx), inverse, 2) == 2                              # bytes, not a shape
        assert _levels(shim, _plan([n1, 4 * n2], 8, f64, cplx), inverse, 5) == _want(kind, inverse, 8, 5)
        assert _levels(shim, _plan([n1, n2], 8, f64, cplx, vf=9, vi=9), inverse, 3) == 0
        assert _levels(shim, _plan([n1, n2], 10, f64, cplx), inverse, 3) == 0
    n2 = max(MIN_BYTES[kind]) // (n1 * ESIZE[kind])
    assert _levels(shim, _plan([n1, n2], 8, f64, cplx, vi=9), True, 3) == 0                               # synthesis alone switched off
    assert _levels(shim, _plan([n1, n2], 8, f64, cplx, vi=9), False, 3) == 3
    if MIN_BYTES[kind][0] != MIN_BYTES[kind][1]:               # between the two: the analysis cascades, the synthesis runs per level
        n2 = min(MIN_BYTES[kind]) // (n1 * ESIZE[kind])
        assert _levels(shim, _plan([n1, n2], 8, f64, cplx), False, 3) == 3 and _levels(shim, _plan([n1, n2], 8, f64, cplx), True, 3) == 0


# float real, from the rule the selector had before the other kinds: rows are (Lp, inverse) -> levels taken with left = 1 .. 5
FLOAT_REAL = {
    (2, False): [0, 2, 3, 3, 3], (2, True): [0, 2, 3, 3, 3], (4, False): [0, 2, 3, 3, 3], (4, True): [0, 2, 3, 3, 3],
    (6, False): [0, 2, 3, 3, 3], (6, True): [0, 2, 3, 3, 3], (8, False): [0, 2, 3, 3, 3], (8, True): [0, 2, 3, 3, 3],
    (10, False): [0, 0, 0, 0, 0], (10, True): [0, 0, 0, 0, 0], (12, False): [0, 2, 2, 2, 2], (12, True): [0, 0, 0, 0, 0],
    (14, False): [0, 0, 0, 0, 0], (14, True): [0, 0, 0, 0, 0], (16, False): [0, 0, 0, 0, 0], (16, True): [0, 0, 0, 0, 0],
    (18, False): [0, 0, 0, 0, 0], (18, True): [0, 0, 0, 0, 0], (20, False): [0, 0, 0, 0, 0], (20, True): [0, 0, 0, 0, 0],
}


def test_float_real_plans_get_what_they_always_got(shim):
    zeros = [0] * 5
    for (Lp, inverse), row in FLOAT_REAL.items():
        def ask(dims, vf=0, vi=0, **kw):
            return [_levels(shim, _plan(dims, Lp, vf=vf, vi=vi, **kw), inverse, left) for left in range(1, 6)]
        assert ask([2048, 3073]) == row, (Lp, inverse)                      # beyond 6 Mi elements
        assert ask([2048, 3072]) == zeros, (Lp, inverse)                    # at it
        assert ask([4096, 4096]) == row
        assert ask([256, 96], vf=11, vi=11) == row                          # on request
        assert ask([256, 96], vf=10, vi=12) == row
        assert ask([256, 96], vf=11, vi=0) == (zeros if inverse else row)
        assert ask([256, 96], vf=0, vi=11) == (row if inverse else zeros)
        assert ask([256, 96]) == zeros
        assert ask([2048, 3073], vf=9) == zeros and ask([2048, 3073], vi=9) == (zeros if inverse else row)
        assert ask([2050, 3073]) == zeros                                   # rows of 2050 floats
        assert ask([2048, 3073], atrous=True) == zeros
        assert ask([256, 3 * (Lp - 1) - 1], vf=11, vi=11) == zeros
    assert shim.sel_cascade2_rec_depth(12) == 2 and shim.sel_cascade2_rec_depth(11) == 1 and shim.sel_cascade2_rec_depth(0) == 1
