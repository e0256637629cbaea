"""The selectors (csrc/ndwt_select.h) as a stack plan (ndwt_plan_create_axes) asks them, without a device: functions of integers, asked
through tests/select/stack_shim.cpp.

  * level_route of a stack: one fused launch at tap stride 1, the per-axis passes for a dilated level (the sub-lattice forms use the
    batch slot themselves), for filters the fused kernels refuse, for more items than a launch can count;
  * cascade2_levels of a stack: on request under the per-item conditions of a single image, every ineligibility one at a time; unasked
    from the measured (item height, bytes of all items) of the kind and direction on (cascade2_stack_default) and not one row or one
    item below it;
  * fused2_select with a batch count on both sides of the Inv2P bound (the waves of all items count against the round);
  * an unbatched SelPlan / a Fused2Query of one image answer exactly what they answered before there were stacks: literal tables,
    written down from the build before this one.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED3_DILATED, FUSED3, FUSED3T, FUSED3FOLDT, FUSED2_DILATED, FUSED2, PER_AXIS = range(7)     # LevelRouteKind
KINDS = {"f32": (0, 0), "c64": (0, 1), "f64": (1, 0), "c128": (1, 1)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++ to compile tests/select/stack_shim.cpp")
    out = str(tmp_path_factory.mktemp("select_stack") / "libstack_shim.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "select", "stack_shim.cpp"), "-o", out],
                   check=True)
    lib = ctypes.CDLL(out)
    lib.stk_level_route.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.stk_cascade2_levels.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.stk_shrink_capable.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.stk_fused2.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.stk_cascade2_stack_default.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong]
    return lib


def _plan(dims, lens, f64=0, cplx=0, atrous=0, vf=0, vi=0, path_auto=1):
    v = [len(dims), 2 if cplx else 1, f64, not cplx, path_auto, atrous, 1] + (list(dims) + [1] * 4)[:4] + (list(lens) + [2] * 4)[:4] + [vf, vi]
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _route(shim, plan, howmany, stride, direction, slab=0):
    Lp = ctypes.c_int(-1)
    return shim.stk_level_route(plan, howmany, stride, direction, slab, ctypes.byref(Lp)), Lp.value


def _levels(shim, plan, howmany, inverse, left):
    Lp = ctypes.c_int(-1)
    return shim.stk_cascade2_levels(plan, howmany, int(inverse), left, ctypes.byref(Lp))


def _fused2(shim, q, nbatch):
    o = (ctypes.c_int * 10)()
    shim.stk_fused2((ctypes.c_int * 9)(*q), nbatch, o)
    return list(o)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_level_route_of_a_stack(shim, kind):
    f64, cplx = KINDS[kind]
    img = _plan([64, 40], [8, 8], f64, cplx)
    vol = _plan([24, 20, 20], [4, 4, 4], f64, cplx)
    for K in (1, 3, 4096):
        for d in (0, 1):
            assert _route(shim, img, K, 1, d) == (FUSED2, 8)
            assert _route(shim, vol, K, 1, d) == (FUSED3, 4)
            for stride in (2, 4):                                 # a dilated level: never a sub-lattice form
                assert _route(shim, img, K, stride, d) == (PER_AXIS, 0)
                assert _route(shim, vol, K, stride, d) == (PER_AXIS, 0)
            assert _route(shim, img, K, 1, d, slab=1) == (PER_AXIS, 0)            # a stack is never a slab
    if not cplx:                                                  # ... where the unbatched plan takes the sub-lattice form
        assert _route(shim, _plan([64, 40], [4, 4], f64), 0, 2, 0)[0] == FUSED2_DILATED
        assert _route(shim, _plan([64, 40], [4, 4], f64), 3, 2, 0) == (PER_AXIS, 0)
        assert _route(shim, _plan([24, 20, 20], [4, 4, 4], f64), 0, 2, 0)[0] == FUSED3_DILATED
        assert _route(shim, _plan([24, 20, 20], [4, 4, 4], f64), 3, 2, 0) == (PER_AXIS, 0)
    # what the fused kernels refuse: db9 / db10 on double and complex data, the generic path, more items than a launch counts
    long_taps = 18 if f64 or cplx else 22
    assert _route(shim, _plan([64, 40], [long_taps] * 2, f64, cplx), 3, 1, 0) == (PER_AXIS, 0)
    assert _route(shim, _plan([64, 40], [8, 8], f64, cplx, path_auto=0), 3, 1, 0) == (PER_AXIS, 0)
    assert _route(shim, _plan([24, 20, 20], [4, 4, 4], f64, cplx, path_auto=0), 3, 1, 1) == (PER_AXIS, 0)
    assert _route(shim, img, (1 << 20) - 1, 1, 0) == (FUSED2, 8) and _route(shim, img, 1 << 20, 1, 0) == (PER_AXIS, 0)
    assert _route(shim, vol, (1 << 20) - 1, 1, 0) == (FUSED3, 4) and _route(shim, vol, 1 << 20, 1, 0) == (PER_AXIS, 0)
    # a batched 1-D plan is no stack: it keeps the per-axis route it had
    assert _route(shim, _plan([512], [8], f64, cplx), 3, 1, 0) == (PER_AXIS, 0)
    # ndwt_denoise thresholds in the synthesis loads wherever every level is a fused launch
    assert shim.stk_shrink_capable(img, 3) == 1 and shim.stk_shrink_capable(vol, 3) == 1
    assert shim.stk_shrink_capable(_plan([64, 40], [8, 8], f64, cplx, atrous=1), 3) == 0


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_cascade2_levels_of_a_stack(shim, kind):
    f64, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    top_inv = 2 if kind == "c128" else 3                          # complex128 synthesis, 8 taps: two levels per launch
    for K in (1, 3, 1000):
        ok = _plan([128, 64], [8, 8], f64, cplx, vf=11, vi=11)
        assert _levels(shim, ok, K, False, 3) == 3 and _levels(shim, ok, K, False, 2) == 2 and _levels(shim, ok, K, False, 1) == 0
        assert _levels(shim, ok, K, True, 3) == top_inv and _levels(shim, ok, K, True, 2) == 2
        for inverse in (False, True):
            want = top_inv if inverse else 3
            n1 = 65 if cplx else 66                               # rows that are not whole groups of 4 scalars
            assert (n1 * comp) % 4 != 0
            assert _levels(shim, _plan([n1, 64], [8, 8], f64, cplx, vf=11, vi=11), K, inverse, 3) == 0
            assert _levels(shim, _plan([128, 20], [8, 8], f64, cplx, vf=11, vi=11), K, inverse, 3) == 0      # n2 < 3 (Lp - 1), per item
            assert _levels(shim, _plan([128, 21], [8, 8], f64, cplx, vf=11, vi=11), K, inverse, 3) == want
            assert _levels(shim, _plan([128, 64], [8, 8], f64, cplx, atrous=1, vf=11, vi=11), K, inverse, 3) == 0
            assert _levels(shim, _plan([128, 64], [8, 8], f64, cplx, vf=9, vi=11), K, inverse, 3) == 0
            assert _levels(shim, _plan([128, 64], [10, 10], f64, cplx, vf=11, vi=11), K, inverse, 3) == 0
            assert _levels(shim, _plan([128, 64], [8, 8], f64, cplx, vf=11, vi=11, path_auto=0), K, inverse, 3) == 0
            assert _levels(shim, _plan([128, 64, 32], [8, 8, 8], f64, cplx, vf=11, vi=11), K, inverse, 3) == 0   # a stack of volumes
            # n1 n2 < 2^31 is per item: the stack as a whole may be larger
            assert _levels(shim, _plan([1 << 16, (1 << 15) // comp], [8, 8], f64, cplx, vf=11, vi=11), K, inverse, 3) == 0
            assert _levels(shim, _plan([1 << 16, (1 << 15) // comp - 1], [8, 8], f64, cplx, vf=11, vi=11), K, inverse, 3) == want
        assert _levels(shim, _plan([128, 64], [8, 8], f64, cplx, vf=11, vi=9), K, True, 3) == 0
        assert _levels(shim, _plan([128, 64], [8, 8], f64, cplx, vf=11, vi=0), K, True, 3) == 0    # per direction
        assert _levels(shim, _plan([128, 64], [8, 8], f64, cplx, vf=0, vi=11), K, False, 3) == 0
        assert _levels(shim, _plan([128, 64], [8, 8], f64, cplx, vf=10, vi=12), K, False, 3) == 3
        assert _levels(shim, _plan([128, 64], [8, 8], f64, cplx, vf=10, vi=12), K, True, 3) == top_inv
    # unasked: per kind and direction from the smallest measured (item height, bytes of all items) on -- float real the
    # analysis from 128 rows, the synthesis from 256, both at 64 MiB; the other kinds from 512 rows at 128 MiB; variant 9 switches it off
    esize = (8 if f64 else 4) * comp
    for inverse in (False, True):
        want = top_inv if inverse else 3
        h = (256 if inverse else 128) if kind == "f32" else 512
        total = (64 << 20) if kind == "f32" else (128 << 20)
        n1 = 512
        K = total // (n1 * h * esize)
        assert K * n1 * h * esize == total and K >= 2
        assert _levels(shim, _plan([n1, h], [8, 8], f64, cplx), K, inverse, 3) == want, (kind, inverse)
        assert _levels(shim, _plan([n1, h], [8, 8], f64, cplx), K - 1, inverse, 3) == 0                   # one item fewer: below the bytes
        assert _levels(shim, _plan([n1, h - 1], [8, 8], f64, cplx), 2 * K, inverse, 3) == 0               # one row fewer per item
        assert _levels(shim, _plan([n1, 4 * h], [8, 8], f64, cplx), K, inverse, 3) == want
        assert _levels(shim, _plan([n1, h], [8, 8], f64, cplx, vf=9, vi=9), K, inverse, 3) == 0
        assert _levels(shim, _plan([n1, h], [8, 8], f64, cplx, atrous=1), K, inverse, 3) == 0
        assert _levels(shim, _plan([n1, h], [10, 10], f64, cplx), K, inverse, 3) == 0
        assert shim.stk_cascade2_stack_default(f64, comp, int(inverse), h, total) == 1
        assert shim.stk_cascade2_stack_default(f64, comp, int(inverse), h - 1, 1 << 40) == 0
        assert shim.stk_cascade2_stack_default(f64, comp, int(inverse), 1 << 20, total - 1) == 0
    for dims, K in (([256, 96], 3), ([128, 64], 1000), ([4096, 100], 64)):                                 # many small items: never unasked
        for inverse in (False, True):
            assert _levels(shim, _plan(dims, [8, 8], f64, cplx), K, inverse, 3) == 0, (dims, K, inverse)
    if kind == "f32":                                          # between the two directions: the analysis cascades, the synthesis does not
        p = _plan([512, 128], [8, 8], f64, cplx)
        assert _levels(shim, p, 256, False, 3) == 3 and _levels(shim, p, 256, True, 3) == 0
    assert _levels(shim, _plan([8192, 8192], [8, 8], f64, cplx), 0, False, 3) == 3                 # (a single image: its own thresholds)


def test_fused2_select_counts_the_waves_of_every_item(shim):
    # synthesis of float real rows of 128 scalars (one tile), 700 rows = 10 chunks of 70: Inv2P while items x 10 <= 1280 waves
    q = [0, 1, 1, 8, 1, 1, 128, 700, 0]
    assert shim.stk_fused2_tile_width(1, 8, 1) >= 128
    assert _fused2(shim, q, 1) == [1, 1, 0, 1, 8, 1, 4, 1, 1024, 1]
    assert _fused2(shim, q, 128) == [1, 1, 0, 1, 8, 1, 4, 1, 1024, 1]
    assert _fused2(shim, q, 129) == [0, 1, 0, 1, 8, 1, 4, 0, 2048, 1]
    q = [1, 1, 1, 4, 1, 1, 128, 700, 0]                        # double, 4 taps: depth 4, scalar FMAs
    assert _fused2(shim, q, 128) == [1, 1, 1, 1, 4, 1, 4, 0, 1024, 1]
    assert _fused2(shim, q, 129)[0] == 0 and _fused2(shim, q, 129)[8] == 2048
    assert _fused2(shim, [0, 1, 1, 8, 1, 1, 128, 700, 4], 129) == [1, 1, 0, 1, 8, 1, 4, 1, 2048, 1]   # a variant that asks: whatever the size
    assert _fused2(shim, [0, 1, 1, 8, 1, 1, 128, 700, 1], 3)[0] == 0                               # keeps Inv2S
    assert _fused2(shim, [0, 1, 1, 8, 1, 1, 128, 40, 0], 3)[0] == 0                                # items of fewer than 64 rows
    assert _fused2(shim, [0, 1, 0, 8, 1, 1, 37, 210, 0], 3) == [0, 1, 0, 0, 8, 1, 4, 0, 2048, 1]   # ragged rows
    assert _fused2(shim, [0, 1, 1, 8, 2, 1, 128, 700, 0], 3)[0] == 0                               # interleaved complex
    assert _fused2(shim, [0, 0, 1, 8, 1, 1, 128, 700, 0], 3) == [0, 0, 0, 1, 8, 1, 4, 0, 2048, 1]  # the analysis has one family


# (plan, [route at (stride, dir) = (1, 0), (1, 1), (2, 0), (2, 1)], [cascade2_levels (analysis, left 2), (analysis, 3), (synthesis, 2),
# (synthesis, 3)]) -- the answers of the build before there were stacks
UNBATCHED = [
    ({'dims': [4096, 2048], 'lens': [8, 8]}, [(5, 8), (5, 8), (4, 8), (4, 8)], [2, 3, 2, 3]),
    ({'dims': [2048, 3073], 'lens': [8, 8]}, [(5, 8), (5, 8), (6, 0), (6, 0)], [2, 3, 2, 3]),
    ({'dims': [2048, 2048], 'lens': [8, 8], 'cplx': 1}, [(5, 8), (5, 8), (6, 0), (6, 0)], [2, 3, 2, 3]),
    ({'dims': [2048, 2048], 'lens': [8, 8], 'f64': 1}, [(5, 8), (5, 8), (4, 8), (4, 8)], [2, 3, 0, 0]),
    ({'dims': [4096, 4096], 'lens': [8, 8], 'f64': 1}, [(5, 8), (5, 8), (4, 8), (4, 8)], [2, 3, 2, 3]),
    ({'dims': [2048, 2048], 'lens': [8, 8], 'f64': 1, 'cplx': 1}, [(5, 8), (5, 8), (6, 0), (6, 0)], [2, 3, 2, 2]),
    ({'dims': [256, 96], 'lens': [4, 4], 'vf': 11, 'vi': 11}, [(5, 4), (5, 4), (4, 4), (4, 4)], [2, 3, 2, 3]),
    ({'dims': [256, 96], 'lens': [12, 12], 'vf': 11, 'vi': 11}, [(5, 12), (5, 12), (6, 0), (6, 0)], [2, 2, 0, 0]),
    ({'dims': [64, 40], 'lens': [4, 4], 'atrous': 1}, [(5, 4), (5, 4), (4, 4), (4, 4)], [0, 0, 0, 0]),
    ({'dims': [37, 21], 'lens': [18, 18], 'f64': 1}, [(6, 0), (6, 0), (6, 0), (6, 0)], [0, 0, 0, 0]),
    ({'dims': [64, 64, 64], 'lens': [8, 8, 8]}, [(1, 8), (1, 8), (0, 8), (0, 8)], [0, 0, 0, 0]),
    ({'dims': [64, 64, 64], 'lens': [4, 4, 4], 'atrous': 1, 'f64': 1}, [(1, 4), (1, 4), (0, 4), (0, 4)], [0, 0, 0, 0]),
    ({'dims': [24, 20, 18], 'lens': [4, 6, 8], 'cplx': 1}, [(1, 8), (1, 8), (6, 0), (6, 0)], [0, 0, 0, 0]),
    ({'dims': [24, 20, 18, 6], 'lens': [4, 4, 4, 4]}, [(2, 4), (2, 4), (6, 0), (6, 0)], [0, 0, 0, 0]),
]
# (Fused2Query: f64, inverse, vec4, Lp, ew, dil, n1, n2, variant_inv; the pick as stk_fused2 lays it out) -- likewise
ONE_IMAGE = [
    ([0, 1, 1, 8, 1, 1, 4096, 4096, 0], [1, 1, 0, 1, 8, 1, 4, 1, 1024, 1]),
    ([0, 1, 1, 8, 1, 1, 4096, 8192, 0], [0, 1, 0, 1, 8, 1, 4, 0, 2048, 1]),
    ([0, 1, 1, 8, 1, 1, 256, 40, 0], [0, 1, 0, 1, 8, 1, 4, 0, 2048, 1]),
    ([0, 1, 1, 8, 1, 1, 256, 64, 0], [1, 1, 0, 1, 8, 1, 4, 1, 1024, 1]),
    ([0, 1, 1, 12, 1, 1, 128, 700, 0], [1, 1, 0, 1, 12, 1, 4, 1, 1024, 1]),
    ([0, 1, 1, 6, 1, 1, 128, 700, 0], [1, 1, 0, 1, 6, 1, 2, 0, 1024, 1]),
    ([1, 1, 1, 4, 1, 1, 1024, 1024, 0], [1, 1, 1, 1, 4, 1, 4, 0, 1024, 1]),
    ([1, 1, 1, 8, 1, 1, 1024, 1024, 0], [1, 1, 1, 1, 8, 1, 2, 0, 1024, 1]),
    ([0, 1, 0, 8, 1, 1, 37, 210, 0], [0, 1, 0, 0, 8, 1, 4, 0, 2048, 1]),
    ([0, 1, 1, 8, 2, 1, 512, 512, 0], [0, 1, 0, 1, 8, 2, 4, 0, 2048, 1]),
    ([0, 0, 1, 8, 1, 1, 4096, 4096, 0], [0, 0, 0, 1, 8, 1, 4, 0, 2048, 1]),
    ([0, 1, 1, 8, 1, 1, 8192, 8192, 2], [1, 1, 0, 1, 8, 1, 2, 0, 2048, 1]),
    ([0, 1, 1, 8, 1, 1, 512, 512, 1], [0, 1, 0, 1, 8, 1, 4, 0, 2048, 1]),
    ([0, 1, 1, 8, 1, 2, 512, 512, 0], [0, 1, 0, 1, 8, 1, 4, 0, 2048, 1]),
]


def test_an_unbatched_plan_answers_what_it_always_answered(shim):
    assert len(UNBATCHED) >= 12 and len(ONE_IMAGE) >= 12
    for kw, routes, levels in UNBATCHED:
        p = _plan(**kw)
        got = [_route(shim, p, 0, stride, d) for stride in (1, 2) for d in (0, 1)]
        assert got == routes, (kw, got)
        got = [_levels(shim, p, 0, inverse, left) for inverse in (0, 1) for left in (2, 3)]
        assert got == levels, (kw, got)
    for q, pick in ONE_IMAGE:
        assert _fused2(shim, q, 1) == pick, (q, _fused2(shim, q, 1))
