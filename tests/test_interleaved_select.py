"""The selectors (csrc/ndwt_select.h) as a plan over interleaved samples (ndwt_plan_create_interleaved) asks them, without a device:
functions of integers, asked through tests/select/interleaved_shim.cpp.

  * inner > 1: level_route answers the per-axis passes whatever the shape, data kind, dilation and slab mode; cascade1_levels and
    cascade2_levels answer 0; fused_shrink_capable answers false (ndwt_denoise then runs dec, the shrink pass, rec);
  * cascadem_levels on both sides of every condition (one axis, inner > 1, the reference's dilation, path_auto, 2 .. 8 taps,
    comp * inner a multiple of 4, at least two levels left) and of every variant (9 off, 11 on, per direction);
  * every pick names an instance of the table, and the table is what the issue lists less the two instances that spill;
  * the unasked default: nothing is taken unasked below a kind's and direction's measured threshold, everything from it on
    (cascadem_min_bytes; LLONG_MAX where the cascade did not win: on request only);
  * inner = 1 answers exactly what the build before this one answered: a literal table, written down from that build.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED3_DILATED, FUSED3, FUSED3T, FUSED3FOLDT, FUSED2_DILATED, FUSED2, PER_AXIS = range(7)     # LevelRouteKind
KINDS = {"f32": (0, 0), "c64": (0, 1), "f64": (1, 0), "c128": (1, 1)}
NEVER = (1 << 63) - 1
LL = ctypes.c_longlong


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++ to compile tests/select/interleaved_shim.cpp")
    out = str(tmp_path_factory.mktemp("select_interleaved") / "libinterleaved_shim.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "select", "interleaved_shim.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    ip = ctypes.POINTER(ctypes.c_int)
    lib.il_level_route.argtypes = [ctypes.c_void_p, LL, LL, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip]
    lib.il_cascade1_levels.argtypes = [ctypes.c_void_p, LL, LL, ctypes.c_int, ctypes.c_int, ip]
    lib.il_cascade2_levels.argtypes = [ctypes.c_void_p, LL, LL, ctypes.c_int, ctypes.c_int, ip]
    lib.il_shrink_capable.argtypes = [ctypes.c_void_p, LL, LL]
    lib.il_cascadem_levels.argtypes = [ctypes.c_void_p, LL, LL, ctypes.c_int, ctypes.c_int, ip, ip]
    lib.il_cascadem_instantiated.argtypes = [ctypes.c_int] * 4
    lib.il_cascadem_default.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, LL]
    lib.il_cascadem_min_bytes.argtypes = [ctypes.c_int] * 3
    lib.il_cascadem_min_bytes.restype = LL
    return lib


def _plan(dims, lens, f64=0, cplx=0, atrous=0, vf=0, vi=0, path_auto=1):
    v = [len(dims), 2 if cplx else 1, f64, not cplx, path_auto, atrous, 1] + (list(dims) + [1] * 4)[:4] + (list(lens) + [2] * 4)[:4] + [vf, vi]
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _route(shim, plan, howmany, inner, stride, direction, slab=0):
    Lp = ctypes.c_int(-1)
    return shim.il_level_route(plan, howmany, inner, stride, direction, slab, ctypes.byref(Lp)), Lp.value


def _mlevels(shim, plan, howmany, inner, inverse, left):
    """(levels of the next cascaded march, its tap length, whether the table lists the instance)"""
    L, listed = ctypes.c_int(-1), ctypes.c_int(-1)
    n = shim.il_cascadem_levels(plan, howmany, inner, int(inverse), left, ctypes.byref(L), ctypes.byref(listed))
    return n, L.value, listed.value


def test_a_positional_selplan_has_inner_one(shim):
    """SelPlan{...} written without the new member (tests/select/*.cpp do) means inner = 1; with howmany given, still inner = 1"""
    assert shim.il_default_inner() == 111


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_interleaved_samples_take_the_per_axis_passes_and_no_other_cascade(shim, kind):
    f64, cplx = KINDS[kind]
    shapes = [([4096], [4]), ([2048, 2048], [4, 4]), ([64, 40], [8, 8]), ([24, 20, 20], [4, 4, 4]), ([16, 16, 16, 8], [4, 4, 4, 4])]
    for dims, lens in shapes:
        for atrous in (0, 1):
            for vf in (0, 10, 11):
                p = _plan(dims, lens, f64, cplx, atrous, vf, vf if vf != 10 else 12)
                for inner in (2, 3, 4, 1 << 20):
                    for K in (1, 3):
                        for stride in (1, 2, 4):
                            for d in (0, 1, -1):
                                for slab in (0, 1, 2):
                                    assert _route(shim, p, K, inner, stride, d, slab) == (PER_AXIS, 0), (dims, inner, K, stride, d, slab)
                        L = ctypes.c_int(-1)
                        for inv in (0, 1):
                            for left in (2, 3, 4):
                                assert shim.il_cascade1_levels(p, K, inner, inv, left, ctypes.byref(L)) == 0
                                assert shim.il_cascade2_levels(p, K, inner, inv, left, ctypes.byref(L)) == 0
                        assert shim.il_shrink_capable(p, K, inner) == 0
    # ... where inner = 1 of the same plans does take them (the questions above are not vacuous)
    assert _route(shim, _plan([64, 40], [8, 8], f64, cplx), 3, 1, 1, 0)[0] == FUSED2
    assert shim.il_shrink_capable(_plan([64, 40], [8, 8], f64, cplx), 3, 1) == 1
    L = ctypes.c_int(-1)
    assert shim.il_cascade1_levels(_plan([4096], [4], f64, cplx), 3, 1, 0, 3, ctypes.byref(L)) == 3
    assert shim.il_cascade2_levels(_plan([2048, 2048], [4, 4], f64, cplx, vf=11, vi=11), 0, 1, 0, 3, ctypes.byref(L)) >= 2


def _table(inverse, f64, L, nlev):
    """the instances the issue lists -- float and double, 2 / 4 / 6 / 8 taps, 2 .. 4 levels -- less the two that spill"""
    return L in (2, 4, 6, 8) and 2 <= nlev <= 4 and not (inverse and f64 and L == 8 and nlev >= 3)


def test_the_instance_table(shim):
    for inverse in (0, 1):
        for f64 in (0, 1):
            for L in range(0, 14):
                for nlev in range(0, 7):
                    assert shim.il_cascadem_instantiated(inverse, f64, L, nlev) == int(_table(inverse, f64, L, nlev)), (inverse, f64, L, nlev)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_cascadem_levels_on_both_sides_of_every_condition(shim, kind):
    f64, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    forced = dict(vf=11, vi=11)
    for inv in (0, 1):
        for L in (2, 4, 6, 8):
            for left in (2, 3, 4, 7):
                want = max(n for n in (2, 3, 4) if n <= left and _table(inv, f64, L, n))
                assert _mlevels(shim, _plan([64], [L], f64, cplx, **forced), 3, 8, inv, left) == (want, L, 1), (inv, L, left)
        ok = _plan([64], [4], f64, cplx, **forced)
        assert _mlevels(shim, ok, 3, 8, inv, 3)[0] == 3
        assert _mlevels(shim, ok, 1, 8, inv, 3)[0] == 3                                     # one item
        assert _mlevels(shim, ok, 3, 8, inv, 1)[0] == 0                                     # a single level left: nothing to cascade
        assert _mlevels(shim, ok, 3, 1, inv, 3)[0] == 0                                     # inner = 1: the batched 1-D plan, not this kernel
        assert _mlevels(shim, _plan([64, 40], [4, 4], f64, cplx, **forced), 3, 8, inv, 3)[0] == 0      # two filtered axes
        assert _mlevels(shim, _plan([64], [4], f64, cplx, atrous=1, **forced), 3, 8, inv, 3)[0] == 0   # a-trous
        assert _mlevels(shim, _plan([64], [4], f64, cplx, path_auto=0, **forced), 3, 8, inv, 3)[0] == 0
        assert _mlevels(shim, _plan([64], [10], f64, cplx, **forced), 3, 8, inv, 3)[0] == 0            # db5
        assert _mlevels(shim, _plan([64], [8], f64, cplx, **forced), 3, 8, inv, 3)[0] == (2 if (inv and f64) else 3)
        # comp * inner in whole groups of 4 scalars
        for inner in (2, 3, 4, 5, 6, 7, 8, 12, 30):
            assert (_mlevels(shim, ok, 3, inner, inv, 3)[0] == 3) == ((comp * inner) % 4 == 0), (inner, comp)
        # the variants, per direction: 9 off, 11 on; anything else = the default of the kind and direction
        for vf, vi in ((9, 11), (11, 9), (9, 9), (0, 11), (11, 0), (10, 12), (0, 0)):
            p = _plan([64], [4], f64, cplx, vf=vf, vi=vi)
            v = vi if inv else vf
            small = 8 * 64 * 3 * comp * (8 if f64 else 4)
            unasked = shim.il_cascadem_min_bytes(f64, comp, inv) <= small
            assert (_mlevels(shim, p, 3, 8, inv, 3)[0] == 3) == (v == 11 or (v != 9 and unasked)), (vf, vi, inv)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("inv", [0, 1], ids=["dec", "rec"])
def test_the_unasked_default_on_both_sides_of_its_threshold(shim, kind, inv):
    """nothing unasked one sample below the measured size of the kind and direction, the cascade from it on; 9 still switches it off"""
    f64, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    thr = shim.il_cascadem_min_bytes(f64, comp, inv)
    assert thr == MEASURED[(kind, "rec" if inv else "dec")]
    assert shim.il_cascadem_default(f64, comp, inv, 0) == 0 and shim.il_cascadem_default(f64, comp, inv, 1 << 20) == int(thr <= (1 << 20))
    if thr == NEVER:                                          # measured: no win -- on request only, whatever the size
        big = _plan([1 << 20], [4], f64, cplx)
        assert _mlevels(shim, big, 1 << 10, 1 << 12, inv, 3)[0] == 0
        assert shim.il_cascadem_default(f64, comp, inv, NEVER - 1) == 0
        return
    esz = comp * (8 if f64 else 4)
    inner, n = 64, 64
    K = thr // (esz * inner * n)
    assert K * esz * inner * n == thr and K >= 1              # the threshold is a whole number of such items
    p = _plan([n], [4], f64, cplx)
    assert _mlevels(shim, p, K, inner, inv, 3)[0] == 3
    if K > 1:
        assert _mlevels(shim, p, K - 1, inner, inv, 3)[0] == 0
    assert _mlevels(shim, _plan([n - 1], [4], f64, cplx), K, inner, inv, 3)[0] == 0
    off = _plan([n], [4], f64, cplx, vf=9, vi=9)
    assert _mlevels(shim, off, K, inner, inv, 3)[0] == 0


# the smallest whole array, in bytes, that takes the cascade unasked, per data kind and direction (the measured table and
# the rule); NEVER = on request only
MEASURED = {
    ("f32", "dec"): 256 << 20, ("f32", "rec"): 256 << 20, ("c64", "dec"): NEVER, ("c64", "rec"): NEVER,
    ("f64", "dec"): NEVER, ("f64", "rec"): NEVER, ("c128", "dec"): NEVER, ("c128", "rec"): NEVER,
}


# (dims, tap lengths, f64, complex, a-trous, howmany, variant fwd = inv) -> level_route (kind, Lp) for (stride 1 dec, stride 1 rec,
# stride 2 dec, stride 2 rec), then (cascade1_levels, L, cascade2_levels, Lp) of 3 levels left for dec and for rec, then
# fused_shrink_capable: the answers of the build before plans over interleaved samples existed
BEFORE = [
    ([4096], [4], 0, 0, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 0, 0, 0, 0, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 0, 0, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 3, 4, 0, 0, 3, 4, 0, 0, 0]),
    ([4096], [4], 0, 0, 0, 3, 11, [6, 0, 6, 0, 6, 0, 6, 0, 3, 4, 0, 0, 3, 4, 0, 0, 0]),
    ([4096], [4], 0, 0, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 0, 0, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 0, 1, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 0, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 3, 4, 0, 0, 3, 4, 0, 0, 0]),
    ([4096], [4], 0, 1, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 0, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 1, 0, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 1, 0, 0, 0, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 1, 0, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 3, 4, 0, 0, 3, 4, 0, 0, 0]),
    ([4096], [4], 1, 0, 0, 3, 11, [6, 0, 6, 0, 6, 0, 6, 0, 3, 4, 0, 0, 3, 4, 0, 0, 0]),
    ([4096], [4], 1, 0, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 1, 0, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 1, 1, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 1, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 3, 4, 0, 0, 3, 4, 0, 0, 0]),
    ([4096], [4], 1, 1, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([4096], [4], 1, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 0, 0, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 0, 0, 0, 0, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 0, 0, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 3, 8, 0, 0, 3, 8, 0, 0, 0]),
    ([96], [8], 0, 0, 0, 3, 11, [6, 0, 6, 0, 6, 0, 6, 0, 3, 8, 0, 0, 3, 8, 0, 0, 0]),
    ([96], [8], 0, 0, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 0, 0, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 0, 1, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 0, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 3, 8, 0, 0, 3, 8, 0, 0, 0]),
    ([96], [8], 0, 1, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 0, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 1, 0, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 1, 0, 0, 0, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 1, 0, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 3, 8, 0, 0, 3, 8, 0, 0, 0]),
    ([96], [8], 1, 0, 0, 3, 11, [6, 0, 6, 0, 6, 0, 6, 0, 3, 8, 0, 0, 3, 8, 0, 0, 0]),
    ([96], [8], 1, 0, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 1, 0, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 1, 1, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 1, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 3, 8, 0, 0, 3, 8, 0, 0, 0]),
    ([96], [8], 1, 1, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([96], [8], 1, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 0, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 0, 0, 0, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 0, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 0, 0, 3, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 0, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 0, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 1, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 1, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 0, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 0, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 0, 0, 0, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 0, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 0, 0, 3, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 0, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 0, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 1, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 1, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([100], [10], 1, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([2048, 2048], [4, 4], 0, 0, 0, 0, 0, [5, 4, 5, 4, 4, 4, 4, 4, 0, 0, 0, 4, 0, 0, 0, 4, 1]),
    ([2048, 2048], [4, 4], 0, 0, 0, 0, 11, [5, 4, 5, 4, 4, 4, 4, 4, 0, 0, 3, 4, 0, 0, 3, 4, 1]),
    ([2048, 2048], [4, 4], 0, 0, 0, 3, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 0, 4, 0, 0, 0, 4, 1]),
    ([2048, 2048], [4, 4], 0, 0, 0, 3, 11, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 3, 4, 0, 0, 3, 4, 1]),
    ([2048, 2048], [4, 4], 0, 0, 1, 0, 0, [5, 4, 5, 4, 4, 4, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([2048, 2048], [4, 4], 0, 0, 1, 3, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([2048, 2048], [4, 4], 0, 1, 0, 0, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 3, 4, 0, 0, 3, 4, 1]),
    ([2048, 2048], [4, 4], 0, 1, 0, 3, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 0, 4, 0, 0, 0, 4, 1]),
    ([2048, 2048], [4, 4], 0, 1, 1, 0, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([2048, 2048], [4, 4], 0, 1, 1, 3, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([2048, 2048], [4, 4], 1, 0, 0, 0, 0, [5, 4, 5, 4, 4, 4, 4, 4, 0, 0, 3, 4, 0, 0, 0, 4, 1]),
    ([2048, 2048], [4, 4], 1, 0, 0, 0, 11, [5, 4, 5, 4, 4, 4, 4, 4, 0, 0, 3, 4, 0, 0, 3, 4, 1]),
    ([2048, 2048], [4, 4], 1, 0, 0, 3, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 0, 4, 0, 0, 0, 4, 1]),
    ([2048, 2048], [4, 4], 1, 0, 0, 3, 11, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 3, 4, 0, 0, 3, 4, 1]),
    ([2048, 2048], [4, 4], 1, 0, 1, 0, 0, [5, 4, 5, 4, 4, 4, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([2048, 2048], [4, 4], 1, 0, 1, 3, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([2048, 2048], [4, 4], 1, 1, 0, 0, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 3, 4, 0, 0, 3, 4, 1]),
    ([2048, 2048], [4, 4], 1, 1, 0, 3, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 3, 4, 0, 0, 3, 4, 1]),
    ([2048, 2048], [4, 4], 1, 1, 1, 0, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([2048, 2048], [4, 4], 1, 1, 1, 3, 0, [5, 4, 5, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [8, 8], 0, 0, 0, 0, 0, [5, 8, 5, 8, 4, 8, 4, 8, 0, 0, 0, 8, 0, 0, 0, 8, 1]),
    ([64, 40], [8, 8], 0, 0, 0, 0, 11, [5, 8, 5, 8, 4, 8, 4, 8, 0, 0, 3, 8, 0, 0, 3, 8, 1]),
    ([64, 40], [8, 8], 0, 0, 0, 3, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 8, 0, 0, 0, 8, 1]),
    ([64, 40], [8, 8], 0, 0, 0, 3, 11, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 3, 8, 0, 0, 3, 8, 1]),
    ([64, 40], [8, 8], 0, 0, 1, 0, 0, [5, 8, 5, 8, 4, 8, 4, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [8, 8], 0, 0, 1, 3, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [8, 8], 0, 1, 0, 0, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 8, 0, 0, 0, 8, 1]),
    ([64, 40], [8, 8], 0, 1, 0, 3, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 8, 0, 0, 0, 8, 1]),
    ([64, 40], [8, 8], 0, 1, 1, 0, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [8, 8], 0, 1, 1, 3, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [8, 8], 1, 0, 0, 0, 0, [5, 8, 5, 8, 4, 8, 4, 8, 0, 0, 0, 8, 0, 0, 0, 8, 1]),
    ([64, 40], [8, 8], 1, 0, 0, 0, 11, [5, 8, 5, 8, 4, 8, 4, 8, 0, 0, 3, 8, 0, 0, 3, 8, 1]),
    ([64, 40], [8, 8], 1, 0, 0, 3, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 8, 0, 0, 0, 8, 1]),
    ([64, 40], [8, 8], 1, 0, 0, 3, 11, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 3, 8, 0, 0, 3, 8, 1]),
    ([64, 40], [8, 8], 1, 0, 1, 0, 0, [5, 8, 5, 8, 4, 8, 4, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [8, 8], 1, 0, 1, 3, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [8, 8], 1, 1, 0, 0, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 8, 0, 0, 0, 8, 1]),
    ([64, 40], [8, 8], 1, 1, 0, 3, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 8, 0, 0, 0, 8, 1]),
    ([64, 40], [8, 8], 1, 1, 1, 0, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [8, 8], 1, 1, 1, 3, 0, [5, 8, 5, 8, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 0, 0, 0, 0, 0, [5, 20, 5, 20, 6, 0, 6, 0, 0, 0, 0, 20, 0, 0, 0, 20, 1]),
    ([64, 40], [20, 4], 0, 0, 0, 0, 11, [5, 20, 5, 20, 6, 0, 6, 0, 0, 0, 0, 20, 0, 0, 0, 20, 1]),
    ([64, 40], [20, 4], 0, 0, 0, 3, 0, [5, 20, 5, 20, 6, 0, 6, 0, 0, 0, 0, 20, 0, 0, 0, 20, 1]),
    ([64, 40], [20, 4], 0, 0, 0, 3, 11, [5, 20, 5, 20, 6, 0, 6, 0, 0, 0, 0, 20, 0, 0, 0, 20, 1]),
    ([64, 40], [20, 4], 0, 0, 1, 0, 0, [5, 20, 5, 20, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 0, 0, 1, 3, 0, [5, 20, 5, 20, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 0, 1, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 0, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 0, 1, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 0, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 0, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 0, 0, 0, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 0, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 0, 0, 3, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 0, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 0, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 1, 0, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 1, 1, 0, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([64, 40], [20, 4], 1, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([24, 20, 20], [4, 4, 4], 0, 0, 0, 0, 0, [1, 4, 1, 4, 0, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 0, 0, 0, 0, 11, [1, 4, 1, 4, 0, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 0, 0, 0, 3, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 0, 0, 0, 3, 11, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 0, 0, 1, 0, 0, [1, 4, 1, 4, 0, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([24, 20, 20], [4, 4, 4], 0, 0, 1, 3, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([24, 20, 20], [4, 4, 4], 0, 1, 0, 0, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 0, 1, 0, 3, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 0, 1, 1, 0, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([24, 20, 20], [4, 4, 4], 0, 1, 1, 3, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([24, 20, 20], [4, 4, 4], 1, 0, 0, 0, 0, [1, 4, 1, 4, 0, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 1, 0, 0, 0, 11, [1, 4, 1, 4, 0, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 1, 0, 0, 3, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 1, 0, 0, 3, 11, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 1, 0, 1, 0, 0, [1, 4, 1, 4, 0, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([24, 20, 20], [4, 4, 4], 1, 0, 1, 3, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([24, 20, 20], [4, 4, 4], 1, 1, 0, 0, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 1, 1, 0, 3, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([24, 20, 20], [4, 4, 4], 1, 1, 1, 0, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([24, 20, 20], [4, 4, 4], 1, 1, 1, 3, 0, [1, 4, 1, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 0, 0, 0, 0, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 0, 0, 0, 11, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 0, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 0, 0, 3, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 0, 1, 0, 0, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 0, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 1, 0, 0, 0, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 1, 1, 0, 0, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 0, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 0, 0, 0, 0, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 0, 0, 0, 11, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 0, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 0, 0, 3, 11, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 0, 1, 0, 0, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 0, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 1, 0, 0, 0, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 1, 0, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 1, 1, 0, 0, [2, 4, 2, 4, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ([16, 16, 16, 8], [4, 4, 4, 4], 1, 1, 1, 3, 0, [6, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
]


def test_inner_one_answers_what_it_answered_before(shim):
    assert len(BEFORE) == 160
    for dims, lens, f64, cplx, atrous, K, v, want in BEFORE:
        p = _plan(dims, lens, f64, cplx, atrous, v, v)
        got = []
        for stride in (1, 2):
            for d in (0, 1):
                got += list(_route(shim, p, K, 1, stride, d))
        Lp = ctypes.c_int(0)
        for inv in (0, 1):
            n = shim.il_cascade1_levels(p, K, 1, inv, 3, ctypes.byref(Lp))
            got += [n, Lp.value]
            n = shim.il_cascade2_levels(p, K, 1, inv, 3, ctypes.byref(Lp))
            got += [n, Lp.value]
        got.append(shim.il_shrink_capable(p, K, 1))
        assert got == want, (dims, lens, f64, cplx, atrous, K, v)
        for inv in (0, 1):                                    # and the new cascade never applies to them
            assert _mlevels(shim, p, K, 1, inv, 3)[0] == 0
