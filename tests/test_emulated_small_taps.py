"""The emulated kernels (tests/emu: the kernel source compiled for the host) under the componentwise bound of tests/bound_cases.py.

Every case runs an emulator entry point on comb inputs -- impulses on the first and last sample of every axis and either side of the
tile, chunk and wave-row edges -- and holds the output to |got - want| <= c u |W||x| at every element, with exact zeros where no tap
reaches (c = sum over the axes of (L_a + 2) for the one level an entry point computes, times the levels of a cascade).  The entry points
take their taps as arguments, so every case also makes the negative run: the kernel gets a table in which the smallest coefficient of one
axis' wavelet (h[L - 1]: the first low-pass and the last high-pass tap) is off by 1e-4 of itself, the oracle keeps the true one, and the
check must fail -- on the kernel source itself, this suite would notice.

The tables of tests/emu/ndwt_emu.cpp take every tap length used here: AxisMarch 2 .. 20, AxisX 10 and 12, Fwd2S / Inv2S 14 .. 20 (pairs:
10 .. 16), Fwd3 with 18 taps on its 512-thread tile, Fwd3 and Inv3S with 14 and 16 taps on the small test tile.  A double case is held
against the float64 oracle: two double computations, each within its own share of the bound.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bound_cases as bc
import ndwt_oracle as orc
from helpers import to_kernel_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = bc.U["single"]
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    asan = "libclang_rt.asan" in os.environ.get("LD_PRELOAD", "")
    target = "libndwt_emu.so" if asan else "libndwt_emu_plain.so"
    subprocess.check_call(["make", "-s", "-j", str(min(8, os.cpu_count() or 1)), "-C", os.path.join(ROOT, "tests", "emu"), target])
    return ctypes.CDLL(os.path.join(ROOT, "tests", "emu", target))


def ktaps(filt, l2, inverse, Lp=None, rows=3):
    """kernel-form taps of the filter pairs (what helpers.kernel_taps builds from a wavelet's name), zero-padded to Lp: lo, hi [rows, 20]"""
    Lp = Lp or max(len(f[0]) for f in filt)
    c, cs = (1 / np.sqrt(2.0), 1 / np.sqrt(2.0)) if l2 else (1.0, 0.5)
    lo, hi = np.zeros((rows, 20)), np.zeros((rows, 20))
    for ax, (lo_d, hi_d) in enumerate(filt):
        pad = (Lp - len(lo_d)) // 2
        lo[ax, pad:pad + len(lo_d)] = cs * lo_d if inverse else c * lo_d[::-1]
        hi[ax, pad:pad + len(hi_d)] = cs * hi_d if inverse else c * hi_d[::-1]
    return Lp, lo, hi


# ---- the entry points of libndwt_emu: arrays of the oracle's shape in, arrays of the oracle's shape out
def run3(emu, arr, filt, l2, inverse, vec4=True, zchunk=0, small=True, variant=0, cplx=False, dil=1, dtype=np.float32):
    Lp, lo, hi = ktaps(filt, l2, inverse)
    cdt = (np.complex64 if dtype == np.float32 else np.complex128) if cplx else dtype
    src = to_kernel_order(arr).astype(cdt)
    n3, n2, n1 = src.shape[1:] if inverse else src.shape
    out = np.full((n3, n2, n1) if inverse else (8, n3, n2, n1), np.nan, dtype=cdt)
    fn = emu.ndwt_emu3_f32 if dtype == np.float32 else emu.ndwt_emu3_f64
    fn.restype = ctypes.c_int
    rc = fn(int(inverse), Lp, int(vec4), P(src), P(out), n1 * (2 if cplx else 1), n2, n3, 1, zchunk, P(lo), P(hi), 1, int(small), int(variant),
            2 if cplx else 1, ctypes.c_double(0.0), 0, 0, int(dil), None, None)
    assert rc == 0, rc
    return np.transpose(out)


def pin3(emu, x, filt, l2, zchunk=0, **_):
    Lp, lo, hi = ktaps(filt, l2, False)
    xs = to_kernel_order(x).astype(np.float32)
    out = np.full((8,) + xs.shape, np.nan, dtype=np.float32)
    n3, n2, n1 = xs.shape
    assert emu.ndwt_emu_pin3_f32(Lp, P(xs), P(out), n1, n2, n3, zchunk, P(lo), P(hi), 1, None, None) == 0
    return np.transpose(out)


def low3(emu, x, filt, l2, vec4=True, zchunk=0, **_):
    Lp, lo, hi = ktaps(filt, l2, False)
    xs = to_kernel_order(x).astype(np.float32)
    out = np.full(xs.shape, np.nan, dtype=np.float32)
    n3, n2, n1 = xs.shape
    assert emu.ndwt_emu_low3_f32(Lp, int(vec4), P(xs), P(out), n1, n2, n3, zchunk, P(lo), P(hi)) == 0
    return np.transpose(out)[..., None]


def tpre(emu, x, filt, l2, zchunk=0, **_):
    Lp, lo, hi = ktaps(filt[:3], l2, False)
    _, tl, th = ktaps(filt[3:], l2, False, Lp, rows=1)
    xs = to_kernel_order(x).astype(np.float32)
    out = np.full((16,) + xs.shape, np.nan, dtype=np.float32)
    n4, n3, n2, n1 = xs.shape
    assert emu.ndwt_emu_tpre_f32(Lp, P(xs), P(out), n1, n2, n3, n4, zchunk, P(lo), P(hi), P(np.ascontiguousarray(tl[0])), P(np.ascontiguousarray(th[0]))) == 0
    return np.transpose(out)


def run2(emu, arr, filt, l2, inverse, vec4=True, ychunk=0, cplx=False, dil=1, dtype=np.float32, **_):
    Lp, lo, hi = ktaps(filt, l2, inverse)
    cdt = (np.complex64 if dtype == np.float32 else np.complex128) if cplx else dtype
    src = to_kernel_order(arr).astype(cdt)
    n2, n1 = src.shape[1:] if inverse else src.shape
    out = np.full((n2, n1) if inverse else (4, n2, n1), np.nan, dtype=cdt)
    fn = emu.ndwt_emu2_f32 if dtype == np.float32 else emu.ndwt_emu2_f64
    fn.restype = ctypes.c_int
    rc = fn(int(inverse), Lp, int(vec4), P(src), P(out), n1 * (2 if cplx else 1), n2, ychunk, P(lo), P(hi), 1, 2 if cplx else 1, ctypes.c_double(0.0), 0, 0,
            int(dil))
    assert rc == 0, rc
    return np.transpose(out)


def inv2p(emu, c, filt, l2, inverse=True, depth=2, ychunk=0, **_):
    Lp, lo, hi = ktaps(filt, l2, True)
    src = to_kernel_order(c).astype(np.float32)
    n2, n1 = src.shape[1:]
    out = np.full((n2, n1), np.nan, dtype=np.float32)
    assert emu.ndwt_emu2_inv2p_f32(Lp, depth, P(src), P(out), n1, n2, ychunk, P(lo), P(hi), ctypes.c_double(0.0), 0, 0) == 0
    return np.transpose(out)


def cascade2(emu, arr, filt, l2, inverse, nlev=2, depth=1, ychunk=0, **_):
    Lp, lo, hi = ktaps(filt, l2, inverse)
    src = to_kernel_order(arr).astype(np.float32)
    n2, n1 = src.shape[-2:]
    out = np.full((n2, n1) if inverse else (1 + 3 * nlev, n2, n1), np.nan, dtype=np.float32)
    if inverse:
        rc = emu.ndwt_emu2_cascade_inv_f32(Lp, nlev, depth, P(src), P(out), n1, n2, ychunk, P(lo), P(hi))
    else:
        rc = emu.ndwt_emu2_cascade_f32(Lp, nlev, P(src), P(out), n1, n2, ychunk, P(lo), P(hi))
    assert rc == 0, rc
    return np.transpose(out)


# ---- one case: the entry point on every comb under the bound, then the negative run
def _level(direction, v, filt, l2, stride, levels):
    if levels > 1:
        return bc.walk_dec(v, filt, levels, l2) if direction == "dec" else bc.walk_rec(v, filt, l2, level=levels)
    return orc.spatial_level_dec(v, filt, l2, stride) if direction == "dec" else orc.spatial_level_rec(v, filt, l2, stride)


def hold(name, call, direction, shape, wn, l2, edges, cplx=False, stride=1, levels=1, u=U32, mutate_axis=0, bands=None):
    """call(input, filter pairs) -> output.  True taps: every comb passes the bound (the worst ratio is printed).  Then the kernel gets the
    smallest low-pass tap of `mutate_axis` off by 1e-4 of itself while the oracle keeps the true one: some comb must fail the check.
    bands: the output holds only these bands of the level (the approximation-only analysis)"""
    d = len(shape)
    filt = bc.filters(list(wn) if not isinstance(wn, str) else wn, d)
    c = levels * sum(len(f[0]) + 2 for f in filt)
    pos = [bc.axis_positions(n, e) for n, e in zip(shape, edges)]
    reach = [(len(f[0]) - 1) * stride + 1 if levels == 1 else levels * len(f[0]) for f in filt]
    if direction == "dec":
        ins = [(None, x) for x in bc.combs(shape, pos, reach, cplx, pairs=True)]
    else:
        ins = bc.rec_combs(shape, pos, reach, levels, cplx, pairs=True)
    bad_filt = bc.mutate(filt, 1e-4, axes=[mutate_axis])        # lo[0] and hi[L - 1]: the one coefficient h[L - 1] in both its places
    worst, caught = 0.0, False
    for m, (band, v) in enumerate(ins):
        want = _level(direction, v, filt, l2, stride, levels)
        cond = _level(direction, bc.magnitude(v), bc.abs_filters(filt), l2, stride, levels)
        if bands is not None:
            want, cond = want[..., bands], cond[..., bands]
        worst = max(worst, bc.check_componentwise(call(v, filt), want, cond, c, u, f"{name} comb {m} band {band}"))
        if not caught and (direction == "dec" or band == 0):     # (a comb in a detail band meets the low-pass taps of the other axes only)
            try:
                bc.check_componentwise(call(v, bad_filt), want, cond, c, u)
            except AssertionError:
                caught = True
    print(f"[emu-small-taps] {name}: worst {worst:.3g} u cond (cap {c}); the 1e-4 mutant of axis {mutate_axis} {'fails' if caught else 'PASSES'} the check")
    assert caught, f"{name}: a kernel whose smallest low-pass tap on axis {mutate_axis} is off by 1e-4 passes the check"
    return worst


def E(n, *tiles):
    return sorted({e for t in tiles for e in bc.tile_edges(n, t, anchor_last=True)})


# ---- the fused 3-D forms
FWD3 = [
    # id, shape, wavelets, kwargs of run3, edges
    ("fwd3-small-12", (24, 22, 21), ("db6", "db4", "db5"), dict(vec4=True, zchunk=7), [E(24, 16), E(22, 8), [7, 14]]),
    ("fwd3-small-12-ragged", (21, 19, 13), ("db5", "db6", "db6"), dict(vec4=False, zchunk=5), [E(21, 16), E(19, 8), [5, 10]]),
    ("fwd3-prod-8", (68, 18, 9), "db4", dict(vec4=True, small=False), [E(68, 64), E(18, 16), []]),
    ("fwd3-prod-8-one-column", (70, 19, 10), "db4", dict(vec4=False, small=False, variant=1, zchunk=6), [E(70, 64), E(19, 16), [6]]),
    ("fwd3-small-16", (24, 22, 21), ("db8", "db6", "db7"), dict(vec4=True, zchunk=7), [E(24, 16), E(22, 8), [7, 14]]),
    ("fwd3-small-14-ragged", (21, 19, 17), "db7", dict(vec4=False, zchunk=6), [E(21, 16), E(19, 8), [6, 12]]),
    ("fwd3-small-16-f64", (24, 18, 17), "db8", dict(vec4=True, zchunk=6, dtype=np.float64), [E(24, 16), E(18, 8), [6, 12]]),
    ("fwd3-c64-12", (14, 15, 13), ("db6", "db5", "db6"), dict(vec4=True, zchunk=5, cplx=True), [E(14, 8), E(15, 8), [5, 10]]),
]


@pytest.mark.slow
@pytest.mark.parametrize("cid,shape,wn,kw,edges", FWD3, ids=[c[0] for c in FWD3])
def test_fwd3(emu, cid, shape, wn, kw, edges):
    for l2 in (0, 1):
        hold(f"{cid} l2={l2}", lambda v, f: run3(emu, v, f, l2, False, **kw), "dec", shape, wn, l2, edges, cplx=kw.get("cplx", False),
             mutate_axis=l2, u=bc.U["double"] if kw.get("dtype") is np.float64 else U32)


PIN3 = [("pin-10", (68, 36, 11), ("db5", "db3", "db5"), 4), ("pin-12", (68, 36, 13), "db6", 0), ("pin-14", (64, 34, 16), ("db7", "db5", "db7"), 6),
        ("wlds2-16", (68, 36, 18), "db8", 7), ("long-18", (68, 20, 20), "db9", 9), ("wlds4-20", (68, 20, 22), ("db10", "db6", "db8"), 9)]


@pytest.mark.slow
@pytest.mark.parametrize("cid,shape,wn,zchunk", PIN3, ids=[c[0] for c in PIN3])
def test_fwd3_pinned_taps_and_window_slots_in_lds(emu, cid, shape, wn, zchunk):
    """Fwd3 PIN (10 / 12 / 14 taps), WLDS = 2 (16), the 512-thread tile at 18 taps and WLDS = 4 (20), on their production tiles"""
    L = max(len(f[0]) for f in bc.filters(wn, 3))
    ty = 16 if L >= 18 else 32
    edges = [E(shape[0], 64), E(shape[1], ty), list(range(zchunk, shape[2], zchunk)) if zchunk else []]
    for l2, ax in ((1, 0), (0, 2)):
        hold(f"{cid} l2={l2}", lambda v, f: pin3(emu, v, f, l2, zchunk), "dec", shape, wn, l2, edges, mutate_axis=ax)


@pytest.mark.slow
def test_fwd3_approximation_only_and_folded_t(emu):
    """Fwd3 LOWONLY (band 0 alone) and TPRE (the t axis of a 4-D level folded in), 8 taps on the tall tile"""
    hold("low3-8", lambda v, f: low3(emu, v, f, 1, True, 4), "dec", (68, 36, 9), "db4", 1, [E(68, 64), E(36, 32), [4, 8]], bands=[0], mutate_axis=1)
    hold("low3-8-ragged", lambda v, f: low3(emu, v, f, 0, False, 5), "dec", (70, 33, 12), ("db3", "db4", "db4"), 0, [E(70, 64), E(33, 32), [5, 10]],
         bands=[0], mutate_axis=2)
    hold("tpre-8", lambda v, f: tpre(emu, v, f, 1, 4), "dec", (68, 36, 6, 9), "db4", 1, [E(68, 64), E(36, 32), [4], []], mutate_axis=3)   # (9 frames: the 8 t taps land on 8 samples)


INV3 = [
    # id, shape, wavelets, kwargs of run3, edges (16 x 8 test tile unless small=False)
    ("inv3-lds-12", (20, 17, 13), ("db6", "db4", "db6"), dict(variant=0, zchunk=5), [E(20, 16), E(17, 8), [5, 10]]),
    ("inv3s-12", (24, 19, 13), ("db6", "db5", "db4"), dict(variant=2, zchunk=5), [E(24, 16), E(19, 8), [5, 10]]),
    ("inv3s-12-ragged", (21, 14, 12), ("db5", "db3", "db6"), dict(variant=2, vec4=False, zchunk=5), [E(21, 16), E(14, 8), [5, 10]]),
    ("inv3s-16", (24, 19, 17), ("db8", "db7", "db7"), dict(variant=2, zchunk=6), [E(24, 16), E(19, 8), [6, 12]]),
    ("inv3s-14-ragged", (21, 15, 15), ("db7", "db6", "db6"), dict(variant=2, vec4=False), [E(21, 16), E(15, 8), []]),
    ("inv3s-16-f64", (24, 18, 17), "db8", dict(variant=2, zchunk=6, dtype=np.float64), [E(24, 16), E(18, 8), [6, 12]]),
    ("inv3s-prod-8", (68, 39, 9), "db4", dict(variant=1, small=False), [E(68, 64), E(39, 32), []]),
    ("inv3s-c64-12", (13, 12, 12), ("db6", "db2", "db4"), dict(variant=0, vec4=False, cplx=True), [E(13, 8), E(12, 8), []]),
    ("inv3y-gather-20", (24, 22, 21), "db10", dict(variant=5), [E(24, 16), E(22, 8), []]),
    ("inv3y-gather-20-depth2", (24, 22, 21), ("db10", "db8", "db10"), dict(variant=8, zchunk=9), [E(24, 16), E(22, 8), [9, 18]]),
    ("inv3y-gather-18-ragged", (23, 19, 18), ("db9", "db7", "db5"), dict(variant=5, vec4=False, zchunk=6), [E(23, 16), E(19, 8), [6, 12]]),
    ("inv3y-gather-14", (24, 23, 19), "db7", dict(variant=8), [E(24, 16), E(23, 8), []]),
    ("inv3y-scatter-20", (24, 22, 21), "db10", dict(variant=10), [E(24, 16), E(22, 8), []]),
    ("inv3y-scatter-18", (20, 26, 20), ("db9", "db9", "db7"), dict(variant=10, zchunk=7), [E(20, 16), E(26, 8), [7, 14]]),
    ("inv3y-scatter-16", (28, 20, 21), ("db8", "db8", "db4"), dict(variant=10, zchunk=7), [E(28, 16), E(20, 8), [7, 14]]),
    ("inv3y-scatter-10", (24, 21, 13), "db5", dict(variant=10), [E(24, 16), E(21, 8), []]),
    ("inv3y-scatter-prod-20", (52, 30, 9), "db10", dict(variant=10, small=False), [E(52, 48), E(30, 28), []]),
    ("inv3y-scatter-prod-12-uniyz", (72, 37, 12), "db6", dict(variant=10, small=False), [E(72, 64), E(37, 32), []]),
    ("inv3y-gather-prod-12", (72, 37, 12), "db6", dict(variant=8, small=False), [E(72, 64), E(37, 32), []]),
    ("inv3y-c64-gather-16", (21, 16, 16), "db8", dict(variant=5, vec4=False, cplx=True), [E(21, 8), E(16, 8), []]),
    ("inv3y-c64-gather-14-depth2", (22, 17, 15), "db7", dict(variant=8, cplx=True), [E(22, 8), E(17, 8), []]),
    ("inv3y-c64-scatter-16", (24, 18, 17), ("db8", "db6", "db4"), dict(variant=10, zchunk=7, cplx=True), [E(24, 8), E(18, 8), [7, 14]]),
    ("inv3y-c64-scatter-prod-12", (50, 35, 8), ("db6", "db6", "db4"), dict(variant=10, zchunk=4, small=False, cplx=True), [E(50, 24), E(35, 32), [4]]),
]


@pytest.mark.slow
@pytest.mark.parametrize("cid,shape,wn,kw,edges", INV3, ids=[c[0] for c in INV3])
def test_inv3(emu, cid, shape, wn, kw, edges):
    """Inv3, Inv3S and Inv3Y in its gather and scatter forms, one and two register sets, real data and (re, im) pairs"""
    l2 = len(cid) % 2
    hold(f"{cid} l2={l2}", lambda v, f: run3(emu, v, f, l2, True, **kw), "rec", shape, wn, l2, edges, cplx=kw.get("cplx", False),
         mutate_axis=len(cid) % 3, u=bc.U["double"] if kw.get("dtype") is np.float64 else U32)


DIL3 = [("fwd3-dil2", "dec", (72, 16, 6), ("db2", "db4", "db1"), dict(small=False, dil=2), 2),
        ("fwd3-dil4", "dec", (72, 16, 8), ("db4", "db3", "db2"), dict(small=False, dil=4), 4),
        ("inv3s-dil4", "rec", (72, 16, 8), ("db4", "db3", "db2"), dict(small=False, dil=4), 4),
        ("inv3y-dil2", "rec", (136, 68, 6), "db4", dict(small=False, dil=2, variant=8), 2),
        ("inv3y-dil4-gather", "rec", (72, 16, 8), "db2", dict(small=False, dil=4, variant=5), 4),
        ("inv3y-dil4-scatter", "rec", (264, 104, 8), ("db4", "db2", "db4"), dict(small=False, dil=4, variant=10), 4)]


@pytest.mark.slow
@pytest.mark.parametrize("cid,direction,shape,wn,kw,dil", DIL3, ids=[c[0] for c in DIL3])
def test_dilated_levels_on_sublattices(emu, cid, direction, shape, wn, kw, dil):
    """a level at tap stride 2 / 4 through EW = 2 / 4: Fwd3, Inv3S, and Inv3Y in its interleaved-pair, whole-lane and scatter forms"""
    edges = [E(shape[0], 64), [shape[1] // 2], []]
    hold(cid, lambda v, f: run3(emu, v, f, 1, direction == "rec", **kw), direction, shape, wn, 1, edges, stride=dil, mutate_axis=0)


@pytest.mark.slow
def test_den3_with_threshold_zero(emu):
    """Den3 at threshold 0: the detail bands recomputed from x on the haloed tile, synthesised with a given approximation band.  Two inputs:
    want = rec([apx, details(x)]), cond = |W^-1| [|apx|, |W| |x| details].  The cap adds the analysis (L + 2 per axis) to a synthesis in which
    every band is non-zero, so each pass sums low-pass and high-pass products: 2 L + 2 per axis"""
    shape, wn, zchunk = (68, 36, 9), "db4", 4
    filt = bc.filters(wn, 3)
    L = 8
    c = 3 * (L + 2) + 3 * (2 * L + 2)
    pos = [bc.axis_positions(n, e) for n, e in zip(shape, [E(68, 64), E(36, 32), [4, 8]])]
    xs = bc.combs(shape, pos, [L] * 3, pairs=True)
    worst, caught = 0.0, False
    for l2 in (1, 0):
        for m, x in enumerate(xs):
            apx = np.roll(xs[(m + 1) % len(xs)], 3, axis=0) * 0.75
            cf = orc.spatial_level_dec(x, filt, l2)
            cf[..., 0] = apx
            want = orc.spatial_level_rec(cf, filt, l2)
            ca = orc.spatial_level_dec(np.abs(x), bc.abs_filters(filt), l2)
            ca[..., 0] = np.abs(apx)
            cond = orc.spatial_level_rec(ca, bc.abs_filters(filt), l2)

            def call(f):
                _, slo, shi = ktaps(f, l2, True)
                _, alo, ahi = ktaps(f, l2, False)
                xk, ak = to_kernel_order(x).astype(np.float32), to_kernel_order(apx).astype(np.float32)
                out = np.full(xk.shape, np.nan, dtype=np.float32)
                n3, n2, n1 = xk.shape
                assert emu.ndwt_emu_den3_f32(L, P(xk), P(ak), P(out), n1, n2, n3, zchunk, P(slo), P(shi), P(alo), P(ahi), ctypes.c_double(0.0), 0) == 0
                return np.transpose(out)
            worst = max(worst, bc.check_componentwise(call(filt), want, cond, c, U32, f"den3 l2={l2} comb {m}"))
            if not caught:
                try:
                    bc.check_componentwise(call(bc.mutate(filt, 1e-4, axes=[1])), want, cond, c, U32)
                except AssertionError:
                    caught = True
    print(f"[emu-small-taps] den3-8 threshold 0: worst {worst:.3g} u cond (cap {c}); the 1e-4 mutant {'fails' if caught else 'PASSES'} the check")
    assert caught


# ---- images: Fwd2S / Inv2S (run2), Inv2P, the cascade
RUN2 = [("2s-20", (260, 24), ("db10", "db7"), dict(vec4=True, ychunk=9)), ("2s-18-ragged", (250, 22), ("db6", "db9"), dict(vec4=False, ychunk=8)),
        ("2s-16", (240, 20), "db8", dict(vec4=True, ychunk=7)), ("2s-14-ragged", (255, 19), ("db7", "db5"), dict(vec4=False)),
        ("2s-12", (252, 30), ("db6", "db5"), dict(vec4=True, ychunk=11)),
        ("2s-c64-16", (124, 20), "db8", dict(vec4=True, ychunk=7, cplx=True)), ("2s-c64-14-ragged", (125, 18), ("db7", "db6"), dict(vec4=False, cplx=True)),
        ("2s-c64-10", (126, 16), ("db4", "db5"), dict(vec4=True, ychunk=6, cplx=True))]


def _wx(syn, L, ew):
    LH, RH = (L // 2, L // 2 - 1) if syn else (L // 2 - 1, L // 2)
    return 4 * (64 - (LH * ew + 3) // 4 - (RH * ew + 3) // 4) // ew


@pytest.mark.slow
@pytest.mark.parametrize("cid,shape,wn,kw", RUN2, ids=[c[0] for c in RUN2])
def test_fused2(emu, cid, shape, wn, kw):
    """Fwd2S / Inv2S at 12 .. 20 taps, and on (re, im) pairs at 10 .. 16"""
    cplx = kw.get("cplx", False)
    L = max(len(f[0]) for f in bc.filters(wn, 2))
    yc = kw.get("ychunk", 0)
    edges = [E(shape[0], _wx(False, L, 2 if cplx else 1)), list(range(yc, shape[1], yc)) if yc else []]
    hold(f"{cid} dec", lambda v, f: run2(emu, v, f, 1, False, **kw), "dec", shape, wn, 1, edges, cplx=cplx, mutate_axis=0)
    hold(f"{cid} rec", lambda v, f: run2(emu, v, f, 0, True, **kw), "rec", shape, wn, 0, edges, cplx=cplx, mutate_axis=1)


@pytest.mark.slow
@pytest.mark.parametrize("depth", [2, 4, 14])
def test_inv2p_12_taps(emu, depth):
    """Inv2P at 12 taps: two and four rows of band loads in flight, and the packed form (depth 14)"""
    shape, yc = (248, 30), 11
    edges = [E(248, _wx(True, 12, 1)), [11, 22]]
    hold(f"inv2p-12-depth{depth}", lambda v, f: inv2p(emu, v, f, 1, depth=depth, ychunk=yc), "rec", shape, "db6", 1, edges, mutate_axis=depth % 2)


@pytest.mark.slow
def test_cascade2(emu):
    """Fwd2C with 12 taps at two levels and 8 at three; Inv2C with 8 taps at three levels, one and two rows in flight"""
    def wxc(syn, L, nlev):
        LH, RH = (L // 2, L // 2 - 1) if syn else (L // 2 - 1, L // 2)
        return 4 * ((64 - nlev * ((LH + 3) // 4 + (RH + 3) // 4)) // 8 * 8)
    hold("fwd2c-12-2", lambda v, f: cascade2(emu, v, f, 1, False, nlev=2, ychunk=20), "dec", (244, 45), "db6", 1, [E(244, wxc(False, 12, 2)), [20, 40]],
         levels=2, mutate_axis=0)
    hold("fwd2c-8-3", lambda v, f: cascade2(emu, v, f, 0, False, nlev=3, ychunk=13), "dec", (244, 30), ("db4", "db3"), 0, [E(244, wxc(False, 8, 3)), [13, 26]],
         levels=3, mutate_axis=0)
    for depth in (1, 2):
        hold(f"inv2c-8-3-depth{depth}", lambda v, f: cascade2(emu, v, f, 1, True, nlev=3, depth=depth, ychunk=13), "rec", (244, 30), ("db4", "db2"), 1,
             [E(244, wxc(True, 8, 3)), [13, 26]], levels=3, mutate_axis=0)


# ---- the per-axis passes: one filter pair along axis 1 of [outer, n, inner] (AxisMarch) or along the rows of [outer, n] (AxisX)
def _axis_hold(name, call_dec, call_rec, shape, wn, edges, cplx=False, u=U32):
    """dec: x -> (lo, hi); rec: (a, d) -> r, with the comb in one of the two bands.  c = L + 2"""
    lo_d, hi_d = orc.wave_filters(wn)
    L, s = len(lo_d), 1 / np.sqrt(2.0)
    cap = L + 2
    bad = bc.mutate([(lo_d, hi_d)], 1e-4)[0]
    pos = bc.axis_positions(shape[1], edges)
    worst, caught = 0.0, [False, False]
    for m, comb in enumerate(bc.combs([shape[1]], [pos], [L], cplx, pairs=True)):
        x = np.zeros(shape, dtype=comb.dtype)
        for idx in np.ndindex(shape[0], *shape[2:]):             # the comb in every column, scaled by another exact amplitude
            x[(idx[0], slice(None)) + idx[1:]] = comb * abs(bc.amplitude(sum(idx) + idx[0]))
        mag = bc.magnitude(x)
        want = orc._analysis_axis(x, lo_d, hi_d, 1, s, 1)
        cond = orc._analysis_axis(mag, np.abs(lo_d), np.abs(hi_d), 1, s, 1)
        got = call_dec(x, (lo_d, hi_d))
        for b in range(2):
            worst = max(worst, bc.check_componentwise(got[b], want[b], cond[b], cap, u, f"{name} dec comb {m} band {b}"))
        if not caught[0]:
            try:
                bc.check_componentwise(call_dec(x, bad)[0], want[0], cond[0], cap, u)
            except AssertionError:
                caught[0] = True
        zero = np.zeros_like(x)
        for b, (a_in, d_in) in enumerate(((x, zero), (zero, x))):
            want_r = orc._synthesis_axis(a_in, d_in, lo_d, hi_d, 1, s, 1)
            cond_r = orc._synthesis_axis(bc.magnitude(a_in), bc.magnitude(d_in), np.abs(lo_d), np.abs(hi_d), 1, s, 1)
            worst = max(worst, bc.check_componentwise(call_rec(a_in, d_in, (lo_d, hi_d)), want_r, cond_r, cap, u, f"{name} rec comb {m} band {b}"))
            if b == 0 and not caught[1]:
                try:
                    bc.check_componentwise(call_rec(a_in, d_in, bad), want_r, cond_r, cap, u)
                except AssertionError:
                    caught[1] = True
    print(f"[emu-small-taps] {name}: worst {worst:.3g} u cond (cap {cap}); the 1e-4 mutant fails the check: dec {caught[0]}, rec {caught[1]}")
    assert all(caught), (name, caught)


MARCH = [((2, 45, 8), "db5", 9), ((1, 60, 16), "db7", 0), ((2, 50, 4), "db8", 17), ((1, 56, 12), "db9", 19), ((1, 62, 16), "db10", 41), ((3, 40, 4), "db6", 13)]


@pytest.mark.slow
@pytest.mark.parametrize("shape,wn,chunk", MARCH, ids=[f"march-{m[1]}" for m in MARCH])
def test_axis_march(emu, shape, wn, chunk):
    """AxisMarch at 10 .. 20 taps in both directions, float and double, the march in chunks"""
    outer, n, inner = shape
    L = len(orc.wave_filters(wn)[0])
    for dtype, u in ((np.float32, U32), (np.float64, bc.U["double"])):
        fn = emu.ndwt_emu_march_f32 if dtype == np.float32 else emu.ndwt_emu_march_f64
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_longlong] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

        def dec(x, f):
            _, tl, th = ktaps([f], 1, False, rows=1)
            xin, lo, hi = np.ascontiguousarray(x, dtype=dtype), np.full(shape, np.nan, dtype=dtype), np.full(shape, np.nan, dtype=dtype)
            assert fn(0, L, P(xin), None, P(lo), P(hi), inner, n, outer, chunk, 1, P(tl), P(th)) == 0
            return lo, hi

        def rec(a, d, f):
            _, tl, th = ktaps([f], 1, True, rows=1)
            ai, di, r = np.ascontiguousarray(a, dtype=dtype), np.ascontiguousarray(d, dtype=dtype), np.full(shape, np.nan, dtype=dtype)
            assert fn(1, L, P(ai), P(di), P(r), None, inner, n, outer, chunk, 1, P(tl), P(th)) == 0
            return r
        # the reference of the double run is the float64 oracle itself: two double computations, each within its own share of the bound
        _axis_hold(f"march-{L} {np.dtype(dtype).name}", dec, rec, shape, wn, list(range(chunk, n, chunk)) if chunk else [], u=u)


AXISX = [((2, 300), "db5", False, True), ((2, 301), "db5", False, False), ((2, 150), "db5", True, True), ((1, 131), "db5", True, False),
         ((2, 300), "db6", False, True), ((1, 277), "db6", True, False)]


@pytest.mark.slow
@pytest.mark.parametrize("shape,wn,cplx,vec4", AXISX, ids=[f"axisx-{a[1]}-{'c' if a[2] else 'r'}-{'v4' if a[3] else 'rg'}" for a in AXISX])
def test_axisx(emu, shape, wn, cplx, vec4):
    """AxisX at 10 and 12 taps, EW = 1 and 2, rows of whole groups of 4 scalars or not: two wave segments per row"""
    outer, n = shape
    L, ew = len(orc.wave_filters(wn)[0]), 2 if cplx else 1
    fn = emu.ndwt_emu_axisx_f32
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 4 + [ctypes.c_longlong] * 2 + [ctypes.c_void_p] * 2
    cdt = np.complex64 if cplx else np.float32

    def dec(x, f):
        _, tl, th = ktaps([f], 1, False, rows=1)
        xin, lo, hi = np.ascontiguousarray(x, dtype=cdt), np.full(shape, np.nan, dtype=cdt), np.full(shape, np.nan, dtype=cdt)
        assert fn(0, L, ew, int(vec4), P(xin), None, P(lo), P(hi), n * ew, outer, P(tl), P(th)) == 0
        return lo, hi

    def rec(a, d, f):
        _, tl, th = ktaps([f], 1, True, rows=1)
        ai, di, r = np.ascontiguousarray(a, dtype=cdt), np.ascontiguousarray(d, dtype=cdt), np.full(shape, np.nan, dtype=cdt)
        assert fn(1, L, ew, int(vec4), P(ai), P(di), P(r), None, n * ew, outer, P(tl), P(th)) == 0
        return r
    _axis_hold(f"axisx-{L} ew={ew} vec4={vec4}", dec, rec, shape, wn, E(n, _wx(False, L, ew)), cplx=cplx)


# ---- the cascaded 1-D families, emulated in libraries of their own (built as their test modules build them): 8 taps, float
def _side_lib(module, name, fn, argtypes):
    mod = __import__(module)
    lib = ctypes.CDLL(mod._build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(mod.EMU, name)))
    getattr(lib, fn).restype = ctypes.c_int
    getattr(lib, fn).argtypes = argtypes
    return lib


def _columns(comb, ncol):
    """[n(, bands), ncol]: the comb in every column, scaled by another exact amplitude"""
    return np.stack([comb * abs(bc.amplitude(k)) for k in range(ncol)], axis=-1)


def _hold_1d(name, call, direction, n, ncol, wn, nlev, l2, edges, cap=None):
    """call(array [n, ncol(, bands)], filter pair) -> [n, ncol(, bands)]: `nlev` levels of the 1-D transform of every column"""
    filt = bc.filters(wn, 1)
    L = len(filt[0][0])
    c = cap or nlev * (L + 2)
    pos, reach = [bc.axis_positions(n, edges)], [nlev * L]
    ins = [(None, x) for x in bc.combs([n], pos, reach, pairs=True)] if direction == "dec" else bc.rec_combs([n], pos, reach, nlev, pairs=True)
    bad = bc.mutate(filt, 1e-4)
    worst, caught = 0.0, False
    for m, (band, v) in enumerate(ins):
        cols = [v * abs(bc.amplitude(k)) for k in range(ncol)]
        one = (lambda a, f: bc.walk_dec(a, f, nlev, l2)) if direction == "dec" else (lambda a, f: bc.walk_rec(a, f, l2, level=nlev))
        want = np.stack([one(a, filt) for a in cols], axis=1)
        cond = np.stack([one(np.abs(a), bc.abs_filters(filt)) for a in cols], axis=1)
        arr = np.stack(cols, axis=1)
        worst = max(worst, bc.check_componentwise(call(arr, filt[0]), want, cond, c, U32, f"{name} comb {m} band {band}"))
        if not caught and band in (None, 0):
            try:
                bc.check_componentwise(call(arr, bad[0]), want, cond, c, U32)
            except AssertionError:
                caught = True
    print(f"[emu-small-taps] {name}: worst {worst:.3g} u cond (cap {c}); the 1e-4 mutant {'fails' if caught else 'PASSES'} the check")
    assert caught, name
    return worst


def _wx1(syn, L, nlev):
    LH, RH = (L // 2, L // 2 - 1) if syn else (L // 2 - 1, L // 2)
    return 4 * ((64 - nlev * ((LH + 3) // 4 + (RH + 3) // 4)) // 8 * 8)


@pytest.mark.slow
def test_cascade1(emu):
    """Fwd1C / Inv1C, 8 taps, three levels, three signals of two wave segments: the comb straddles the segment edge"""
    lib = _side_lib("test_emulated_cascade1", "libndwt_emu_cascade1.so", "ndwt_emu1_cascade",
                    [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [ctypes.c_longlong] * 2 + [ctypes.c_void_p] * 2)
    K, nlev = 3, 3
    for inverse in (False, True):
        n = _wx1(inverse, 8, nlev) + 32

        def call(a, f):
            _, lo, hi = ktaps([f], 1, inverse, rows=1)
            src = np.ascontiguousarray(to_kernel_order(a).astype(np.float32))
            out = np.full((K, n) if inverse else (1 + nlev, K, n), np.nan, dtype=np.float32)
            assert lib.ndwt_emu1_cascade(int(inverse), 0, 1, 8, nlev, src.ctypes.data, out.ctypes.data, n, K, lo.ctypes.data, hi.ctypes.data) == 0
            return np.transpose(out)
        _hold_1d(f"{'inv1c' if inverse else 'fwd1c'}-8-3", call, "rec" if inverse else "dec", n, K, "db4", nlev, 1, [_wx1(inverse, 8, nlev)])


@pytest.mark.slow
def test_marchc(emu):
    """FwdMC / InvMC, 8 taps, three levels of a strided axis in one march: samples of 4 floats, two items, the march in chunks"""
    lib = _side_lib("test_emulated_marchc", "libndwt_emu_marchc.so", "ndwt_emu_marchc",
                    [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_longlong] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2)
    K, inner, n, nlev, chunk = 2, 4, 60, 3, 23
    for inverse in (False, True):
        def call(a, f):                                          # a: [n, K * inner(, bands)] -> the emulator's [(bands,) K, n, inner]
            _, lo, hi = ktaps([f], 0, inverse, rows=1)
            a4 = a.reshape((n, K, inner) + a.shape[2:])
            src = np.ascontiguousarray((np.moveaxis(a4, -1, 0).transpose(0, 2, 1, 3) if inverse else a4.transpose(1, 0, 2)).astype(np.float32))
            out = np.full((K, n, inner) if inverse else (1 + nlev, K, n, inner), np.nan, dtype=np.float32)
            assert lib.ndwt_emu_marchc(int(inverse), 0, 8, nlev, src.ctypes.data, out.ctypes.data, inner, n, K, chunk, lo.ctypes.data, hi.ctypes.data) == 0
            if inverse:
                return out.transpose(1, 0, 2).reshape(n, K * inner)
            return np.moveaxis(out.transpose(0, 2, 1, 3).reshape(1 + nlev, n, K * inner), 0, -1)
        _hold_1d(f"{'invmc' if inverse else 'fwdmc'}-8-3", call, "rec" if inverse else "dec", n, K * inner, "db4", nlev, 0, [chunk, 2 * chunk])


@pytest.mark.slow
def test_den1c_with_thresholds_zero(emu):
    """Den1C at thresholds 0: dec then rec of every signal in one launch is the identity.  want = x, cond = |W^-1| |W| |x|; the cap adds the
    analysis (L + 2 a level) to a synthesis whose bands are all non-zero: low-pass and high-pass products, 2 L + 2 a level"""
    lib = _side_lib("test_emulated_den1c", "libndwt_emu_den1c.so", "ndwt_emu1_denoise",
                    [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_longlong] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int])
    K, nlev, L = 3, 2, 8
    wd = 4 * ((64 - nlev * 4) // 8 * 8)
    n = wd + 32
    filt = bc.filters("db4", 1)
    cap = nlev * (L + 2) + nlev * (2 * L + 2)
    worst, caught = 0.0, False
    for m, x in enumerate(bc.combs([n], [bc.axis_positions(n, [wd])], [2 * nlev * L], pairs=True)):
        cols = [x * abs(bc.amplitude(k)) for k in range(K)]
        arr = np.stack(cols, axis=1)
        cond = np.stack([bc.abs_rec(bc.abs_dec(a, filt, nlev, 1), filt, 1, level=nlev) for a in cols], axis=1)

        def call(f):
            taps = np.zeros((4, 20))
            taps[0], taps[1] = [t[0] for t in ktaps([f], 1, False, rows=1)[1:]]
            taps[2], taps[3] = [t[0] for t in ktaps([f], 1, True, rows=1)[1:]]
            src = np.ascontiguousarray(to_kernel_order(arr).astype(np.float32))
            out = np.full(src.shape, np.nan, dtype=np.float32)
            thr = np.zeros(8)
            assert lib.ndwt_emu1_denoise(0, 1, L, nlev, src.ctypes.data, out.ctypes.data, n, K, taps.ctypes.data, thr.ctypes.data, 0) == 0
            return np.transpose(out)
        worst = max(worst, bc.check_componentwise(call(filt[0]), arr, cond, cap, U32, f"den1c comb {m}"))
        if not caught:
            try:
                bc.check_componentwise(call(bc.mutate(filt, 1e-4)[0]), arr, cond, cap, U32)
            except AssertionError:
                caught = True
    print(f"[emu-small-taps] den1c-8-2 thresholds 0: worst {worst:.3g} u cond (cap {cap}); the 1e-4 mutant {'fails' if caught else 'PASSES'} the check")
    assert caught


@pytest.mark.slow
def test_cascade2_kinds(emu):
    """Fwd2C / Inv2C on (re, im) pairs (complex64), 8 taps, two levels: two waves along x, rows in chunks"""
    lib = _side_lib("test_emulated_cascade2_kinds", "libndwt_emu_cascade2_kinds.so", "ndwt_emu2_cascade_kinds",
                    [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_double, ctypes.c_int])
    nlev, shape, yc = 2, (122, 30), 13
    for inverse in (False, True):
        LH, RH = (4, 3) if inverse else (3, 4)
        wx = 4 * ((64 - nlev * ((LH * 2 + 3) // 4 + (RH * 2 + 3) // 4)) // 8 * 8) // 2         # elements of a row one wave stores

        def call(v, f):
            Lp, lo, hi = ktaps(f, 1, inverse)
            src = np.ascontiguousarray(to_kernel_order(v).astype(np.complex64))
            n2, n1 = src.shape[-2:]
            out = np.full((n2, n1) if inverse else (1 + 3 * nlev, n2, n1), np.nan, dtype=np.complex64)
            assert lib.ndwt_emu2_cascade_kinds(int(inverse), 0, 2, Lp, nlev, 1, src.ctypes.data, out.ctypes.data, 2 * n1, n2, yc, lo.ctypes.data, hi.ctypes.data,
                                               0.0, 0) == 0
            return np.transpose(out)
        hold(f"{'inv2c' if inverse else 'fwd2c'}-c64-8-2", call, "rec" if inverse else "dec", shape, ("db4", "db3"), 1, [E(122, wx), [13, 26]], cplx=True,
             levels=nlev, mutate_axis=0)


@pytest.mark.slow
def test_stack2(emu):
    """the cascade on a stack of images (the items in the batch slot of the launch), float, 8 taps, three levels: the comb in one item, another
    comb in the other, each item slot checked in turn"""
    lib = _side_lib("test_emulated_stack2", "libndwt_emu_stack2.so", "ndwt_emu2_stack",
                    [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2)
    nlev, yc = 3, 21                                             # (the emulator holds the 8-tap stack instances at three levels)
    for inverse in (False, True):
        wx = _wx1(inverse, 8, nlev)
        shape = (wx + 32, 40)
        for slot in (0, 1):
            def call(v, f):
                Lp, lo, hi = ktaps(f, 1, inverse)
                other = np.roll(v, 5, axis=0) * 0.75
                stack = np.stack([v, other] if slot == 0 else [other, v], axis=2)           # [n1, n2, items(, bands)]
                src = np.ascontiguousarray(to_kernel_order(stack).astype(np.float32))
                out = np.full(((2, shape[1]) if inverse else (1 + 3 * nlev, 2, shape[1])) + (shape[0],), np.nan, dtype=np.float32)
                assert lib.ndwt_emu2_stack(int(inverse), 0, 1, Lp, nlev, src.ctypes.data, out.ctypes.data, shape[0], shape[1], 2, yc, lo.ctypes.data,
                                           hi.ctypes.data) == 0
                got = np.transpose(out)
                assert np.isfinite(got).all()
                return got[:, :, slot]
            hold(f"stack2-{'inv2c' if inverse else 'fwd2c'}-8-3 item {slot}", call, "rec" if inverse else "dec", shape, "db4", 1, [E(shape[0], wx), [21]],
                 levels=nlev, mutate_axis=slot)


@pytest.mark.slow
def test_den1r_with_thresholds_zero(emu):
    """Den1C with a threshold row per signal (ROWTHR), float, 8 taps, four levels, all thresholds 0: the identity, as test_den1c above"""
    lib = _side_lib("test_emulated_den1r", "libndwt_emu_den1r.so", "ndwt_emu1r_denoise",
                    [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int])
    K, nlev, L = 3, 4, 8
    wd = 4 * ((64 - nlev * 4) // 8 * 8)
    n = wd + 32
    filt = bc.filters("db4", 1)
    cap = nlev * (L + 2) + nlev * (2 * L + 2)
    worst, caught = 0.0, False
    for m, x in enumerate(bc.combs([n], [bc.axis_positions(n, [wd])], [2 * nlev * L], pairs=True)):
        cols = [x * abs(bc.amplitude(k)) for k in range(K)]
        arr = np.stack(cols, axis=1)
        cond = np.stack([bc.abs_rec(bc.abs_dec(a, filt, nlev, 1), filt, 1, level=nlev) for a in cols], axis=1)

        def call(f):
            taps = np.zeros((4, 20))
            taps[0], taps[1] = [t[0] for t in ktaps([f], 1, False, rows=1)[1:]]
            taps[2], taps[3] = [t[0] for t in ktaps([f], 1, True, rows=1)[1:]]
            src = np.ascontiguousarray(to_kernel_order(arr).astype(np.float32))
            out = np.full(src.shape, np.nan, dtype=np.float32)
            thr = np.zeros((K, 1 + nlev))
            assert lib.ndwt_emu1r_denoise(0, src.ctypes.data, out.ctypes.data, n, K, taps.ctypes.data, thr.ctypes.data, 0, 1) >= 0
            return np.transpose(out)
        worst = max(worst, bc.check_componentwise(call(filt[0]), arr, cond, cap, U32, f"den1r comb {m}"))
        if not caught:
            try:
                bc.check_componentwise(call(bc.mutate(filt, 1e-4)[0]), arr, cond, cap, U32)
            except AssertionError:
                caught = True
    print(f"[emu-small-taps] den1r-8-4 thresholds 0: worst {worst:.3g} u cond (cap {cap}); the 1e-4 mutant {'fails' if caught else 'PASSES'} the check")
    assert caught
