"""What the tests of the neighbourhood shrinkage share (tests/test_emulated_neigh.py, tests/test_gpu_neigh.py): the contents of a
coefficient array, the reference in numpy, the shapes and the case file of the stand-alone emulator program.

The definition (include/ndwt.h: ndwt_shrink_neigh), T the scalar type, d = 1, 2 or 3 filtered axes of one item, axis 0 the fastest,
r the radius, every index periodic within the item of the band:
  A = over dx = -r .. r ascending along axis 0, re before im, a = fma(e, e, a) in double from 0
  B = over dy = -r .. r ascending along axis 1, A(.., y + dy), plain double additions, the first term first;  C likewise along axis 2
  S = A, B or C;  t = T(threshold), tt = double(t) * double(t);  S > tt: soft every part times g = T((S - tt) / S) in T, hard the
  coefficient itself; else +0.  threshold == 0: the band is copied bit for bit.
The reference takes np.roll per axis in that order.  What is expected, and why:
  float, complex64    a float squared is exact in double, so the kernels' fma and numpy's multiply-and-add give the same A bit for bit;
                      every later step is one correctly rounded operation in both: BIT-EQUAL on all data.
  double, complex128  numpy rounds the square and the sum, an fma rounds once: the reference is computed with an exact fma too (rational
                      arithmetic, joint_cases._fma) and the kernels are held to THAT one bit for bit; on an integer-valued band every
                      square and sum is an integer below 2^53 and plain numpy is bit-equal as well.
"""
import ctypes
import struct

import numpy as np

from items_cases import build_named_shim
from joint_cases import _fma
from select_cases import KINDS

GUARD_VALUE = 1e30
OUT_FILL = -3e30                      # what the output buffer holds before a call: every scalar outside a band's items must keep it
INT_BAND, NAN_BAND, ZERO_BAND = 0, 1, 2   # integer-valued in every item; one NaN; an all-zero item with one -0


def dims3(dims):
    """(n0, n1, n2) with 1 for the axes a plan does not have"""
    d = [int(v) for v in dims]
    return tuple(d + [1] * (3 - len(d)))


def nan_position(dims):
    """the position (x, y, z) of the one NaN of NAN_BAND's last item: off every edge where the axis is long enough, so that its window
    wraps on the short axes only"""
    return tuple(n // 2 for n in dims3(dims))


def neigh_array(kind, items, dims, nb, guard, seed):
    """(flat, lead, pitch): nb bands of items x prod(dims) elements at pitch = items * n + guard scalars, `lead` = guard scalars in front
    of band 0 and `guard` behind every band, all holding 1e30.  Item j of a band is random, scaled by j + 1.  Band INT_BAND is
    integer-valued in [-8, 8]; the last item of band NAN_BAND holds one NaN at nan_position; item min(1, items - 1) of band ZERO_BAND is
    all zeros with one -0, and every band holds one -0 in its item 0."""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    N = int(np.prod(dims))
    n = N * comp
    pitch = items * n + guard
    lead = guard
    flat = np.full(lead + nb * pitch, GUARD_VALUE, dtype=rdt)
    rng = np.random.default_rng(seed)
    n0, n1, _ = dims3(dims)
    for b in range(nb):
        blk = (rng.standard_normal((items, n)) * (np.arange(items)[:, None] + 1.0)).astype(rdt)
        if b == INT_BAND:
            blk = rng.integers(-8, 9, (items, n)).astype(rdt)
        if b == ZERO_BAND:
            blk[min(1, items - 1)] = 0
            blk[min(1, items - 1), n // 3] = -0.0
        if b == NAN_BAND:
            x, y, z = nan_position(dims)
            blk[items - 1, ((z * n1 + y) * n0 + x) * comp] = np.nan
        blk[0, (2 * n) // 3] = -0.0
        flat[lead + b * pitch:lead + b * pitch + items * n] = blk.reshape(-1)
    return flat, lead, pitch


def _fma_vec(e, s):
    """e * e + s with one rounding, elementwise"""
    with np.errstate(invalid="ignore", over="ignore"):
        plain = s + e * e
    differs = np.nonzero(~((e == np.floor(e)) & (np.abs(e) < 2.0 ** 20) & (s == np.floor(s)) & (s < 2.0 ** 52)).reshape(-1))[0]
    ef, sf, pf = e.reshape(-1), s.reshape(-1), plain.reshape(-1)
    for p in differs:                                          # (integers: the plain sum is exact already)
        pf[p] = _fma(ef[p], sf[p])
    return plain


_SUMS = {}


def window_sums(kind, blk, dims, r, fused=False):
    """S of one band: blk is [items, n] scalars (complex interleaved); [items, n2, n1, n0] doubles.  fused: every square added with one
    rounding (what an fma does); only the double kinds can differ"""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    exact = bool(fused) and rdt == np.float64
    key = (kind, exact, tuple(dims), r, blk.shape, blk.tobytes())
    if key in _SUMS:
        return _SUMS[key].copy()
    n0, n1, n2 = dims3(dims)
    a = blk.astype(np.float64).reshape(blk.shape[0], n2, n1, n0, comp)
    A = np.zeros(a.shape[:-1])
    with np.errstate(invalid="ignore", over="ignore"):
        for dx in range(-r, r + 1):
            v = np.roll(a, -dx, axis=3)                        # v[p] = a[p + dx]
            for part in range(comp):
                A = _fma_vec(v[..., part], A) if exact else A + v[..., part] * v[..., part]
        S = A
        for axis in (2, 1)[:len(dims) - 1]:                   # axis 1 of the item, then axis 2
            T = np.roll(S, r, axis=axis)                       # the first term: S[p - r]
            for d in range(-r + 1, r + 1):
                T = T + np.roll(S, -d, axis=axis)
            S = T
    _SUMS[key] = S
    return S.copy()


def band_view(kind, flat, lead, pitch, items, dims, b):
    n = int(np.prod(dims)) * (2 if KINDS[kind][1] else 1)
    return flat[lead + b * pitch:lead + b * pitch + items * n].reshape(items, n)


def reference_neigh(kind, flat, lead, pitch, items, dims, nb, thr, r, hard, fused=False):
    """the whole output buffer after ndwt_shrink_neigh of `flat` into a buffer of the same layout filled with OUT_FILL"""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    out = np.full(flat.shape, OUT_FILL, dtype=rdt)
    for b in range(nb):
        blk = band_view(kind, flat, lead, pitch, items, dims, b)
        dst = band_view(kind, out, lead, pitch, items, dims, b)
        if thr[b] == 0:
            dst[...] = blk
            continue
        S = window_sums(kind, blk, dims, r, fused).reshape(items, -1)
        t = rdt(thr[b])
        tt = float(t) * float(t)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            keep = S > tt
            g = np.ones(S.shape, dtype=rdt) if hard else ((S - tt) / S).astype(rdt)
            res = (blk * np.repeat(g, comp, axis=1)).astype(rdt)
        if hard:
            res = blk.copy()
        res[~np.repeat(keep, comp, axis=1)] = rdt(0)           # an explicit +0, whatever c is
        dst[...] = res
    return out


def median_thresholds(kind, flat, lead, pitch, items, dims, nb, r, zero_bands=(), below=False):
    """one threshold per band with t^2 just above the median of the band's finite window sums (about half of the positions survive), off
    every sum, so that no position sits on its threshold where the last bit of S would decide; 0 for the bands of `zero_bands`.  The
    positions just above it get a gain near 2^-10 from the difference S - t^2, in which the last bits of S show.  below: just BELOW the
    median instead -- for an item that is one window, where every position has (nearly) the same S and would go to zero otherwise"""
    rdt = KINDS[kind][0]
    thr = np.zeros(nb)
    for b in range(nb):
        if b in zero_bands:
            continue
        S = window_sums(kind, band_view(kind, flat, lead, pitch, items, dims, b), dims, r, True)
        fin = S[np.isfinite(S)]
        if fin.size == 0 or np.median(fin) == 0:               # (one item that is all zero, or one window with a NaN: everything goes to +0)
            thr[b] = 1.0
            continue
        t = float(rdt(np.sqrt(float(np.median(fin)) * (1.0 + (-1 if below else 1) * 2.0 ** -10))))
        tt = float(rdt(t)) ** 2
        assert t > 0 and not (np.abs(fin - tt) <= 2.0 ** -40 * tt).any()
        thr[b] = t
    return thr


def first_difference(got, want, lead, pitch):
    bad = np.nonzero(got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(want.size, -1))[0]
    i = int(bad[0])
    where = "the leading guard" if i < lead else f"band {(i - lead) // pitch}, offset {(i - lead) % pitch}"
    return f"{np.unique(bad).size} scalars differ; first at {i} ({where}): got {float(got[i])!r}, want {float(want[i])!r}"


def check_neigh(kind, src, got, lead, pitch, items, dims, nb, thr, r, hard, what=""):
    """the whole buffer `got` (OUT_FILL before the call) after a neighbourhood shrink of `src`: bit for bit the reference with the exact
    fma -- for the float kinds that IS plain numpy -- and on the integer-valued band plain numpy for the double kinds too"""
    rdt, cplx = KINDS[kind]
    assert got.dtype == src.dtype and got.shape == src.shape
    fused = reference_neigh(kind, src, lead, pitch, items, dims, nb, thr, r, hard, fused=True)
    assert got.tobytes() == fused.tobytes(), (what, first_difference(got, fused, lead, pitch))
    if rdt == np.float64 and thr[INT_BAND] != 0:
        plain = reference_neigh(kind, src, lead, pitch, items, dims, nb, thr, r, hard, fused=False)
        a, b = band_view(kind, got, lead, pitch, items, dims, INT_BAND), band_view(kind, plain, lead, pitch, items, dims, INT_BAND)
        assert a.tobytes() == b.tobytes(), (what, "the integer-valued band against plain numpy")


# ---- the host-side decisions of the library (csrc/ndwt_select.h through tests/select/neigh_shim.cpp) ----
BIG = 1 << 30                                                  # target_blocks: the smallest chunk


def neigh_shim(tmp_path_factory):
    lib = build_named_shim(tmp_path_factory, "neigh_shim")
    lib.sel_neigh_geometry.argtypes = [ctypes.c_int] + [ctypes.c_longlong] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                                                                 ctypes.POINTER(ctypes.c_longlong)]
    lib.sel_neigh_geometry.restype = None
    return lib


def geometry(shim, nd, dims, elem_bytes, r, blocks, num_cus, target_blocks):
    d = list(dims) + [1] * (3 - len(dims))
    out = (ctypes.c_longlong * 4)()
    shim.sel_neigh_geometry(nd, d[0], d[1], d[2], elem_bytes, r, blocks, num_cus, target_blocks, out)
    return tuple(int(v) for v in out)


# ---- the shapes (the list of the issue this came with), from the tile of the instance under test ----
def shape_list(nd, r, tx, ty):
    """[(id, dims, items)]: the shapes on which an instance (nd, r) with tile tx (x ty) can go wrong.  The marched axis of `march` is
    3 (2r + 1) + 2 long: with the smallest chunk, 2r + 1 .. 2r + 2 planes, three chunks, every seam and the wrap of the first chunk's
    priming"""
    w = 2 * r + 1
    march = 3 * w + 2
    if nd == 1:
        return [("window", [w], 1), ("tile+1", [tx + 1], 1), ("2tile-1", [2 * tx - 1], 1), ("items", [w + 2], 3)]
    if nd == 2:
        return [("window", [w, w], 1), ("tile+1", [tx + 1, march], 1), ("2tile-1", [2 * tx - 1, w], 1), ("items", [w + 2, w + 1], 3)]
    return [("window", [w, w, w], 1), ("tile+1", [tx + 1, ty + 1, march], 1), ("2tile-1", [2 * tx - 1, 2 * ty - 1, w], 1), ("items", [w + 2, w, w + 1], 3)]


def levels_for(nd):
    """the level of a test: at least 3 bands (INT_BAND, NAN_BAND, ZERO_BAND)"""
    return 2 if nd == 1 else 1


def num_bands(nd, level):
    return (2 ** nd - 1) * level + 1


# ---- the case file of tests/emu/ndwt_emu_neigh_main.cpp ----
def pack_case(kind, nd, r, hard, dims, items, lead, pitch, nb, geom, thr, src, expect):
    """int32 f64, comp, nd, r, hard, nb, ntx, nty, chunk, nchunks; int32 n0, n1, n2; int64 items, lead, pitch; double thr[nb]; then the
    array and the expected output, each lead + nb * pitch scalars"""
    rdt, cplx = KINDS[kind]
    n0, n1, n2 = dims3(dims)
    ntx, nty, chunk, nchunks = geom
    return (struct.pack("<13i3q", int(rdt == np.float64), 2 if cplx else 1, nd, r, int(hard), nb, ntx, nty, chunk, nchunks, n0, n1, n2, items, lead, pitch) +
            np.asarray(thr, dtype="<f8").tobytes() + src.tobytes() + expect.tobytes())
