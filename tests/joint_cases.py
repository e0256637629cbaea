"""What the tests of the joint shrinkage and the group norms share (tests/test_emulated_joint.py, tests/test_gpu_joint.py): the contents of a
coefficient array, the reference in numpy and the checks against it.

The group at position p of band b is the K coefficients y[b][j][p], j = 0 .. K - 1 (include/ndwt.h: ndwt_shrink_joint).  The reference
loops over the items in ascending order in float64 -- s = s + re * re (then + im * im) -- and then applies the operations of the scalar
type T as the header states them: m = sqrt(T(s)), t = T(threshold), m > t: every part times g = 1 (hard) or (m - t) / m, all in T; else +0.

What is expected, and why (K = items, u = 2^-53):

  float, complex64   a float squared is exact in double, so the fma of the kernels and the multiply-and-add of numpy give the same s bit
                     for bit; sqrt, -, / and * are single correctly rounded operations in both.  The outputs are BIT-EQUAL on all data,
                     and so are the magnitudes: max and nnz of the group norms are exact.
  double, complex128 on integer-valued data every square and every partial sum is an integer below 2^53: bit-equal.  On other data numpy
                     rounds the square and the sum (two roundings a term), the kernels' fma once: after K (2 K) terms the two s differ by
                     at most K 2^-52 relative (2K terms of 2^-53 each way, all terms non-negative), m by half of that plus its own
                     rounding, g = 1 - t / m by at most delta(m) / m in absolute terms (t <= m), and the product adds one rounding:
                     |out - ref| <= (K + 4) 2^-52 |c|, the bound of DOUBLE_BOUND below.
                     The reference is ALSO computed with an exact fused multiply-add (sum_squares(.., fused=True): rational arithmetic,
                     one rounding a term); against that one the double kinds are held bit for bit too, and it is the one the group norms'
                     max and nnz are exact against.
  a group with a NaN goes to zeros (m > t is false); a band with threshold 0 and every guard scalar is untouched bit for bit.
  the group norms    nnz and max exact; l1 and l2sq within N 2^-52 relative, N = the positions of a band: the tolerance norms_cases.py
                     derives for a sum of N non-negative doubles in any order (every term equals the reference's bit for bit); on an
                     integer-valued band l2sq is exact.  A band with a NaN: l1, l2sq and max are NaN, nnz counts the NaN group.
"""
from fractions import Fraction

import numpy as np

from norms_cases import L1, L2SQ, MAX, NNZ, norms_array
from select_cases import KINDS


def DOUBLE_BOUND(items):
    return (items + 4) * 2.0 ** -52


def joint_array(kind, items, N, nb, guard, seed, integer_bands=()):
    """(flat array of nb bands at pitch = items * N * comp + guard scalars, pitch): the contents of norms_cases.norms_array -- random items
    scaled by j + 1, with three items or more an all-equal item and an item with one NaN, with five or more an all-zero item with one -0
    and an integer-valued item; the guard scalars hold 1e30 -- and every item of the bands in `integer_bands` integer-valued in [-8, 8]"""
    rdt, cplx = KINDS[kind]
    n = N * (2 if cplx else 1)
    flat, pitch, _ = norms_array(kind, items, N, nb, guard, seed)
    rng = np.random.default_rng(seed + 17)
    for b in integer_bands:
        flat[b * pitch:b * pitch + items * n] = rng.integers(-8, 9, items * n).astype(rdt)
    return flat, pitch


def _fma(a, s):
    """a * a + s with one rounding"""
    if not (np.isfinite(a) and np.isfinite(s)):
        return a * a + s
    fa = Fraction(float(a))
    return float(fa * fa + Fraction(float(s)))


def sum_squares(kind, blk, fused=False):
    """s[p] of one band: blk is [items, n] scalars (complex interleaved); the items in ascending order, re before im, in float64.
    fused: every term added with one rounding (what an fma does); only the double kinds can differ"""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    exact = fused and rdt == np.float64
    key = (kind, exact, blk.shape, blk.tobytes())
    if key not in _SUMS:
        _SUMS[key] = _sum_squares(blk.astype(np.float64), comp, exact)
    return _SUMS[key].copy()


_SUMS = {}


def _sum_squares(a, comp, exact):
    s = np.zeros(a.shape[1] // comp)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(a.shape[0]):
            for part in range(comp):
                v = a[j, part::comp]
                if not exact:
                    s = s + v * v
                    continue
                plain = s + v * v
                differs = np.nonzero(~((v == np.floor(v)) & (np.abs(v) < 2.0 ** 20) & (s == np.floor(s)) & (s < 2.0 ** 52)))[0]
                for p in differs:                              # (integers: the plain sum is exact already)
                    plain[p] = _fma(v[p], s[p])
                s = plain
    return s


def magnitudes(kind, s):
    rdt = KINDS[kind][0]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(s.astype(rdt))


def band_view(kind, flat, pitch, items, N, b):
    n = N * (2 if KINDS[kind][1] else 1)
    return flat[b * pitch:b * pitch + items * n].reshape(items, n)


def reference_shrink(kind, flat, pitch, items, N, nb, thr, hard, fused=False):
    """the whole buffer after ndwt_shrink_joint; thr: nb thresholds, 0 = the band stays"""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    out = flat.copy()
    for b in range(nb):
        if thr[b] == 0:
            continue
        blk = band_view(kind, flat, pitch, items, N, b)
        m = magnitudes(kind, sum_squares(kind, blk, fused))
        t = rdt(thr[b])
        with np.errstate(invalid="ignore", divide="ignore"):
            keep = m > t
            g = np.ones_like(m) if hard else ((m - t) / m).astype(rdt)
            gs = np.repeat(np.where(keep, g, rdt(0)), comp)
            res = (blk * gs[None, :]).astype(rdt)
        res[:, ~np.repeat(keep, comp)] = rdt(0)               # an explicit +0, whatever c is
        band_view(kind, out, pitch, items, N, b)[...] = res
    return out


def reference_norms(kind, flat, pitch, items, N, nb, fused=True):
    """[nb, 4]: the group norms of every band"""
    out = np.zeros((nb, 4))
    for b in range(nb):
        s = sum_squares(kind, band_view(kind, flat, pitch, items, N, b), fused)
        m = magnitudes(kind, s).astype(np.float64)
        with np.errstate(invalid="ignore"):
            out[b] = [m.sum(), s.sum(), np.nan if np.isnan(m).any() else m.max(), float(np.count_nonzero(s != 0))]
    return out


def median_thresholds(kind, flat, pitch, items, N, nb, zero_bands=()):
    """one threshold per band, just above the median of the band's finite group magnitudes (about half of the groups survive); 0 for the
    bands of `zero_bands`"""
    thr = np.zeros(nb)
    for b in range(nb):
        if b in zero_bands:
            continue
        m = magnitudes(kind, sum_squares(kind, band_view(kind, flat, pitch, items, N, b), True)).astype(np.float64)
        thr[b] = float(np.median(m[np.isfinite(m)])) * (1.0 + 2.0 ** -10)   # (off every magnitude: no group sits on its threshold, where the
                                                                            #  last bit of s would decide)
        assert thr[b] > 0
    return thr


def check_shrink(kind, src, got, pitch, items, N, nb, thr, hard, integer_bands=(), what=""):
    """the whole buffer `got` after a joint shrink of `src`, by the table above"""
    rdt, cplx = KINDS[kind]
    assert got.dtype == src.dtype and got.shape == src.shape
    fused = reference_shrink(kind, src, pitch, items, N, nb, thr, hard, fused=True)
    if got.tobytes() != fused.tobytes():
        bad = np.nonzero(got.view(np.uint8).reshape(got.size, -1) != fused.view(np.uint8).reshape(got.size, -1))[0]
        i = int(bad[0])
        raise AssertionError((what, "not bit-equal", f"{np.unique(bad).size} scalars differ; first at {i} (band {i // pitch}, offset {i % pitch})",
                              float(got[i]), float(fused[i]), float(src[i])))
    if rdt != np.float64:
        return
    plain = reference_shrink(kind, src, pitch, items, N, nb, thr, hard, fused=False)
    n = N * (2 if cplx else 1)
    for b in range(nb):
        sl = slice(b * pitch, b * pitch + items * n)
        if b in integer_bands:
            assert got[sl].tobytes() == plain[sl].tobytes(), (what, "integer-valued band", b)
        else:
            with np.errstate(invalid="ignore"):
                c = np.abs(src[sl])
                err = np.abs(got[sl] - plain[sl])
            ok = (err <= DOUBLE_BOUND(items) * c) | (got[sl].view(np.uint64) == plain[sl].view(np.uint64))   # (a NaN: its group is zeros in both, or untouched)
            assert ok.all(), (what, "band", b, float(np.nanmax(err / np.where(c > 0, c, 1))), DOUBLE_BOUND(items))


def check_group_norms(kind, src, got, pitch, items, N, nb, integer_bands=(), what=""):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (nb, 4), (what, got.shape)
    ref = reference_norms(kind, src, pitch, items, N, nb, fused=True)
    tol = N * 2.0 ** -52
    for b in range(nb):
        w = f"{what} band {b}"
        assert got[b, NNZ] == ref[b, NNZ], (w, "nnz", got[b, NNZ], ref[b, NNZ])
        if np.isnan(ref[b, MAX]):
            assert np.isnan(got[b, [L1, L2SQ, MAX]]).all(), (w, "a NaN in the band", got[b])
            continue
        assert got[b, MAX] == ref[b, MAX], (w, "max", got[b, MAX], ref[b, MAX])
        assert abs(got[b, L1] - ref[b, L1]) <= tol * ref[b, L1], (w, "l1", got[b, L1], ref[b, L1])
        if b in integer_bands:
            assert got[b, L2SQ] == ref[b, L2SQ], (w, "l2sq of integers", got[b, L2SQ], ref[b, L2SQ])
        else:
            assert abs(got[b, L2SQ] - ref[b, L2SQ]) <= tol * ref[b, L2SQ], (w, "l2sq", got[b, L2SQ], ref[b, L2SQ])
