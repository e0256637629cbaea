"""What the tests of the band norms share (tests/test_emulated_norms.py, tests/test_gpu_norms.py): the contents of a coefficient array,
the reference of one (band, item) block in numpy and the check of the four values against it.

The reference is numpy in float64 / complex128 on the same block.  The tolerances are derived, not tuned; n = the scalars of the block,
u_T = 2^-24 for float data and 2^-53 for double:

  nnz, max (real)                    exact
  l1, l2sq of integer-valued real    exact: every partial sum is an integer below 2^53, so the order cannot matter
  l2sq of integer-valued complex     exact, for the same reason
  l1, l2sq otherwise (real), l2sq    relative error <= n 2^-52: a sum of n non-negative doubles in any order is within (n - 1) 2^-53 of
  (complex)                          exact, and the same again covers numpy's own sum
  l1 (complex)                       relative error <= 4 u_T + n 2^-52: the three roundings of sqrt(re^2 + im^2) in T add at most 2 u_T per
                                     term, doubled because the compiler may or may not contract the sum of squares
  max (complex)                      equals sqrt(re^2 + im^2) in T of some element bit for bit -- for one of the ways the sum of squares can
                                     be rounded: both products rounded, or either one fused into the sum -- and no element's exceeds it
A block with a NaN: l1, l2sq and max are NaN, nnz counts the NaN.
"""
from fractions import Fraction

import numpy as np

from items_cases import items_band
from select_cases import KINDS

L1, L2SQ, MAX, NNZ = 0, 1, 2, 3


def norms_array(kind, items, N, nb, guard, seed):
    """(flat array of nb bands at pitch = items * N * comp + guard scalars, pitch, set of (band, item) blocks that are integer-valued).
    Band b holds the items of items_cases.items_band (item j scaled by j + 1; with three items or more item 1 all-equal, item 2 with one
    NaN); with five items item 3 is all zeros with one -0 and item 4 integer-valued in [-8, 8]; with two items item 1 of band 1, with one
    item band 2 is integer-valued.  The guard scalars between and behind the bands hold 1e30 (a kernel that read them would show it)."""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    n = N * comp
    pitch = items * n + guard
    flat = np.full(nb * pitch, 1e30, dtype=rdt)
    integer = set()
    rng = np.random.default_rng(seed)
    for b in range(nb):
        blk = items_band(kind, items, N, seed + 101 * b)
        ints = []
        if items >= 5:
            blk[3] = 0
            blk[3, n // 3] = -0.0
            ints = [4]
        elif items == 2 and b == 1:
            ints = [1]
        elif items == 1 and b == 2:
            ints = [0]
        for j in ints:
            blk[j] = rng.integers(-8, 9, n).astype(rdt)
            integer.add((b, j))
        flat[b * pitch:b * pitch + items * n] = blk.reshape(-1)
    return flat, pitch, integer


def reference(kind, block):
    """(l1, l2sq, max, nnz) of one block (a 1-D array of scalars, complex interleaved) in float64 / complex128"""
    cplx = KINDS[kind][1]
    a = block.astype(np.float64)
    if not cplx:
        m = np.abs(a)
        return m.sum(), (a * a).sum(), m.max(), float(np.count_nonzero(a))
    re, im = a[0::2], a[1::2]
    m = np.abs(re + 1j * im)
    return m.sum(), (re * re + im * im).sum(), m.max(), float(np.count_nonzero((re != 0) | (im != 0)))


def _rounded(frac, rdt):
    """the value of type rdt nearest to the exact `frac`"""
    best = rdt(float(frac))
    for c in (np.nextafter(best, rdt(-np.inf)), np.nextafter(best, rdt(np.inf))):
        if abs(Fraction(float(c)) - frac) < abs(Fraction(float(best)) - frac):
            best = c
    return best


def magnitude_candidates(re, im, rdt):
    """sqrt(re^2 + im^2) in rdt for every way the compiler may round the sum of squares: both products rounded, or one of them fused"""
    R, I = Fraction(float(re)), Fraction(float(im))
    rr, ii = Fraction(float(_rounded(R * R, rdt))), Fraction(float(_rounded(I * I, rdt)))
    return {float(np.sqrt(_rounded(s, rdt))) for s in (rr + ii, R * R + ii, rr + I * I)}


def check_block(kind, block, got, what="", integer=False):
    """the four values `got` of one block against numpy, by the table above"""
    rdt, cplx = KINDS[kind]
    u = 2.0 ** -24 if rdt == np.float32 else 2.0 ** -53
    n = block.size
    got = [float(g) for g in got]
    with np.errstate(invalid="ignore"):
        l1, l2, mx, nnz = reference(kind, block)
    assert got[NNZ] == nnz, (what, "nnz", got[NNZ], nnz)
    if np.isnan(block).any():
        assert np.isnan(got[L1]) and np.isnan(got[L2SQ]) and np.isnan(got[MAX]), (what, "a NaN in the block", got)
        return
    tol = n * 2.0 ** -52
    if integer:
        assert got[L2SQ] == l2, (what, "l2sq of integers", got[L2SQ], l2)
    else:
        assert abs(got[L2SQ] - l2) <= tol * l2, (what, "l2sq", got[L2SQ], l2)
    if not cplx:
        assert got[MAX] == mx, (what, "max", got[MAX], mx)
        if integer:
            assert got[L1] == l1, (what, "l1 of integers", got[L1], l1)
        else:
            assert abs(got[L1] - l1) <= tol * l1, (what, "l1", got[L1], l1)
        return
    assert abs(got[L1] - l1) <= (4 * u + tol) * l1, (what, "l1", got[L1], l1)
    a = block.astype(np.float64)
    m = np.abs(a[0::2] + 1j * a[1::2])
    top = np.nonzero(m >= got[MAX] * (1 - 8 * u))[0]              # every other element is below whatever way it is rounded
    assert top.size and m.max() <= got[MAX] * (1 + 8 * u), (what, "max", got[MAX], m.max())
    cands = [magnitude_candidates(block[2 * e], block[2 * e + 1], rdt) for e in top[:64]]
    assert any(got[MAX] in c for c in cands), (what, "max is no element's magnitude", got[MAX], cands[:3])
    assert all(min(c) <= got[MAX] for c in cands), (what, "an element's magnitude exceeds max", got[MAX])


def check_array(kind, flat, pitch, items, N, nb, got, integer=(), what=""):
    """got[items, nb, 4] against every (band, item) block of the array"""
    comp = 2 if KINDS[kind][1] else 1
    n = N * comp
    got = np.asarray(got)
    assert got.shape == (items, nb, 4), (what, got.shape)
    for b in range(nb):
        for j in range(items):
            check_block(kind, flat[b * pitch + j * n:b * pitch + (j + 1) * n], got[j, b], f"{what} band {b} item {j}", (b, j) in integer)
