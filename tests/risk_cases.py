"""What the tests of the SURE statistics share (tests/test_emulated_risk.py, tests/test_gpu_risk.py): the candidate rows of a block, the
reference of one (band, item) block in numpy, the check of the three values against it, Stein's estimate and a restatement of the
threshold search.

The arrays are those of tests/norms_cases.py (the all-equal item, the item with a NaN, the all-zero item with one -0, integer-valued
items).  A block's statistics at a candidate t (rounded once to the scalar type), with m the magnitude of an element IN THE SCALAR TYPE:

  count   elements with not (m > t); a NaN counts
  energy  the sum of c^2 (re^2 + im^2) over those elements, in float64 from the widened parts
  invsum  complex data: the sum of 1 / float64(m) over the elements with m > t; real data: 0

The magnitude of complex data is reproduced bit for bit (`magnitude`): the kernels write its two forms out (norms_magnitude of
csrc/ndwt_device_norms.h) -- the element-wise float form rounds both products, sqrt(fl(re re) + fl(im im)); every other form fuses the
first, sqrt(fma(re, re, fl(im im))) -- and the fused multiply-add here is libm's, which is exact.  So the sets are the kernel's sets
even where a candidate EQUALS a magnitude of the data, and the tolerances are derived, not tuned; n = the scalars of the block:

  count                         exact
  energy                        relative error <= n 2^-52: a sum of at most n non-negative doubles in any order is within (n - 1) 2^-53
                                of exact, and the same again covers numpy's own sum (the bound norms_cases.py derives for L2SQ);
                                exact on integer-valued data (every partial sum is an integer below 2^53), and 0 where count is 0
  invsum                        relative error <= n 2^-52 of the sum, for the same reason: the terms 1 / float64(m) are the same doubles
                                on both sides (a correctly rounded division of the same bits)
A block with a NaN: energy is NaN at every candidate, the count includes the NaN, invsum leaves it out.
A row that begins with a negative entry: the block is skipped, all zeros.
"""
import ctypes
import ctypes.util

import numpy as np

from select_cases import KINDS

COUNT, ENERGY, INVSUM = 0, 1, 2

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.argtypes = [ctypes.c_double] * 3
_libm.fma.restype = ctypes.c_double
_libm.fmaf.argtypes = [ctypes.c_float] * 3
_libm.fmaf.restype = ctypes.c_float
_fma = np.frompyfunc(lambda a, b, c: _libm.fma(float(a), float(b), float(c)), 3, 1)
_fmaf = np.frompyfunc(lambda a, b, c: _libm.fmaf(float(a), float(b), float(c)), 3, 1)


def magnitude(kind, block, vec):
    """the magnitude of every element of a block (1-D scalars, complex interleaved) in the scalar type, bit for bit the kernels'.
    vec: whether the 4-scalar form of the kernel ran (it decides the float form, see above)"""
    rdt, cplx = KINDS[kind]
    if not cplx:
        return np.abs(block)
    re, im = block[0::2], block[1::2]
    with np.errstate(invalid="ignore", over="ignore"):
        if rdt == np.float32 and not vec:
            return np.sqrt(re * re + im * im)                    # (float32 arithmetic throughout: every operation rounds once)
        q = im * im
        s = (_fmaf if rdt == np.float32 else _fma)(re.astype(object), re.astype(object), q.astype(object))
        return np.sqrt(np.asarray(s, dtype=np.float64).astype(rdt))


def reference(kind, block, cand_row, vec):
    """[nc, 3]: count, energy and invsum of one block at every candidate of its row"""
    rdt, cplx = KINDS[kind]
    cand_row = np.asarray(cand_row, dtype=np.float64)
    out = np.zeros((cand_row.size, 3))
    if cand_row[0] < 0:
        return out
    m = magnitude(kind, block, vec)
    a = block.astype(np.float64)
    sq = a * a if not cplx else a[0::2] * a[0::2] + a[1::2] * a[1::2]
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = 1.0 / m.astype(np.float64)
        for i, t in enumerate(cand_row.astype(rdt)):
            z = ~(m > t)
            out[i] = [float(z.sum()), sq[z].sum(), inv[~z].sum() if cplx else 0.0]
    return out


def candidate_row(kind, block, nc, vec, seed=0):
    """nc candidates of a block: a value that occurs in the data first (nc >= 3: then +inf and 0; nc = 8: also one below the smallest
    non-zero magnitude, one above the largest, two more values of the data and one between)"""
    m = magnitude(kind, block, vec).astype(np.float64)
    ok = m[np.isfinite(m)]
    e = np.sort(ok)
    occurs = float(e[(2 * e.size) // 3])
    row = [occurs, np.inf, 0.0]
    if nc == 8:
        pos = e[e > 0]
        low = float(pos[0]) * 0.5 if pos.size else 0.0
        row += [low, float(e[-1]) * 2.0 + 1.0, float(e[e.size // 4]), float(e[-1]), 0.5 * (float(e[e.size // 2]) + occurs)]
    assert nc in (1, 3, 8), nc
    return [row[i] for i in np.random.default_rng(seed).permutation(nc)]


def check_block(kind, block, cand_row, got, vec, integer=False, what=""):
    """the [nc, 3] values `got` of one block against numpy, by the table above"""
    rdt, cplx = KINDS[kind]
    want = reference(kind, block, cand_row, vec)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape)
    tol = block.size * 2.0 ** -52
    if cand_row[0] < 0:
        assert not got.any() and not np.signbit(got).any(), (what, "a skipped block", got)
        return
    nan = bool(np.isnan(block).any())
    for i in range(want.shape[0]):
        w = f"{what} candidate {i} ({cand_row[i]!r})"
        assert got[i, COUNT] == want[i, COUNT], (w, "count", got[i, COUNT], want[i, COUNT])
        if nan:
            assert np.isnan(got[i, ENERGY]), (w, "energy with a NaN in the block", got[i, ENERGY])
        elif integer or want[i, COUNT] == 0:
            assert got[i, ENERGY] == want[i, ENERGY], (w, "energy, exact", got[i, ENERGY], want[i, ENERGY])
        else:
            assert abs(got[i, ENERGY] - want[i, ENERGY]) <= tol * want[i, ENERGY], (w, "energy", got[i, ENERGY], want[i, ENERGY])
        if not cplx:
            assert got[i, INVSUM] == 0.0, (w, "invsum of real data", got[i, INVSUM])
        else:
            assert abs(got[i, INVSUM] - want[i, INVSUM]) <= tol * want[i, INVSUM], (w, "invsum", got[i, INVSUM], want[i, INVSUM])


def blocks_of(kind, flat, pitch, items, N, nb):
    """(band, item, the block's scalars) of an array of norms_cases.norms_array"""
    n = N * (2 if KINDS[kind][1] else 1)
    for b in range(nb):
        for j in range(items):
            yield b, j, flat[b * pitch + j * n:b * pitch + (j + 1) * n]


def sure(comp, n, s, cand, stats):
    """Stein's unbiased estimate of the risk of a soft threshold at every candidate: n d s^2 + E + t^2 (n - C) - 2 s^2 (d C + (d - 1) t I)
    (the terms in n - C and I are 0 where nothing lies above t)"""
    t = np.asarray(cand, dtype=np.float64)
    st = np.asarray(stats, dtype=np.float64)
    C, E, I = st[:, COUNT], st[:, ENERGY], st[:, INVSUM]
    d = float(comp)
    with np.errstate(invalid="ignore"):
        above = np.where(n - C == 0.0, 0.0, t * t * (n - C))
        curl = np.where(I == 0.0, 0.0, (d - 1.0) * t * I) if comp == 2 else 0.0
    return n * d * s * s + E + above - 2.0 * s * s * (d * C + curl)


def search(kind, N, n, s, rounds, stats):
    """The search of ndwt_sure_thresholds on ONE block, restated: N the elements of one item's filtered axes, n the elements of the block,
    s the noise of the band, stats(row) -> [8, 3] the statistics of the block at 8 candidates.  (threshold, estimate there)."""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    t_max = s * np.sqrt(2.0 * np.log(float(N)))
    best_t, best_r = 0.0, n * comp * s * s
    if not t_max > 0.0:
        return best_t, best_r
    lo, hi = 0.0, t_max
    for _ in range(rounds):
        row = [float(rdt(lo + (hi - lo) * (i + 1) / 8.0)) for i in range(8)]
        v = sure(comp, n, s, row, stats(row))
        at = 0
        for i in range(1, 8):
            if v[i] < v[at] or (np.isnan(v[at]) and not np.isnan(v[i])):
                at = i
        if v[at] < best_r:
            best_t, best_r = row[at], float(v[at])
        step = (hi - lo) / 8.0
        lo, hi = max(best_t - step, 0.0), min(best_t + step, t_max)
    return best_t, best_r
