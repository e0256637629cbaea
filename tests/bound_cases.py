"""Componentwise error bounds for the transform: the instrument of tests/test_bound_cases.py, tests/test_emulated_small_taps.py and
tests/test_gpu_small_taps.py (CPU side, numpy and the oracle only).

The metric.  The parity tests measure max|got - want| / max|want| over all bands at once, on white noise.  The outer taps of the long
filters are 2e-5 (db10) .. 5e-4 (db7) of the largest tap, so a kernel that drops or misplaces one of them passes at 2e-6 .. 4e-5.  Here every
element is held to the forward error bound of a filter bank in its componentwise form,

    |got_i - want_i| <= c * u * (|W| |x|)_i ,

where |W| |x| (`cond`) is the same level walk run on |x| with the absolute values of the taps (abs_dec / abs_rec), u is the unit roundoff
of the working precision and c counts the roundings on the path of one element.  On a sparse input an element is one product of taps (or
a short sum of such), the bound is as small as the element, and each tap is checked against its own size.

The cap.  c = levels * sum over the filtered axes a of (L_a + 2)  (`cap`), from:
  * one axis pass of one level sums L_a products: L_a roundings of products and L_a - 1 of additions -- in any order, and fewer with fused
    multiply-adds.  The standard bound of such a sum is gamma_n with n = L_a (Higham, Accuracy and Stability of Numerical Algorithms, 3.1):
    every term carries at most L_a factors (1 + delta), whatever the order of the additions;
  * each tap carries two more: its rounding to the working precision and the rounding of folding the scale (1/sqrt 2, or 1/2) into it;
  * the passes of one level follow each other, the levels too, and the factors multiply: to first order in u the counts add.  Storing a
    band between two passes or two levels is the rounding of the last addition, already counted;
  * the final 1 / 2^d of a synthesis without pres_l2_norm is a power of two: exact.
  A synthesis pass adds the low-pass and the high-pass sum of an axis, 2 L_a products; the synthesis inputs of `rec_combs` hold one band
  only, the products with the zeros of every other band are exact and so are the additions of those zeros, which leaves L_a terms again.
  L_a is the axis' own tap length (zero padding to a common length multiplies by exact zeros).  Terms of second order, (c u)^2 / 2, are
  below 1e-10 of the bound in single precision and are left out.  Nothing here is tuned to what a kernel gives.

The check.  `check_componentwise` holds every element to c * u * cond, and wants got == 0 exactly wherever cond == 0: products with zero
inputs are exact, so a non-zero there is a read from a place the filter cannot reach.  No element is left out.

The inputs.  Combs of impulses (`axis_positions`, `combs`, `rec_combs`): exactly representable amplitudes of both signs that are no powers
of two, at the first and the last sample of every filtered axis (every tap crosses the periodic wrap both ways) and on the two samples
either side of the tile, chunk and wave-row edges of the kernel under test; positions closer than the reach of the filters go into
combs of their own, since overlapping supports only dull the test.
"""
import numpy as np

import ndwt_oracle as orc

U = {"single": 2.0 ** -24, "double": 2.0 ** -53, np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}


# ---- the level walk of ndwt_oracle.spatial_dec / spatial_rec with the filter pairs as an argument (true taps, their absolute values, mutants)
def filters(wn, d=None):
    """[(lo, hi)] per axis of a wavelet name or a list of names"""
    wl = [wn] * d if isinstance(wn, str) else list(wn)
    return [orc.wave_filters(w) for w in wl]


def walk_dec(x, filt, level, pres_l2_norm=0, dilation="reference", level_fn=None):
    level_fn = level_fn or orc.spatial_level_dec
    y = None
    for lev in range(1, level + 1):
        stride = 1 if dilation == "reference" else 1 << (lev - 1)
        if lev == 1:
            y = level_fn(x, filt, pres_l2_norm, stride)
        else:
            y = np.concatenate([level_fn(y[..., 0], filt, pres_l2_norm, stride), y[..., 1:]], axis=-1)
    return y


def walk_rec(c, filt, pres_l2_norm=0, dilation="reference", level=None, level_fn=None):
    level_fn = level_fn or orc.spatial_level_rec
    d = c.ndim - 1
    nb = 1 << d
    level = level or orc.level_from_bands(d, c.shape[-1])
    y = None
    for ind in range(1, level + 1):
        lev = level - ind + 1
        stride = 1 if dilation == "reference" else 1 << (lev - 1)
        if ind == 1:
            blk = c[..., :nb]
        else:
            lo = nb + (ind - 2) * (nb - 1)
            blk = np.concatenate([y[..., None], c[..., lo:lo + nb - 1]], axis=-1)
        y = level_fn(blk, filt, pres_l2_norm, stride)
    return y


def magnitude(x):
    """the input magnitude of the bound: |x|, complex data |re| + |im| (real and imaginary part are filtered on their own)"""
    x = np.asarray(x)
    return np.abs(x.real) + np.abs(x.imag) if np.iscomplexobj(x) else np.abs(x).astype(np.float64)


def abs_filters(filt):
    return [(np.abs(lo), np.abs(hi)) for lo, hi in filt]


def abs_dec(x, filt, level, pres_l2_norm=0, dilation="reference"):
    """|W| |x| of `level` levels of analysis: spatial_dec's level walk on |x| with |taps|"""
    return walk_dec(magnitude(x), abs_filters(filt), level, pres_l2_norm, dilation)


def abs_rec(c, filt, pres_l2_norm=0, dilation="reference", level=None):
    return walk_rec(magnitude(c), abs_filters(filt), pres_l2_norm, dilation, level)


def cap(filt, level, axes=None):
    """c = levels * sum over the filtered axes of (L_a + 2): the module docstring has the derivation"""
    axes = range(len(filt)) if axes is None else axes
    return level * sum(len(filt[a][0]) + 2 for a in axes)


def check_componentwise(got, want, cond, c, u, what=""):
    """|got - want| <= c u cond at EVERY element, got == 0 exactly where cond == 0; returns the worst |got - want| / (u cond)"""
    got, want, cond = np.asarray(got), np.asarray(want), np.asarray(cond, dtype=np.float64)
    assert got.shape == want.shape == cond.shape, (what, got.shape, want.shape, cond.shape)
    assert np.isfinite(got).all(), f"{what}: {np.count_nonzero(~np.isfinite(got))} non-finite values"
    zero = cond == 0
    if zero.any():
        bad = zero & (got != 0)
        assert not bad.any(), (f"{what}: {np.count_nonzero(bad)} non-zero values where no tap reaches, first at {tuple(np.argwhere(bad)[0])}: "
                               f"{got[tuple(np.argwhere(bad)[0])]!r}")
    diff = got.astype(np.complex128 if np.iscomplexobj(got) else np.float64) - want
    # complex data: real and imaginary part are filtered on their own and each holds the bound (cond is that of |re| + |im|, the larger)
    err = np.maximum(np.abs(diff.real), np.abs(diff.imag)) if np.iscomplexobj(diff) else np.abs(diff)
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, u * cond))
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > c:
        i = tuple(np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        raise AssertionError(f"{what}: |got - want| = {err[i]:.3e} at {i} is {worst:.4g} u cond, the cap is {c} (got {got[i]!r}, want {want[i]!r}, "
                             f"cond {cond[i]:.3e}; {np.count_nonzero(ratio > c)} of {ratio.size} elements over)")
    return worst


def relerr(got, want):
    """the metric of tests/test_gpu_parity.py, for the record"""
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


# ---- mutants and the plain single-precision restatement
def smallest_tap(taps):
    nz = np.flatnonzero(taps)
    return int(nz[np.argmin(np.abs(taps[nz]))])


def mutate(filt, rel=1e-4, axes=None, which=("lo", "hi")):
    """the filter pairs with the smallest low-pass and the smallest high-pass tap of `axes` (default: every axis) changed by `rel` of itself"""
    out = []
    for a, (lo, hi) in enumerate(filt):
        lo, hi = lo.copy(), hi.copy()
        if axes is None or a in axes:
            if "lo" in which:
                lo[smallest_tap(lo)] *= 1 + rel
            if "hi" in which:
                hi[smallest_tap(hi)] *= 1 + rel
        out.append((lo, hi))
    return out


def _f32_axis_dec(x, lo_d, hi_d, axis, s, stride):
    s32 = np.float32(s)
    lo = np.zeros_like(x)
    hi = np.zeros_like(x)
    for m in range(len(lo_d)):                                   # sequential sums, every operation rounded to float32
        xs = np.roll(x, (m - len(lo_d) // 2) * stride, axis=axis)
        lo = lo + (s32 * np.float32(lo_d[m])) * xs
        hi = hi + (s32 * np.float32(hi_d[m])) * xs
    return lo, hi


def f32_level_dec(x, filt, pres_l2_norm, stride=1):
    """spatial_level_dec in plain float32: taps rounded to float32, then the scale folded in (a second rounding), sequential sums"""
    x = np.asarray(x, dtype=np.complex64 if np.iscomplexobj(x) else np.float32)
    s = 1 / np.sqrt(2.0) if pres_l2_norm else 1.0
    bands = [x]
    for a in range(x.ndim):
        lo_hi = [_f32_axis_dec(b, filt[a][0], filt[a][1], a, s, stride) for b in bands]
        bands = [p[0] for p in lo_hi] + [p[1] for p in lo_hi]
    return np.stack(bands, axis=-1)


def f32_level_rec(c, filt, pres_l2_norm, stride=1):
    c = np.asarray(c, dtype=np.complex64 if np.iscomplexobj(c) else np.float32)
    d = c.ndim - 1
    s32 = np.float32(1 / np.sqrt(2.0) if pres_l2_norm else 0.5)  # the 1 / 2^d of the reference, folded in per axis: exact
    bands = [c[..., b] for b in range(1 << d)]
    for a in range(d - 1, -1, -1):
        half = len(bands) // 2
        lo_d, hi_d = filt[a]
        nxt = []
        for i in range(half):
            r = np.zeros_like(bands[i])
            for m in range(len(lo_d)):
                sh = -(m - len(lo_d) // 2) * stride
                r = r + (s32 * np.float32(lo_d[m])) * np.roll(bands[i], sh, axis=a)
                r = r + (s32 * np.float32(hi_d[m])) * np.roll(bands[i + half], sh, axis=a)
            nxt.append(r)
        bands = nxt
    return bands[0]


def f32_dec(x, filt, level, pres_l2_norm=0, dilation="reference"):
    return walk_dec(x, filt, level, pres_l2_norm, dilation, level_fn=f32_level_dec)


def f32_rec(c, filt, pres_l2_norm=0, dilation="reference", level=None):
    return walk_rec(c, filt, pres_l2_norm, dilation, level, level_fn=f32_level_rec)


# ---- the comb inputs
def amplitude(k):
    """exactly representable in float32, both signs, no power of two: +-(2 j + 3) / 8 for j = k mod 13"""
    return (-1.0 if k % 2 else 1.0) * (2 * (k * 7 % 13) + 3) / 8.0


def axis_positions(n, edges=()):
    """first and last sample of an axis of n, and the two samples either side of every interior edge e (a tile, chunk or wave-row start)"""
    pos = {0, n - 1}
    for e in edges:
        if 0 < e < n:
            pos.update((e - 1, e))
    return sorted(pos)


def tile_edges(n, tile, anchor_last=False):
    """starts of the tiles of `tile` samples that cover an axis of n; anchor_last: the last tile ends on the last sample (the fused 3-D
    kernels anchor a ragged last tile at the row end), which puts one more edge at n - tile"""
    e = list(range(tile, n, tile)) if tile > 0 else []
    if anchor_last and tile > 0 and n > tile and n % tile:
        e.append(n - tile)
    return sorted(set(e))


def _sites(pos, n, pairs):
    """the positions of one axis as sites: every position on its own, or (pairs) the runs of cyclically adjacent positions -- the first and
    the last sample, the two samples either side of an edge -- as one site each"""
    if not pairs:
        return [[p] for p in pos]
    sites = []
    for p in sorted(pos):
        if sites and p - sites[-1][-1] == 1:
            sites[-1].append(p)
        else:
            sites.append([p])
    if len(sites) > 1 and sites[0][0] == 0 and sites[-1][-1] == n - 1:
        sites[0] = sites.pop() + sites[0]                        # the wrap: .., n - 1, 0, ..
    return sites


def _classes(pos, n, reach, pairs=False):
    """split the sites of one axis into the fewest classes in which any two are `reach` or more apart, cyclically (greedy, in order)"""
    classes = []
    for site in _sites(pos, n, pairs):
        for cl in classes:
            if all(min((p - q) % n, (q - p) % n) >= reach for p in site for q in cl):
                cl.extend(site)
                break
        else:
            classes.append(list(site))
    return classes


def combs(shape, positions, reach, cplx=False, pairs=False):
    """Comb inputs of `shape`: comb m is the lattice of the m-th class of positions of every axis (an axis with fewer classes cycles), so
    that in one comb no two supports overlap wherever the axes allow it.  positions[a]: sample indices on axis a; reach[a]: how far the
    filters of all levels carry an impulse on axis a.  pairs: the two samples either side of an edge share a comb (and overlap: each keeps
    the far end of its support to itself, where the smallest low-pass tap of the one and the smallest high-pass tap of the other land) --
    half the inputs for a large array; without, every position of a short axis gets a comb of its own"""
    d = len(shape)
    cls = [_classes(positions[a], shape[a], reach[a], pairs) for a in range(d)]
    n = max(len(c) for c in cls)
    out = []
    for m in range(n):
        x = np.zeros(shape, dtype=np.complex128 if cplx else np.float64)
        sel = [cls[a][m % len(cls[a])] for a in range(d)]
        k = 3 * m
        for idx in np.ndindex(*[len(s) for s in sel]):
            p = tuple(sel[a][i] for a, i in enumerate(idx))
            x[p] = amplitude(k) + (1j * amplitude(k + 5) if cplx else 0)
            k += 1
        out.append(x)
    return out


def rec_bands(d, level):
    """the bands a synthesis comb goes into, one at a time: the approximation, the all-high-pass detail of the finest level, one mixed
    detail (high-pass on the first axis only; 1-D: the detail) of the coarsest"""
    nb, nd = orc.num_bands(d, level), (1 << d) - 1
    finest_all_high = nb - 1                                     # details of the finest level come last; bits 2^d - 1 is the last of them
    coarsest_mixed = 1                                           # band 1 = detail 1 of the coarsest level: high-pass on axis 0
    assert finest_all_high == 1 + nd * (level - 1) + nd - 1
    return sorted({0, finest_all_high, coarsest_mixed})


def rec_combs(shape, positions, reach, level, cplx=False, pairs=False):
    """[(band, coefficients of shape + (bands,))]: every comb of `combs` in each band of rec_bands, all other bands zero"""
    d = len(shape)
    nb = orc.num_bands(d, level)
    out = []
    for x in combs(shape, positions, reach, cplx=cplx, pairs=pairs):
        for b in rec_bands(d, level):
            c = np.zeros(tuple(shape) + (nb,), dtype=x.dtype)
            c[..., b] = x
            out.append((b, c))
    return out
