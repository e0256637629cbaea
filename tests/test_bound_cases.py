"""The componentwise bound of tests/bound_cases.py is sharp without any kernel: on the comb inputs an oracle whose smallest low-pass and
smallest high-pass tap are off by 1e-4 of themselves fails it, and a plain float32 restatement of the transform with the true taps passes
it.  The mutant's error in the metric of the parity tests (max|got - want| / max|want|) is printed beside it: the gap is on record."""
import numpy as np
import pytest

import bound_cases as bc
import ndwt_oracle as orc

SHAPES = {1: [96], 2: [44, 41], 3: [44, 41, 40]}                 # every axis holds the reach of two 20-tap levels (39) once
WAVELETS = ["db4", "db7", "db8", "db9", "db10"]


def _reach(L, level, dil):
    return level * L if dil == "reference" else ((1 << level) - 1) * (L - 1) + 1


def _setup(wn, d, level, dil):
    filt = bc.filters(wn, d)
    L = len(filt[0][0])
    shape = SHAPES[d]
    if min(shape) < _reach(L, level, dil):                       # a dilated level reaches further: 1-D and 2-D take longer axes, 3-D runs
        if d == 3:                                               # the dilated walk for the wavelets that fit (the supports must not wrap
            return None                                          # onto themselves, or the smallest tap is never alone in an element)
        shape = [96] if d == 1 else [64, 60]
    # the wrap and an edge in the interior, as a tile edge would sit
    pos = [bc.axis_positions(n, [n // 2 + 1]) for n in shape]
    return shape, filt, pos, [_reach(L, level, dil)] * d


def _inputs(direction, shape, pos, reach, level):
    if direction == "dec":
        return [(None, x) for x in bc.combs(shape, pos, reach)]
    return bc.rec_combs(shape, pos, reach, level)


def _transform(direction, v, filt, level, l2, dil, f32=False):
    if direction == "dec":
        return (bc.f32_dec if f32 else bc.walk_dec)(v, filt, level, l2, dil)
    return (bc.f32_rec if f32 else bc.walk_rec)(v, filt, l2, dil, level)


def _cond(direction, v, filt, level, l2, dil):
    return bc.abs_dec(v, filt, level, l2, dil) if direction == "dec" else bc.abs_rec(v, filt, l2, dil, level)


@pytest.mark.parametrize("direction", ["dec", "rec"])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("wn", WAVELETS)
def test_mutant_fails_and_float32_restatement_passes(wn, d, direction):
    u = bc.U["single"]
    for level, l2, dil in ((1, 1, "reference"), (2, 0, "reference"), (2, 1, "atrous")):
        case = _setup(wn, d, level, dil)
        if case is None:
            continue
        shape, filt, pos, reach = case
        c = bc.cap(filt, level)
        inputs = _inputs(direction, shape, pos, reach, level)
        worst, caught = 0.0, {"lo+hi": False, "lo": False, "hi": False}
        old_metric = 0.0
        for band, v in inputs:
            want = _transform(direction, v, filt, level, l2, dil)
            cond = _cond(direction, v, filt, level, l2, dil)
            assert (cond >= np.abs(want)).all()                                  # |W||x| bounds |W x|
            # the plain float32 restatement, true taps: under the derived cap
            got = _transform(direction, v, filt, level, l2, dil, f32=True)
            worst = max(worst, bc.check_componentwise(got, want, cond, c, u, f"f32 {wn} {d}-D {direction} L{level} band {band}"))
            # the mutants, computed in double: only the tap is wrong
            for name, which in (("lo+hi", ("lo", "hi")), ("lo", ("lo",)), ("hi", ("hi",))):
                bad = _transform(direction, v, bc.mutate(filt, 1e-4, which=which), level, l2, dil)
                if name == "lo+hi":
                    old_metric = max(old_metric, bc.relerr(bad, want))
                try:
                    bc.check_componentwise(bad, want, cond, c, u)
                except AssertionError:
                    caught[name] = True
        print(f"[bound] {wn} {d}-D {direction} L{level} l2={l2} {dil}: float32 restatement worst {worst:.3g} u cond (cap {c}); "
              f"1e-4 mutant in the old metric {old_metric:.3g} (TOL 2e-6), caught by the bound: {caught}")
        assert worst <= c
        assert all(caught.values()), (wn, d, direction, level, caught)


def test_complex_input_magnitude_and_zero_rule():
    """complex data: |re| + |im| is the input magnitude; a value where no tap reaches fails however small it is"""
    filt = bc.filters("db2", 1)
    x = np.zeros(32, dtype=np.complex128)
    x[5] = 0.375 - 1.25j
    want = bc.walk_dec(x, filt, 1, 1)
    cond = bc.abs_dec(x, filt, 1, 1)
    assert np.count_nonzero(cond[:, 0]) == 4 and cond.max() <= 1.625
    assert bc.check_componentwise(want.astype(np.complex64), want, cond, bc.cap(filt, 1), bc.U["single"]) <= 1.0   # one rounding
    got = want.copy()
    got[20, 1] = 1e-30
    with pytest.raises(AssertionError, match="where no tap reaches"):
        bc.check_componentwise(got, want, cond, bc.cap(filt, 1), bc.U["single"])
    got = want.copy()
    got[np.unravel_index(np.argmin(np.where(cond > 0, cond, 9)), cond.shape)] *= 1 + 1e-5                          # the smallest element alone
    with pytest.raises(AssertionError, match="the cap is"):
        bc.check_componentwise(got, want, cond, bc.cap(filt, 1), bc.U["single"])


def test_cap_and_comb_properties():
    filt = bc.filters(["db10", "db7", "db8"])
    assert bc.cap(filt, 2) == 2 * (22 + 16 + 18) and bc.cap(filt, 1, axes=[1]) == 16
    for k in range(40):
        a = bc.amplitude(k)
        assert np.float32(a) == a and np.log2(abs(a)) % 1 != 0               # exact in float32, no power of two
    assert {np.sign(bc.amplitude(k)) for k in range(4)} == {-1.0, 1.0}
    pos = bc.axis_positions(72, bc.tile_edges(72, 64, anchor_last=True))
    assert pos == [0, 7, 8, 63, 64, 71]
    cs = bc.combs([72, 40], [pos, bc.axis_positions(40)], [40, 40])
    hit = np.zeros(72, bool)                                     # every position of the axis is in some comb
    for c in cs:
        hit |= np.abs(c).sum(axis=1) > 0
    assert sorted(np.flatnonzero(hit)) == pos
    assert bc.rec_bands(3, 2) == [0, 1, 14] and bc.rec_bands(1, 2) == [0, 1, 2] and bc.rec_bands(2, 1) == [0, 1, 3]
    assert orc.num_bands(3, 2) == 15
