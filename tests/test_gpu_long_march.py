"""Every fused kernel over full turns of its plane window.

The fused kernels of csrc/ndwt_device.h keep a window of L planes (rows) and pick, at every step of their march, one of L compile-time
specialisations of the step body (zdispatch / yzdispatch / rot_dispatch, the load slots of Inv2P / Inv2C): separate code with its own slot
indices, LDS slots (WLDS), register sets (DEPTH) and pending sums (ZLDS).  On the small shapes of tests/test_gpu_dispatch.py the launch
geometry (csrc/ndwt_geom.h) fills the chip with chunks of 2 planes, so only the first few of the L specialisations ever store anything.

Here every row is a twin of a row of test_gpu_dispatch.ROWS -- the same n1, n2, wavelets, layout, variant -- with the marched axis
(n3; n2 of an image) long enough and the chunk forced (Plan.set_tuning) so that a workgroup's march is more than two turns of the window:

    L = padded tap length,  chunk C = 2 L + 1,  marched length N >= 3 L + 2 with N % C != 0

so the first chunk of every tile emits 2 L + 1 planes and the last one is shorter, starts off plane 0 and ends on the periodic wrap.  A
dilated row obeys the rule on the sub-lattice of its deepest fused level (N / stride).  A cascade (Fwd2C / Inv2C) takes the forced value
as rows per wave and equalises them: n2 is chosen so that every wave emits at least 2 L + 1 rows and the last one fewer.  run_row checks
dec, rec, round trip and soft denoise against the fp64 oracle with the tolerances of test_gpu_dispatch; this module adds the proof, from the
grid of every fused launch record, that the chunk took effect, and a coverage gate over the fused entries of helpers.COVERAGE.
"""
import pytest

from helpers import COVERAGE, check_trace, matches
from test_gpu_dispatch import ROWS, R, run_row

pytestmark = pytest.mark.gpu

FUSED3 = ("Fwd3", "Inv3", "Inv3S", "Inv3Y", "Den3")
FUSED2 = ("Fwd2S", "Inv2S", "Inv2P")
CASCADE2 = ("Fwd2C", "Inv2C")
BASE = {p.id: p.values[0] for p in ROWS + [
    # Den3 at 8 taps keeps 6 of its 8 pending z sums in LDS (ZLDS); ndwt_denoise takes it only on request (set_fused_level1(2)), so no row
    # of test_gpu_dispatch runs it
    R("den3-db4-on-request", [64, 40, 36], "db4", level=2, fused_level1=2, dec=["Fwd3 L=8"], rec=["Inv3Y L=8"],
      den=["Fwd3 L=8 LOWONLY=true", "Den3 L=8 ZLDS=6", "Fwd3 L=8 LOWONLY=false", "Inv3Y L=8"]),
]}


def _taps(row):
    """the padded tap length of the row's fused kernels (csrc/ndwt_select.h: padded_len over x, y, z; the longer axis of an image)"""
    d = len(row["dims"])
    wl = [row["wn"]] * d if isinstance(row["wn"], str) else row["wn"]
    return max(2 * int(w[2:]) for w in wl[:3])


def twin(rid, n, sub=1, force=True, chunk=None, tag="-long", **changed):
    """the row `rid` with its marched axis `n` long and chunks of 2 L + 1; sub: tap stride of the deepest fused level of a dilated row;
    force = False: a row of the per-axis kernels, which size their own march; chunk: rows per wave of a cascade twin (checked below)"""
    row = dict(BASE[rid])
    L = _taps(row)
    dims = list(row["dims"])
    dims[1 if len(dims) == 2 else 2] = n
    C = 2 * L + 1
    assert n % sub == 0 and n // sub >= 3 * L + 2 and (chunk or (n // sub) % C != 0), (rid, n, L)
    row.update(dims=dims, chunk=(chunk or C) if force else None, **changed)
    return rid + tag, row


# 3-D / 4-D rows march n3 = 3 L + 2 planes (the remainder is L + 1); an image keeps its n2 where that already obeys the rule
LONG_ROWS = [
    # ---- the rows of test_gpu_dispatch.COVERAGE_ROWS (the 1-D rows have no marched axis: AxisX keeps no window)
    twin("tall-tile-4d-frames-32", 26), twin("tall-tile-4d-frames-16", 26),
    twin("pin-db6", 38), twin("nopin-n1-70", 32), twin("inv3y-scatter-20", 62), twin("inv3y-gather-20-ragged", 62),
    twin("inv3y-uniyz-false", 38), twin("inv3s-odd-16", 50),
    twin("c64-db5", 32), twin("c128-db5", 32),
    twin("c128-db6", 38, force=False),                      # (its synthesis is per-axis: AxisMarch takes min(n, 4 (L - 1)) steps on its own)
    twin("c128-db6", 38, tag="-long-forced"),               # ... and its analysis, Fwd3<double, 12, EW = 2, WLDS = 2>, in chunks of 25 planes
    twin("atrous-db4-l3", 104, sub=4), twin("atrous-db4-l3-offset", 104, sub=4),
    twin("atrous-indivisible", 30, sub=2),                  # 30 % 4 != 0: level 3 stays per-axis, level 2 marches 15 planes per sub-lattice
    # level 1 of the image is 104 rows of tap stride 1: n2 >= 64 makes that synthesis Inv2P (fused2_select); the dilated levels keep Inv2S
    twin("atrous-2d-l3", 104, sub=4, rec=["Inv2P L=8 PD=4 PK=true", "Inv2S L=8 EW=2", "Inv2S L=8 EW=4"]),
    twin("f64-db4", 26),
    twin("inv2p-n2-64", 70), twin("2d-db9-ragged", 65), twin("2d-f64-db8", 96), twin("2d-f64-db4", 96), twin("2d-c64-db5", 70),
    twin("den3-db2", 14), twin("den3-db4-on-request", 26), twin("den-4d", 14), twin("fwd7-folded-t", 14), twin("inv3-lds-kernel", 26), twin("inv7-inv2p-scalar", 70),
    # cascades: ceil(n2 / chunk) = 3 waves along y of 17 + 17 + 16, 13 + 13 + 12 and 25 + 25 + 24 rows (74 rows: Inv2P needs n2 >= 64)
    twin("fwd11-inv11-small-cascade", 50, chunk=17), twin("fwd10-inv12-small-cascade", 38, chunk=13), twin("fwd11-db6-cascade-2lev", 74, chunk=25),
    # ---- fp64, pinned taps, scatter / lane-shift synthesis, complex64 and the long 2-D filters
    twin("f64-db3", 20), twin("f64-db5", 32), twin("f64-db6", 38), twin("f64-db7", 44), twin("f64-db8", 50),
    twin("f64-db9-per-axis", 56, force=False),
    twin("pin-db5", 32), twin("pin-db7", 44), twin("inv3y-scatter-16", 50), twin("inv3y-scatter-18", 56), twin("inv3s-odd-14", 44),
    twin("c64-db4", 26), twin("c64-db6", 38),
    twin("2d-db7-long", 96), twin("2d-db10-long", 70), twin("2d-c64-db8", 70),
    twin("inv2s-n2-63", 63),                                # Inv2S<8, EW = 1> on rows of whole groups of 4 (the image above took Inv2P there)
]


# ---- launch geometry, restated from csrc/ndwt_select.h (fused2_tile_width) and the cascade launch units (fwd2c_ / inv2c_tile_width)
def fused2_tile_width(inverse, Lp, ew):
    LH, RH = (Lp // 2, Lp // 2 - 1) if inverse else (Lp // 2 - 1, Lp // 2)
    return 4 * (64 - (LH * ew + 3) // 4 - (RH * ew + 3) // 4)


def cascade2_tile_width(Lp, nlev):
    return 4 * ((64 - nlev * ((Lp // 2 - 1 + 3) // 4 + (Lp // 2 + 3) // 4)) // 8 * 8)


def _ceil(a, b):
    return -(-a // b)


def march_of(row, r):
    """(tiles, batch items, marched length) of a fused launch record of this row"""
    dims, p = row["dims"], r.params
    n1s = dims[0] * (2 if row["cplx"] else 1)                   # scalars along x
    s = p.get("EW", 1) if row["dil"] == "atrous" else 1         # a dilated level: x through EW = stride, the sub-lattices as batch items
    if r.family in FUSED3:
        batch = s * s if s > 1 else (dims[3] if len(dims) == 4 else 1)
        return _ceil(n1s, p["TX"]) * _ceil(dims[1] // s, p["TY"]), batch, dims[2] // s
    if r.family in FUSED2:
        return _ceil(n1s, fused2_tile_width(r.family != "Fwd2S", p["L"], p.get("EW", 1))), s, dims[1] // s
    assert r.family in CASCADE2, r
    return _ceil(n1s, cascade2_tile_width(p["L"], p["NLEV"])), 1, dims[1]


def check_long_march(row, recs, what):
    """every fused launch ran chunks of row["chunk"] (its grid says so) and so emitted at least 2 L + 1 planes per workgroup, the last
    chunk fewer; returns the fused records"""
    C, fused = row["chunk"], [r for r in recs if r.family in FUSED3 + FUSED2 + CASCADE2]
    assert fused, f"{what}: no fused launch"
    for r in fused:
        L = r.params["L"]
        tiles, batch, n = march_of(row, r)
        nchunks = _ceil(n, C)
        assert r.grid == (tiles * batch * nchunks, 1, 1), f"{what}: {r!r} did not run {tiles} tiles x {batch} x ceil({n} / {C}) chunks"
        each = _ceil(n, nchunks) if r.family in CASCADE2 else C     # (a cascade equalises its waves: cascade2_launch in csrc/ndwt_api.hip)
        last = n - (nchunks - 1) * each
        assert each >= 2 * L + 1 and 0 < last < each, f"{what}: {r!r} marches {each} planes per workgroup, {last} in the last"
    return fused


_RECS = {}          # row id -> fused launch records of a row that passed (the gate below re-uses what the row tests ran)


def long_march_records(rid, row):
    if rid not in _RECS:
        recs = run_row(row)
        _RECS[rid] = check_long_march(row, recs, rid) if row["chunk"] else []
    return _RECS[rid]


@pytest.mark.parametrize("rid,row", LONG_ROWS, ids=[rid for rid, _ in LONG_ROWS])
def test_long_march_row(rid, row):
    long_march_records(rid, row)


def test_long_march_coverage():
    """every fused-family entry of helpers.COVERAGE is launched by this sweep with at least 2 L + 1 emitting steps per workgroup"""
    recs = [r for rid, row in LONG_ROWS for r in long_march_records(rid, row)]
    missing = [f"{fam} {' '.join(f'{k}={v}' for k, v in p.items())}" for fam, p in COVERAGE
               if fam in FUSED3 + FUSED2 + CASCADE2 and not any(matches(r, (fam, p)) for r in recs)]
    assert not missing, f"no long march of: {missing}"


def test_a_sweep_that_runs_short_chunks_fails():
    """the proof above has teeth: the same row without the forced chunk is rejected by it"""
    row = dict(LONG_ROWS)["f64-db4-long"]
    recs = run_row(dict(row, chunk=None))
    check_trace(recs, row["dec"] + row["rec"] + row["den"], "f64-db4 unforced")
    with pytest.raises(AssertionError, match="did not run"):
        check_long_march(row, recs, "f64-db4 unforced")
