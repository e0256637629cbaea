"""Two or three 2-D levels in one launch (Fwd2C / Inv2C) on double and interleaved complex images.

Every row forces the cascade on a small image (variant 11; the synthesis also with 12, two rows of band loads in flight where that
instance exists) and checks, for dec, rec of random coefficients, soft / hard denoise and the round trip:

  * the launch trace: the cascade kernels with the row's T, EW, L, NLEV (and PD) in the split the instance table gives (INSTANCES below,
    written down from csrc/ndwt_fused_list.h), on a grid of tiles x ceil(n2 / rows per wave);
  * the fp64 oracle (oracle/ndwt_spatial.c) within TOL of tests/test_gpu_parity.py (dec) and 2 TOL max(|want|, |c|) (rec);
  * one launch per level (variant 9): dec bit for bit; rec to 2 TOL -- DESIGN.md 4.3 promises rounding agreement only for the new kinds:
    the complex64 form packs its y stage where Inv2S rounds a two-term sum first, and the double form follows Inv2P<double> but may
    run where the per-level default is Inv2S; denoise within 4 TOL.

Fallback rows (rows that are not whole groups of 4 scalars, an unaligned pointer, a band pitch that breaks the 4-scalar alignment) must
run one launch per level and still agree with the oracle.  The default rows are the smallest images that take the cascade unasked
(csrc/ndwt_select.h: cascade2_min_bytes, per kind and direction), and the images one row shorter.  The last test is the coverage gate over INSTANCES.
"""
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
import ndwt_spatial as orc_c

pytestmark = pytest.mark.gpu

TOL = {"double": 1e-12, "single": 2e-6}                       # tests/test_gpu_parity.py
KINDS = {"c64": ("single", True), "f64": ("double", False), "c128": ("double", True)}
CASCADE = ("Fwd2C", "Inv2C")

# ---- the instance table (csrc/ndwt_fused_list.h: NDWT_LIST_{C64,F64,C128}_{FWD,INV}2C): (family, T, EW, L, NLEV, PD, WPE)
def _table():
    t = set()
    for L in (2, 4, 6, 8):
        for nlev in (2, 3):
            t.add(("Fwd2C", "float", 2, L, nlev, 0, 2))
            for pd in (1, 2):
                if (L, nlev, pd) != (8, 3, 2):
                    t.add(("Inv2C", "float", 2, L, nlev, pd, 2))
            for ew in (1, 2):
                t.add(("Fwd2C", "double", ew, L, nlev, 0, 2 if (L <= 4 or (L, nlev) == (6, 2)) else 1))
                if (ew, L, nlev) != (2, 8, 3):
                    t.add(("Inv2C", "double", ew, L, nlev, 1, 2 if (L == 2 or (L, nlev) == (4, 2)) else 1))
    return t


INSTANCES = _table()
# default dispatch: bytes of the smallest image that takes the cascade without being asked, (analysis, synthesis): cascade2_min_bytes
MIN_BYTES = {"c64": (32 << 20, 32 << 20), "f64": (32 << 20, 128 << 20), "c128": (64 << 20, 64 << 20)}


def _exists(fam, kind, L, nlev, pd):
    T, ew = ("float" if KINDS[kind][0] == "single" else "double"), (2 if KINDS[kind][1] else 1)
    return any(i[:6] == (fam, T, ew, L, nlev, pd) for i in INSTANCES)


def cascade_split(kind, inverse, L, level, want_pd=1):
    """[(nlev, pd)] of the cascade launches of a `level`-level transform, and how many levels are left to one launch each"""
    fam, out, left = ("Inv2C" if inverse else "Fwd2C"), [], level
    while left >= 2:
        n = 3 if (left >= 3 and _exists(fam, kind, L, 3, 1 if inverse else 0)) else 2 if _exists(fam, kind, L, 2, 1 if inverse else 0) else 0
        if not n:
            break
        out.append((n, (want_pd if _exists(fam, kind, L, n, want_pd) else 1) if inverse else 0))
        left -= n
    return out, left


def tile_width(kind, inverse, L, nlev):
    prec, cplx = KINDS[kind]
    ew, lpl = (2 if cplx else 1), (8 if prec == "single" else 4)
    LH, RH = (L // 2, L // 2 - 1) if inverse else (L // 2 - 1, L // 2)
    return 4 * ((64 - nlev * ((LH * ew + 3) // 4 + (RH * ew + 3) // 4)) // lpl * lpl)


def K(rid, kind, dims, wn, level, chunk=None, layout="packed"):
    return pytest.param(dict(kind=kind, dims=dims, wn=wn, level=level, chunk=chunk, layout=layout), id=rid)


# sizes in elements; a complex row of n1 elements is 2 n1 scalars
ROWS = []
for _k in ("c64", "c128"):
    ROWS += [K(f"{_k}-db4-l3-two-tiles", _k, [128, 50], "db4", 3, 17),     # 256 scalars: two tiles; 17 rows per wave < the march-in of 21
             K(f"{_k}-db3-l2", _k, [128, 38], "db3", 2, 13),
             K(f"{_k}-db1-l5", _k, [96, 64], "db1", 5),                     # launches of 3 + 2 levels
             K(f"{_k}-db2-db3-l4", _k, [132, 80], ["db2", "db3"], 4),       # 3 + 1
             K(f"{_k}-db2-l5", _k, [128, 40], "db2", 5, 9),                 # 4 taps: 3 + 2
             K(f"{_k}-db4-l2", _k, [128, 50], "db4", 2)]
ROWS += [K("f64-db4-l3-two-tiles", "f64", [256, 50], "db4", 3, 17),
         K("f64-db3-l2", "f64", [256, 38], "db3", 2),
         K("f64-db1-l5", "f64", [512, 64], "db1", 5),
         K("f64-db3-l4", "f64", [260, 80], "db3", 4),
         K("f64-db2-l5", "f64", [256, 40], "db2", 5, 9),
         K("f64-db4-l2", "f64", [256, 50], "db4", 2)]
FALLBACK_ROWS = [K("c64-n1-65", "c64", [65, 50], "db4", 3), K("c128-n1-65", "c128", [65, 50], "db2", 3),
                 K("c64-offset", "c64", [128, 50], "db4", 3, layout="offset"), K("f64-offset", "f64", [256, 50], "db4", 3, layout="offset"),
                 K("c64-pitch", "c64", [128, 50], "db4", 3, layout="pitch"), K("f64-pitch", "f64", [256, 50], "db4", 3, layout="pitch")]


def _np_shrink(c, t, hard):
    m = np.abs(c)
    out = c * (np.where(m > t, 1.0, 0.0) if hard else np.where(m > t, (m - t) / np.where(m > 0, m, 1.0), 0.0))
    out[..., 0] = c[..., 0]
    return out


class _Buf:
    def __init__(self, n, tdt, off):
        self.t = torch.zeros(n + 8, dtype=tdt, device="cuda")
        self.off, self.n, self.view = off, n, self.t[off:off + n]

    def ptr(self):
        return self.view.data_ptr()


_RECS = {}          # row id -> cascade launch records of a row that passed


def run_kind_row(rid, row):
    kind, dims, wn, level, chunk = row["kind"], row["dims"], row["wn"], row["level"], row["chunk"]
    prec, cplx = KINDS[kind]
    wl = [wn] * 2 if isinstance(wn, str) else wn
    L = max(2 * int(w[2:]) for w in wl)
    tol = TOL[prec]
    rdt = torch.float32 if prec == "single" else torch.float64
    ndt = (np.complex64 if prec == "single" else np.complex128) if cplx else (np.float32 if prec == "single" else np.float64)
    tdt = (torch.complex64 if prec == "single" else torch.complex128) if cplx else rdt
    T, ew = ("float" if prec == "single" else "double"), (2 if cplx else 1)
    rng = np.random.default_rng(zlib.crc32(repr((rid, dims, wn, level)).encode()))
    x = rng.standard_normal(dims) + (1j * rng.standard_normal(dims) if cplx else 0)
    x = x.astype(ndt).astype(np.complex128 if cplx else np.float64)
    nb, vol = ndwt.num_bands(2, level), int(np.prod(dims))
    off = 1 if row["layout"] == "offset" else 0
    pitch = vol + (1 if vol % 4 == 0 else 0) + (2 if vol % 4 in (1, 3) else 0) if row["layout"] == "pitch" else vol
    bp = 0 if pitch == vol else pitch
    fallback = row["layout"] != "packed" or (dims[0] * ew) % 4 != 0
    stream = torch.cuda.current_stream().cuda_stream

    def plan(vf, vi):
        p = ndwt.Plan(dims, wl, rdt, cplx, True, "reference", max_level=level)
        p.set_variant(fwd=vf, inv=vi)
        if chunk and vf != 9:
            p.set_tuning(0, chunk)
        return p

    def to_dev(a, n_bands=None):
        if n_bands is None:
            b = _Buf(vol, tdt, off)
            b.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(a)).astype(ndt).reshape(-1)).cuda())
            return b
        ck = np.ascontiguousarray(np.transpose(a)).astype(ndt).reshape(n_bands, vol)
        b = _Buf(n_bands * pitch, tdt, off)
        for k in range(n_bands):
            b.view[k * pitch:k * pitch + vol] = torch.from_numpy(ck[k]).cuda()
        return b

    def coef(b):
        ck = torch.stack([b.view[k * pitch:k * pitch + vol] for k in range(nb)]).cpu().numpy().reshape([nb] + dims[::-1])
        return np.transpose(ck)

    def image(b):
        return np.transpose(b.view.cpu().numpy().reshape(dims[::-1]))

    def check_launches(recs, inverse, want_pd, what):
        fam = "Inv2C" if inverse else "Fwd2C"
        cas = [r for r in recs if r.family in CASCADE]
        if fallback:
            assert not cas and len(recs) == level, f"{what}: expected one launch per level, launched {recs}"
            return []
        split, left = cascade_split(kind, inverse, L, level, want_pd)
        got = [(r.family, r.params["T"], r.params["EW"], r.params["L"], r.params["NLEV"], r.params["PD"] if inverse else 0) for r in cas]
        assert got == [(fam, T, ew, L, n, pd) for n, pd in split], f"{what}: cascade launches {cas}, expected {fam} x {split}"
        assert len(recs) == len(split) + left, f"{what}: {len(recs)} launches, expected {len(split)} cascades + {left} levels: {recs}"
        for r, (n, _) in zip(cas, split):
            tiles = -(-dims[0] * ew // tile_width(kind, inverse, L, n))
            rows = min(chunk if chunk else n * (L - 1), dims[1])   # unforced, on an image this small: the shortest chunk the host allows
            each = -(-dims[1] // -(-dims[1] // rows))       # (the host equalises the waves: cascade2_launch in csrc/ndwt_api.hip)
            assert r.grid == (tiles * -(-dims[1] // each), 1, 1) and r.block == (64, 1, 1), f"{what}: {r!r}, expected {tiles} tiles x ceil({dims[1]} / {rows})"
            assert (r.family, T, ew, L, n, r.params["PD"] if inverse else 0, r.params["WPE"]) in INSTANCES, f"{what}: {r!r} is not in the table"
        return cas

    p9, launched = plan(9, 9), []
    xb = to_dev(x)
    # ---- dec: the oracle, and bit for bit one launch per level
    want = orc_c.spatial_dec(x, wl, level, 1)
    y9 = _Buf(nb * pitch, tdt, off)
    p9.dec(xb.ptr(), y9.ptr(), level, stream, band_pitch=bp)
    p11 = plan(11, 11)
    yb = _Buf(nb * pitch, tdt, off)
    with ndwt.kernel_trace() as recs:
        p11.dec(xb.ptr(), yb.ptr(), level, stream, band_pitch=bp)
    torch.cuda.synchronize()
    launched += check_launches(recs, False, 0, f"dec {rid}")
    err = np.abs(coef(yb) - want).max() / np.abs(want).max()
    print(f"{rid}: dec error {err:.3g} (bound {tol:.3g})")
    assert err <= tol, (rid, "dec", err)
    assert torch.equal(yb.view.view(rdt), y9.view.view(rdt)), f"{rid}: dec differs from one launch per level"
    # ---- rec of random coefficients, one and two rows of band loads in flight
    c = rng.standard_normal(want.shape) + (1j * rng.standard_normal(want.shape) if cplx else 0)
    c = c.astype(ndt).astype(want.dtype)
    want_r = orc_c.spatial_rec(c, wl, 1)
    scale = max(np.abs(want_r).max(), np.abs(c).max())
    cb = to_dev(c, nb)
    r9 = _Buf(vol, tdt, off)
    p9.rec(cb.ptr(), r9.ptr(), level, stream, band_pitch=bp)
    for vi, pd in ((11, 1), (12, 2)):
        p = plan(11, vi)
        rb = _Buf(vol, tdt, off)
        with ndwt.kernel_trace() as recs:
            p.rec(cb.ptr(), rb.ptr(), level, stream, band_pitch=bp)
        torch.cuda.synchronize()
        launched += check_launches(recs, True, pd, f"rec {rid} variant {vi}")
        err, d9 = np.abs(image(rb) - want_r).max() / scale, np.abs(image(rb) - image(r9)).max() / scale
        print(f"{rid}: rec variant {vi} error {err:.3g}, against one launch per level {d9:.3g} (bound {2 * tol:.3g})")
        assert err <= 2 * tol, (rid, "rec", vi, err)
        assert d9 <= 2 * tol, (rid, "rec against per-level", vi, d9)
        assert float(rb.t[:off].abs().sum()) == 0 and float(rb.t[off + vol:].abs().sum()) == 0      # nothing written outside the output
        # ---- round trip
        p.rec(yb.ptr(), rb.ptr(), level, stream, band_pitch=bp)
        torch.cuda.synchronize()
        err = np.abs(image(rb) - x).max() / np.abs(x).max()
        assert err <= 20 * tol, (rid, "round trip", vi, err)
    # ---- denoise, soft and hard: the per-level result; the oracle with the magnitude shrunk (complex: |re + i im|)
    thr = float(np.median(np.abs(want[..., 1:])))
    for hard in (False, True):
        o9, ob = _Buf(vol, tdt, off), _Buf(vol, tdt, off)
        p9.denoise(xb.ptr(), o9.ptr(), level, thr, hard, stream)
        with ndwt.kernel_trace() as recs:
            p11.denoise(xb.ptr(), ob.ptr(), level, thr, hard, stream)
        torch.cuda.synchronize()
        cas = [r for r in recs if r.family in CASCADE]
        # (the coefficients of a denoise live in the plan's own scratch at its own pitch: a caller's band pitch does not reach them)
        assert bool(cas) == (not fallback or row["layout"] == "pitch"), f"denoise {rid}: {recs}"
        launched += [] if fallback else cas
        want_x = orc_c.spatial_rec(_np_shrink(want, thr, hard), wl, 1)
        d9 = np.abs(image(ob) - image(o9)).max() / max(np.abs(image(o9)).max(), 1.0)
        print(f"{rid}: {'hard' if hard else 'soft'} denoise against one launch per level {d9:.3g} (bound {4 * tol:.3g})")
        assert d9 <= 4 * tol, (rid, "denoise against per-level", hard, d9)
        if not hard:                                          # (hard: a coefficient within rounding of the threshold may fall either side)
            err = np.abs(image(ob) - want_x).max() / max(np.abs(want_x).max(), 1.0)
            assert err <= 20 * tol, (rid, "soft denoise against the oracle", err)
    return launched


def cascade_records(rid, row):
    if rid not in _RECS:
        _RECS[rid] = run_kind_row(rid, row)
    return _RECS[rid]


@pytest.mark.parametrize("row", ROWS)
def test_cascade_kind_row(row, request):
    assert cascade_records(request.node.callspec.id, row)


@pytest.mark.parametrize("row", FALLBACK_ROWS)
def test_fallback_row_runs_one_launch_per_level(row, request):
    assert run_kind_row(request.node.callspec.id, row) == []


@pytest.mark.parametrize("kind", sorted(MIN_BYTES))
@pytest.mark.parametrize("inverse", [False, True], ids=["dec", "rec"])
def test_default_takes_the_cascade_from_the_kind_threshold_on(kind, inverse):
    """the smallest image of 2048 elements per row that takes the cascade unasked, db4, three levels, no variant: the launches of the
    instance table's split (ndwt_plan_get_profile) and, for dec, the bits of one launch per level; one row fewer: three launches"""
    prec, cplx = KINDS[kind]
    rdt = torch.float32 if prec == "single" else torch.float64
    comp = 2 if cplx else 1
    n1, level = 2048, 3
    n2 = MIN_BYTES[kind][inverse] // (n1 * comp * (4 if prec == "single" else 8))
    split, left = cascade_split(kind, inverse, 8, level)
    stream = torch.cuda.current_stream().cuda_stream
    nb = ndwt.num_bands(2, level)
    x = torch.randn(n2 * n1 * comp, dtype=rdt, device="cuda")
    y = torch.randn(nb * x.numel(), dtype=rdt, device="cuda") if inverse else torch.empty(nb * x.numel(), dtype=rdt, device="cuda")
    outs = []
    for rows, vf, want_launches in ((n2, -1, len(split) + left), (n2, 9, level), (n2 - 1, -1, level)):
        p = ndwt.Plan([n1, rows], ["db4"] * 2, rdt, cplx, True, "reference", max_level=level)
        if vf >= 0:
            p.set_variant(fwd=vf, inv=vf)
        p.set_profiling(True)
        if inverse:
            out = torch.empty_like(x)
            p.rec(y.data_ptr(), out.data_ptr(), level, stream)
        else:
            out = torch.empty_like(y)
            p.dec(x.data_ptr(), out.data_ptr(), level, stream)
        torch.cuda.synchronize()
        assert p.get_profile(1 if inverse else 0)[1] == want_launches, (kind, inverse, rows, vf, p.get_profile(1 if inverse else 0))
        outs.append(out)
    if inverse:
        d = float((outs[0] - outs[1]).abs().max()) / max(float(outs[1].abs().max()), float(y.abs().max()))
        print(f"{kind} default rec against one launch per level: {d:.3g} (bound {2 * TOL[prec]:.3g})")
        assert d <= 2 * TOL[prec]
    else:
        assert torch.equal(outs[0], outs[1])


def test_every_instance_of_the_table_was_launched():
    """the coverage gate: every entry of INSTANCES ran in some row above (each of which agreed with the oracle)"""
    recs = [r for p in ROWS for r in cascade_records(p.id, p.values[0])]
    ran = {(r.family, r.params["T"], r.params["EW"], r.params["L"], r.params["NLEV"], r.params["PD"] if r.family == "Inv2C" else 0, r.params["WPE"])
           for r in recs}
    assert not (INSTANCES - ran), f"never launched: {sorted(INSTANCES - ran)}"
