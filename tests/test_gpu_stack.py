"""Stacks of images and volumes (ndwt_plan_create_axes): the 2-D or 3-D transform of every item of [n1, n2, K] / [n1, n2, n3, K], no filter
along the last axis.

Every row checks
  1. the launch trace: the kernel family, its T, L, NLEV, EW and the grid -- ntx nyc K waves for the 2-D families, the workgroups of one
     item times K for the 3-D ones;
  2. the fp64 oracle (oracle/ndwt_spatial.c) applied to each item alone: dec, rec of random coefficients and the round trip, within TOL of
     tests/test_gpu_parity.py (dec) and 2 TOL max(|want|, |c|) (rec);
  3. bits: dec of item j equals dec of that item on an unbatched plan pinned to the same variants, bit for bit; rec is held to the
     tolerance, and whether it is bit-identical is printed;
  4. isolation: with item 1 of the input (rec: of every band) filled with NaN, items 0 and 2 of the result are bit-identical to the clean
     run and free of NaN -- the test of the y / z wrap and of the item offset;
  5. guard elements before and after every output buffer, and with a pitch the gap between bands;
  6. on one row per kind, ndwt_shrink / ndwt_denoise against numpy dec -> shrink -> rec of the oracle.

Fallback rows (a-trous dilation, db9 in double, an offset pointer, a pitch that breaks the 4-scalar alignment) must trace per-axis or
one-level kernels only and still meet the oracle.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
import ndwt_spatial as orc_c

pytestmark = pytest.mark.gpu

TOL = {"double": 1e-12, "single": 2e-6}                       # tests/test_gpu_parity.py
KINDS = {"f32": ("single", False), "c64": ("single", True), "f64": ("double", False), "c128": ("double", True)}
CASCADE = ("Fwd2C", "Inv2C")
ONE_LEVEL_2D = ("Fwd2S", "Inv2S", "Inv2P")
FUSED_3D = ("Fwd3", "Inv3", "Inv3S", "Inv3Y")
PER_AXIS = ("AxisX", "AxisMarch", "axis_analysis_kernel", "axis_synthesis_kernel")
# the most levels one Inv2C launch takes where that is not 3 (csrc/ndwt_fused_list.h): complex128, 8 taps
INV_TOP = {("c128", 8): 2}


def cdiv(a, b):
    return -(-a // b)


def wave_row_width(syn, Lp, ew, f64, nlev):
    """csrc/ndwt_fused_tile.h: scalars of a row one wave stores"""
    LH, RH, lpl = (Lp // 2, Lp // 2 - 1, 4 if f64 else 8) if syn else (Lp // 2 - 1, Lp // 2, 4 if f64 else 8)
    GL, GR = (LH * ew + 3) // 4, (RH * ew + 3) // 4
    return 4 * (64 - GL - GR) if nlev == 1 else 4 * ((64 - nlev * (GL + GR)) // lpl * lpl)


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def cascade_waves(n1s, n2, K, WX, nlev, Lp, inverse, force):
    """cascade2_launch: one round of 8 (synthesis: 4) waves per CU shared by the items, equal chunks of at least nlev (Lp - 1) rows"""
    ntx = cdiv(n1s, WX)
    chunks = max(1, (cus() * (4 if inverse else 8)) // (ntx * K))
    yc = max(cdiv(n2, chunks), nlev * (Lp - 1))
    yc = min(force or yc, n2)
    ychunk = cdiv(n2, cdiv(n2, yc))
    return ntx * cdiv(n2, ychunk) * K


def fused2_waves(n1s, n2, K, WX, Lp, target, force):
    """csrc/ndwt_geom.h: fused2_geometry"""
    per_chunk = cdiv(n1s, WX) * K
    yc = cdiv(n2, max(1, cdiv(target, per_chunk)))
    min_chunk = max(4 * (Lp - 1), 8)
    if per_chunk * cdiv(n2, min_chunk) < target // 2:
        min_chunk = 2
    yc = min(max(yc, min_chunk), n2)
    if force:
        yc = min(force, n2)
    return per_chunk * cdiv(n2, yc)


def R(rid, kind, wn, level, dims, K=3, vf=0, vi=0, force=0, layout="packed", dilation="reference", expect="cascade", denoise=False):
    return pytest.param(dict(kind=kind, wn=wn, level=level, dims=dims, K=K, vf=vf, vi=vi, force=force, layout=layout, dilation=dilation,
                             expect=expect, denoise=denoise), id=rid)


WAVELETS_2D = [("db4", 3), ("db2", 2), ("db3", 3)]
# dims None: n1 comp = WX + 32 of the row's analysis cascade (two tiles, the second anchored and wrapping), 40 rows
CASCADE_ROWS = [R(f"{k}-{wn}x{lev}-{'chunks-of-21' if force else 'default-chunks'}", k, wn, lev, None, vf=11, vi=11, force=force,
                  denoise=(wn == "db4" and force == 21))
                for k in KINDS for wn, lev in WAVELETS_2D for force in (21, 0)]
PER_LEVEL_ROWS = [R(f"{k}-{wn}x{lev}-per-level", k, wn, lev, None, vf=9, vi=9, expect="fused2") for k in KINDS for wn, lev in WAVELETS_2D]
PER_LEVEL_ROWS += [R("f32-ragged-37x21", "f32", "db2", 2, (37, 21), vf=9, vi=9, expect="fused2", denoise=True),
                   R("f64-ragged-37x21", "f64", "db3", 2, (37, 21), vf=9, vi=9, expect="fused2"),
                   R("f32-db6-40-rows", "f32", "db6", 2, (256, 40), vf=9, vi=9, expect="fused2"),          # Inv2S: items of fewer than 64 rows
                   R("f32-db6-64-rows", "f32", "db6", 2, (256, 64), vf=9, vi=9, expect="fused2"),          # Inv2P
                   R("f32-default-variants", "f32", "db4", 3, None, expect="fused2")]                      # nothing asked: no cascade on a stack
VOLUME_ROWS = [R("f32-db4x2-volumes", "f32", "db4", 2, (24, 20, 18), force=9, expect="fused3", denoise=True),
               R("f64-db2x2-volumes", "f64", "db2", 2, (24, 20, 18), force=9, expect="fused3"),
               R("c64-db4x2-volumes", "c64", "db4", 2, (24, 20, 18), force=9, expect="fused3"),
               R("c128-db2x1-volumes", "c128", "db2", 1, (24, 20, 18), force=9, expect="fused3"),
               R("f32-db4x2-stack-of-one", "f32", "db4", 2, (24, 20, 18), K=1, force=9, expect="fused3")]
FALLBACK_ROWS = [R("f32-atrous", "f32", "db2", 3, (64, 40), vf=11, vi=11, dilation="atrous", expect="fallback", denoise=True),
                 R("f64-db9", "f64", "db9", 2, (64, 40), vf=11, vi=11, expect="fallback"),
                 R("f32-offset", "f32", "db4", 3, None, vf=11, vi=11, layout="offset", expect="fallback"),
                 R("c128-offset", "c128", "db2", 2, None, vf=11, vi=11, layout="offset", expect="fallback"),
                 R("f32-bad-pitch", "f32", "db4", 3, None, vf=11, vi=11, layout="badpitch", expect="fallback"),
                 R("c64-bad-pitch", "c64", "db2", 2, None, vf=11, vi=11, layout="badpitch", expect="fallback")]
PITCH_ROWS = [R("f32-db4x3-pitched", "f32", "db4", 3, None, vf=11, vi=11, layout="pitch"),
              R("c128-db3x3-pitched", "c128", "db3", 3, None, vf=11, vi=11, layout="pitch", denoise=True),
              R("c64-db4x3-one-item", "c64", "db4", 3, None, K=1, vf=11, vi=11, denoise=True),
              R("f64-db4x3-denoise", "f64", "db4", 3, None, vf=11, vi=11, denoise=True)]


def _np_shrink(c, t):
    m = np.abs(c)
    out = c * np.where(m > t, (m - t) / np.where(m > 0, m, 1.0), 0.0)
    out[..., 0] = c[..., 0]
    return out


class _Buf:
    GUARD, FRONT = 8, 64

    def __init__(self, n, tdt, off):
        # FRONT elements of guard before the buffer (256 bytes and more: the view keeps the alignment of the allocation, so the rows
        # that are to take aligned and nontemporal stores take them) and at least GUARD - 1 after it
        self.t = torch.zeros(self.FRONT + n + self.GUARD, dtype=tdt, device="cuda")
        self.off = self.FRONT + off
        self.n, self.view = n, self.t[self.off:self.off + n]
        assert self.t.data_ptr() % 256 == 0 and self.off >= self.FRONT and self.t.numel() - (self.off + n) >= self.GUARD - 1

    def ptr(self):
        return self.view.data_ptr()

    def clean_outside(self, written=None):
        """nothing but zeros before the buffer, after it and -- `written`: [(start, stop)] -- between the runs that were to be written"""
        ok = float(self.t[:self.off].abs().sum()) == 0 and float(self.t[self.off + self.n:].abs().sum()) == 0
        if written:
            edges = [0] + [e for run in written for e in run] + [self.n]
            for a, b in zip(edges[0::2], edges[1::2]):
                ok = ok and (a == b or float(self.view[a:b].abs().sum()) == 0)
        return ok


def run_row(rid, row):
    kind, wn, level, K, dil, expect = row["kind"], row["wn"], row["level"], row["K"], row["dilation"], row["expect"]
    prec, cplx = KINDS[kind]
    Lp, tol, comp, f64 = 2 * int(wn[2:]), TOL[prec], 2 if cplx else 1, prec == "double"
    rdt = torch.float32 if prec == "single" else torch.float64
    ndt = (np.complex64 if prec == "single" else np.complex128) if cplx else (np.float32 if prec == "single" else np.float64)
    tdt = (torch.complex64 if prec == "single" else torch.complex128) if cplx else rdt
    T = "double" if f64 else "float"
    first = min(level, 3)
    dims = row["dims"] or ((wave_row_width(False, Lp, comp, f64, first) + 32) // comp, 40)
    k = len(dims)
    n1s, n2 = dims[0] * comp, dims[1]
    item = int(np.prod(dims))
    vol, nb = item * K, int(ndwt.num_bands(k, level))
    force, off = row["force"], (1 if row["layout"] == "offset" else 0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(zlib.crc32(repr((rid, dims, K, wn, level)).encode()))
    wns = [wn] * k

    def stack_plan():
        p = ndwt.Plan(list(dims) + [K], wns + [None], rdt, cplx, True, dil, max_level=level, axes=tuple(range(k)))
        p.set_variant(fwd=row["vf"], inv=row["vi"])
        p.set_tuning(0, force)
        return p

    def item_plan():
        p = ndwt.Plan(list(dims), wns, rdt, cplx, True, dil, max_level=level)
        p.set_variant(fwd=row["vf"], inv=row["vi"])
        p.set_tuning(0, force)
        return p

    ps, pu = stack_plan(), item_plan()
    want_desc = {"cascade": "stack2d cascade", "fused2": "stack2d fused", "fused3": "stack3d fused"}.get(expect)
    if expect == "fallback" and Lp > 16:
        want_desc = "stack axis"
    if want_desc:
        assert ps.describe() == want_desc, (rid, ps.describe())
    if row["layout"] == "pitch":
        pitch = ps.band_pitch()
        assert pitch == vol + 256 // (comp * (8 if f64 else 4))                    # prod(dims) plus the usual skew
    elif row["layout"] == "badpitch":
        pitch = vol + (1 if (vol * comp) % 4 == 0 and comp == 1 else 0) + (1 if comp == 2 else 0)
        assert (pitch * comp) % 4 != 0
    else:
        pitch = vol
    bp = 0 if pitch == vol else pitch
    bands = [(b * pitch, b * pitch + vol) for b in range(nb)]
    shape = tuple(dims) + (K,)

    def to_dev(a, n_bands=None, p=pitch, o=off):
        if n_bands is None:
            b = _Buf(a.size, tdt, o)
            b.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(a)).astype(ndt).reshape(-1)).cuda())
            return b
        ck = np.ascontiguousarray(np.transpose(a)).astype(ndt).reshape(n_bands, -1)
        v = ck.shape[1]
        b = _Buf((n_bands - 1) * p + v, tdt, o)
        for i in range(n_bands):
            b.view[i * p:i * p + v] = torch.from_numpy(ck[i]).cuda()
        return b

    def coef(b):
        ck = torch.stack([b.view[i * pitch:i * pitch + vol] for i in range(nb)]).cpu().numpy().reshape((nb, K) + tuple(reversed(dims)))
        return np.transpose(ck)                                                     # [dims, K, bands]

    def items(b):
        return np.transpose(b.view.cpu().numpy().reshape((K,) + tuple(reversed(dims))))   # [dims, K]

    def per_item(f, a):
        return np.stack([f(a[(slice(None),) * k + (j,)]) for j in range(K)], axis=k)

    def raw(b):
        return b.view.view(rdt) if cplx else b.view

    def check_launches(recs, inverse, what):
        fams = [r.family for r in recs]
        if expect == "fallback":
            assert recs and not any(f in CASCADE for f in fams), f"{what}: a cascade ran: {recs}"
            assert all(f in PER_AXIS + ONE_LEVEL_2D + FUSED_3D for f in fams), f"{what}: {recs}"
            if dil == "atrous":
                assert all(r.family in PER_AXIS for r in recs[(1 if not inverse else 0):(None if not inverse else -1)]), f"{what}: a dilated level ran a fused form: {recs}"
            if Lp > 16:
                assert all(f in PER_AXIS for f in fams), f"{what}: {recs}"
            return
        if expect == "fused3":
            assert len(recs) == level and all(f in FUSED_3D for f in fams), f"{what}: {recs}"
            for r in recs:
                assert r.params["T"] == T and r.params["L"] == Lp and r.params["EW"] == comp, f"{what}: {r!r}"
                one = cdiv(n1s, r.params["TX"]) * cdiv(n2, r.params["TY"]) * cdiv(dims[2], force)
                assert cdiv(dims[2], force) >= 2 and r.grid == (one * K, 1, 1), f"{what}: {r!r}, expected {one} workgroups x {K} items"
            return
        fam_c = "Inv2C" if inverse else "Fwd2C"
        split, left = [], level
        if expect == "cascade":
            top = INV_TOP.get((kind, Lp), 3) if inverse else 3
            while left >= 2:
                split.append(min(left, top))
                left -= split[-1]
        assert len(recs) == len(split) + left, f"{what}: {recs}"
        cas = recs[:len(split)]
        for r, nl in zip(cas, split):
            assert (r.family, r.params["T"], r.params["L"], r.params["NLEV"], r.params["EW"]) == (fam_c, T, Lp, nl, comp), f"{what}: {r!r}"
            waves = cascade_waves(n1s, n2, K, wave_row_width(inverse, Lp, comp, f64, nl), nl, Lp, inverse, force)
            assert r.grid == (waves, 1, 1) and r.block == (64, 1, 1), f"{what}: {r!r}, expected {waves} waves"
        for r in recs[len(split):]:
            assert r.family in ONE_LEVEL_2D and (r.family != "Fwd2S") == inverse, f"{what}: {r!r}"
            assert r.params["T"] == T and r.params["L"] == Lp and r.params.get("EW", 1) == comp, f"{what}: {r!r}"
            vec4 = n1s % 4 == 0
            assert r.params.get("VEC4", True) == vec4, f"{what}: {r!r}"
            target = 1024 if r.family == "Inv2P" else 2048
            waves = fused2_waves(n1s, n2, K, wave_row_width(inverse, Lp, comp, f64, 1), Lp, target, force)
            assert r.grid == (waves, 1, 1) and r.block == (64, 1, 1), f"{what}: {r!r}, expected {waves} waves"
        if rid == "f32-db6-64-rows" and inverse:
            assert all(r.family == "Inv2P" for r in recs), recs
        if rid == "f32-db6-40-rows" and inverse:
            assert all(r.family == "Inv2S" for r in recs), recs

    x = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
    x = x.astype(ndt).astype(np.complex128 if cplx else np.float64)
    xb = to_dev(x)
    # ---- dec: trace, the oracle item by item, guards
    want = per_item(lambda v: orc_c.spatial_dec(v, wns, level, 1, dil), x)
    yb = _Buf((nb - 1) * pitch + vol, tdt, off)
    with ndwt.kernel_trace() as recs:
        ps.dec(xb.ptr(), yb.ptr(), level, stream, band_pitch=bp)
    torch.cuda.synchronize()
    check_launches(recs, False, f"dec {rid}")
    got = coef(yb)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{rid}: items of {dims} x {K}, dec error {err:.3g} (bound {tol:.3g})")
    assert np.isfinite(got).all() and err <= tol, (rid, "dec", err)
    assert yb.clean_outside(bands), f"{rid}: dec wrote outside its bands"
    # ---- bits: item j on an unbatched plan pinned to the same variants (and given the same pointer offset)
    for j in range(K):
        xj = to_dev(x[(slice(None),) * k + (j,)])
        yj = _Buf(nb * item, tdt, off)
        pu.dec(xj.ptr(), yj.ptr(), level, stream)
        torch.cuda.synchronize()
        for b in range(nb):
            s = yb.view[b * pitch + j * item:b * pitch + (j + 1) * item]
            assert torch.equal(s.view(rdt) if cplx else s, raw(yj)[b * item * comp:(b + 1) * item * comp]), f"{rid}: dec of item {j}, band {b} differs from the unbatched plan"
    # ---- rec of random coefficients
    c = rng.standard_normal(want.shape) + (1j * rng.standard_normal(want.shape) if cplx else 0)
    c = c.astype(ndt).astype(want.dtype)
    want_r = per_item(lambda v: orc_c.spatial_rec(v, wns, 1, dil), c)
    scale = max(np.abs(want_r).max(), np.abs(c).max())
    cb = to_dev(c, nb)
    rb = _Buf(vol, tdt, off)
    with ndwt.kernel_trace() as recs:
        ps.rec(cb.ptr(), rb.ptr(), level, stream, band_pitch=bp)
    torch.cuda.synchronize()
    check_launches(recs, True, f"rec {rid}")
    got_r = items(rb)
    err = np.abs(got_r - want_r).max() / scale
    same = True
    for j in range(K):
        cj = to_dev(c[(slice(None),) * k + (j,)], nb, p=item)
        rj = _Buf(item, tdt, off)
        pu.rec(cj.ptr(), rj.ptr(), level, stream)
        torch.cuda.synchronize()
        dj = np.abs(np.transpose(rj.view.cpu().numpy().reshape(tuple(reversed(dims)))) - got_r[(slice(None),) * k + (j,)]).max() / scale
        assert dj <= 2 * tol, (rid, "rec against the unbatched plan", j, dj)
        same = same and torch.equal(raw(rj), raw(rb)[j * item * comp:(j + 1) * item * comp])
    print(f"{rid}: rec error {err:.3g} (bound {2 * tol:.3g}); bit-identical to the unbatched plan: {same}")
    assert np.isfinite(got_r).all() and err <= 2 * tol, (rid, "rec", err)
    assert rb.clean_outside(), f"{rid}: rec wrote outside its output"
    # ---- round trip
    r2 = _Buf(vol, tdt, off)
    ps.rec(yb.ptr(), r2.ptr(), level, stream, band_pitch=bp)
    torch.cuda.synchronize()
    err = np.abs(items(r2) - x).max() / np.abs(x).max()
    assert err <= 20 * tol, (rid, "round trip", err)
    # ---- isolation: item 1 is NaN; items 0 and 2 come out as in the clean run
    if K >= 3:
        xn = x.copy()
        xn[(slice(None),) * k + (1,)] = np.nan
        xnb, ynb = to_dev(xn), _Buf((nb - 1) * pitch + vol, tdt, off)
        ps.dec(xnb.ptr(), ynb.ptr(), level, stream, band_pitch=bp)
        cn = c.copy()
        cn[(slice(None),) * k + (1,)] = np.nan
        cnb, rnb = to_dev(cn, nb), _Buf(vol, tdt, off)
        ps.rec(cnb.ptr(), rnb.ptr(), level, stream, band_pitch=bp)
        torch.cuda.synchronize()
        for j in (0, 2):
            for b in range(nb):
                lo, hi = (b * pitch + j * item) * comp, (b * pitch + (j + 1) * item) * comp
                assert torch.equal(raw(ynb)[lo:hi], raw(yb)[lo:hi]), f"{rid}: NaN in item 1 changed item {j} of band {b} (dec)"
            assert torch.equal(raw(rnb)[j * item * comp:(j + 1) * item * comp], raw(rb)[j * item * comp:(j + 1) * item * comp]), f"{rid}: NaN in item 1 changed item {j} (rec)"
        assert bool(torch.isnan(raw(ynb)[item * comp:2 * item * comp]).any()) and bool(torch.isnan(raw(rnb)[item * comp:2 * item * comp]).any())
        assert ynb.clean_outside(bands) and rnb.clean_outside()
    if not row["denoise"]:
        return
    # ---- shrink and denoise (soft): numpy dec -> shrink -> rec of the oracle, band 0 kept, the magnitude shrunk for complex kinds
    thr = float(np.median(np.abs(want[..., 1:])))
    sb = to_dev(want, nb)
    with ndwt.kernel_trace() as recs:
        ps.shrink(sb.ptr(), level, thr, False, stream, band_pitch=bp)
    torch.cuda.synchronize()
    assert recs and all(r.family == "shrink_kernel" for r in recs), recs
    ws = _np_shrink(want.astype(ndt).astype(want.dtype), thr)
    assert np.abs(coef(sb) - ws).max() / np.abs(want).max() <= 20 * tol, (rid, "shrink")
    assert sb.clean_outside(bands)
    ob = _Buf(vol, tdt, off)
    with ndwt.kernel_trace() as recs:
        ps.denoise(xb.ptr(), ob.ptr(), level, thr, False, stream)
    torch.cuda.synchronize()
    assert recs and "Den3" not in [r.family for r in recs], f"denoise {rid}: {recs}"
    want_x = per_item(lambda v: orc_c.spatial_rec(v, wns, 1, dil), _np_shrink(want, thr))
    err = np.abs(items(ob) - want_x).max() / max(np.abs(want_x).max(), 1.0)
    print(f"{rid}: soft denoise error {err:.3g} (bound {20 * tol:.3g})")
    assert err <= 20 * tol, (rid, "soft denoise against the oracle", err)
    assert ob.clean_outside()


@pytest.mark.parametrize("row", CASCADE_ROWS + PITCH_ROWS)
def test_stack_of_images_cascades(row, request):
    run_row(request.node.callspec.id, row)


@pytest.mark.parametrize("row", PER_LEVEL_ROWS)
def test_stack_of_images_one_launch_per_level(row, request):
    run_row(request.node.callspec.id, row)


@pytest.mark.parametrize("row", VOLUME_ROWS)
def test_stack_of_volumes(row, request):
    run_row(request.node.callspec.id, row)


@pytest.mark.parametrize("row", FALLBACK_ROWS)
def test_fallback_row_runs_no_cascade(row, request):
    run_row(request.node.callspec.id, row)


def test_a_large_stack_takes_the_cascade_unasked_where_it_was_measured_to_win():
    """256 float images of 512 x 128 = 64 MiB, db4, 3 levels, no variant set: the analysis is one Fwd2C launch -- items of
    128 rows and more --, the synthesis stays one launch per level below 256 rows; both equal the plan with the cascade off bit for bit
    (dec) / to the tolerance (rec).  One item fewer is below the bytes: no cascade."""
    n1, n2, K, level = 512, 128, 256, 3
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.randn(K * n2 * n1, dtype=torch.float32, device="cuda")
    out = {}
    for name, v, items in (("default", 0, K), ("off", 9, K), ("fewer", 0, K - 1)):
        p = ndwt.Plan([n1, n2, items], ["db4", "db4", None], torch.float32, False, True, max_level=level, axes=(0, 1))
        p.set_variant(fwd=v, inv=v)
        y = torch.empty(10 * items * n2 * n1, dtype=torch.float32, device="cuda")
        r = torch.empty(items * n2 * n1, dtype=torch.float32, device="cuda")
        with ndwt.kernel_trace() as recs:
            p.dec(x.data_ptr(), y.data_ptr(), level, stream)
            p.rec(y.data_ptr(), r.data_ptr(), level, stream)
        torch.cuda.synchronize()
        out[name] = ([rc.family for rc in recs], y, r, p.describe(), recs)
    fams, y, r, desc, recs = out["default"]
    assert fams[0] == "Fwd2C" and len(fams) == 1 + level and all(f in ("Inv2S", "Inv2P") for f in fams[1:]), recs
    assert desc == "stack2d cascade" and recs[0].params["NLEV"] == 3
    assert recs[0].grid == (cascade_waves(n1, n2, K, wave_row_width(False, 8, 1, False, 3), 3, 8, False, 0), 1, 1), recs[0]
    assert not any(f in CASCADE for f in out["off"][0]) and not any(f in CASCADE for f in out["fewer"][0]), (out["off"][0], out["fewer"][0])
    assert out["fewer"][3] == "stack2d fused"
    assert torch.equal(y, out["off"][1])
    assert float((r - out["off"][2]).abs().max()) <= 2 * TOL["single"] * float(x.abs().max())
    assert float((r - x).abs().max()) <= 20 * TOL["single"] * float(x.abs().max())


def test_describe_names_the_stack_route():
    def desc(dims, wn, dt=torch.float32, k=2, dilation="reference", vf=0, vi=0):
        p = ndwt.Plan(dims, [wn] * k + [None] * (len(dims) - k), dt, dilation=dilation, max_level=3, axes=tuple(range(k)))
        p.set_variant(fwd=vf, inv=vi)
        return p.describe()
    assert desc([64, 40, 3], "db4") == "stack2d fused"
    assert desc([64, 40, 3], "db4", vf=11, vi=11) == "stack2d cascade"
    assert desc([66, 40, 3], "db4", vf=11, vi=11) == "stack2d fused"              # rows that are no whole groups of 4
    assert desc([64, 40, 3], "db9", torch.float64) == "stack axis"
    assert desc([24, 20, 18, 3], "db4", k=3) == "stack3d fused"
    assert desc([64, 3], "db4", k=1) == "batched1d cascade"                       # k = 1 is the batched 1-D plan
    assert desc([64, 40], "db4", k=2) == "fused2d" and desc([24, 20, 18], "db4", k=3) == "fused3d"   # k = ndim is ndwt_plan_create


def test_refused_entry_points_say_so():
    """whatever sizes a buffer by one array's dimensions refuses a stack plan: NDWT_ERR_UNSUPPORTED with a message, nothing launched"""
    lib = ndwt.lib()
    for dims, k in (([64, 40, 3], 2), ([24, 20, 18, 3], 3)):
        p = ndwt.Plan(dims, ["db2"] * k + [None], torch.float64, max_level=2, axes=tuple(range(k)))
        h = p._h
        n = int(np.prod(dims)) * 16
        host = np.zeros(n)
        hp = host.ctypes.data_as(ctypes.c_void_p)
        dev = torch.zeros(n, dtype=torch.float64, device="cuda")
        dp = ctypes.c_void_p(dev.data_ptr())
        pp = (ctypes.c_void_p * 16)(*[dev.data_ptr()] * 16)
        i64 = (ctypes.c_int64 * 8)(*[1] * 8)
        coef = ctypes.c_void_p(None)
        calls = {
            "ndwt_dec_host": lambda: lib.ndwt_dec_host(h, hp, hp, 1),
            "ndwt_rec_host": lambda: lib.ndwt_rec_host(h, hp, hp, 1),
            "ndwt_denoise_host": lambda: lib.ndwt_denoise_host(h, hp, hp, 1, 0.1, 0),
            "ndwt_dec_split_host": lambda: lib.ndwt_dec_split_host(h, hp, None, hp, None, 1),
            "ndwt_rec_split_host": lambda: lib.ndwt_rec_split_host(h, hp, None, hp, None, 1),
            "ndwt_coef_create": lambda: lib.ndwt_coef_create(h, 1, ctypes.byref(coef)),
            "ndwt_coef_dec_host": lambda: lib.ndwt_coef_dec_host(h, hp, 1, ctypes.byref(coef)),
            "ndwt_coef_put_host": lambda: lib.ndwt_coef_put_host(h, 1, hp, ctypes.byref(coef)),
            "ndwt_coef_rec_host": lambda: lib.ndwt_coef_rec_host(h, None, hp),
            "ndwt_coef_shrink": lambda: lib.ndwt_coef_shrink(h, None, 0.1, 0),
            "ndwt_coef_get_host": lambda: lib.ndwt_coef_get_host(h, None, hp),
            "ndwt_analysis_level_slab": lambda: lib.ndwt_analysis_level_slab(h, dp, pp, 1, None),
            "ndwt_synthesis_level_slab": lambda: lib.ndwt_synthesis_level_slab(h, pp, dp, 1, None),
            "ndwt_analysis_level_slab_split": lambda: lib.ndwt_analysis_level_slab_split(h, dp, dp, dp, pp, 1, None),
            "ndwt_synthesis_level_slab_ext": lambda: lib.ndwt_synthesis_level_slab_ext(h, pp, dp, 1, None),
            "ndwt_analysis_level_slab_part": lambda: lib.ndwt_analysis_level_slab_part(h, dp, dp, dp, pp, 1, 1, None),
            "ndwt_synthesis_level_slab_part": lambda: lib.ndwt_synthesis_level_slab_part(h, pp, 1, 0, 1, dp, 1, None),
            "ndwt_analysis_level_slab_runs": lambda: lib.ndwt_analysis_level_slab_runs(h, dp, pp, 1, 1, 1, 1, None),
            "ndwt_synthesis_level_slab_runs": lambda: lib.ndwt_synthesis_level_slab_runs(h, pp, 1, 0, 0, 1, 1, dp, 1, None),
            "ndwt_slab_segments": lambda: lib.ndwt_slab_segments(h, 0, 1, pp, pp, i64, None),
            "ndwt_slab_segments_strided": lambda: lib.ndwt_slab_segments_strided(h, 0, 1, pp, pp, i64, 1, i64, i64, None),
        }
        with ndwt.kernel_trace() as recs:
            for name, call in calls.items():
                rc = call()
                msg = lib.ndwt_last_error().decode()
                assert rc == 7 and "batched plan" in msg, (name, rc, msg)
        assert recs == [] and not coef.value
        assert lib.ndwt_plan_slab_fast(h) == 0


@pytest.mark.parametrize("dims,wn,level", [((64, 40), "db4", 2), ((24, 20, 18), "db2", 2)], ids=["images", "volumes"])
def test_split_complex_hooks_and_profiling_serve_a_stack(dims, wn, level):
    """the served entry points beside dec / rec: ndwt_dec_split / ndwt_rec_split (separate re / im arrays on a real plan), the generic path
    (ndwt_plan_set_path) and the profiling records -- against the oracle item by item, guards on both sides of every output"""
    K, k = 3, len(dims)
    item, tol = int(np.prod(dims)), TOL["double"]
    vol, nb = item * K, int(ndwt.num_bands(k, level))
    rng = np.random.default_rng(5)
    x = rng.standard_normal(tuple(dims) + (K,)) + 1j * rng.standard_normal(tuple(dims) + (K,))
    want = np.stack([orc_c.spatial_dec(x[(slice(None),) * k + (j,)], [wn] * k, level, 1) for j in range(K)], axis=k)
    stream = torch.cuda.current_stream().cuda_stream
    p = ndwt.Plan(list(dims) + [K], [wn] * k + [None], torch.float64, False, True, max_level=level, axes=tuple(range(k)))

    def dev(a):
        b = _Buf(a.size, torch.float64, 0)
        b.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(a)).reshape(-1)).cuda())
        return b

    def coef(b):
        return np.transpose(b.view.cpu().numpy().reshape((nb, K) + tuple(reversed(dims))))

    xr, xi = dev(x.real), dev(x.imag)
    for generic in (False, True):
        p.set_path(generic)
        p.set_profiling(True)
        yr, yi = _Buf(nb * vol, torch.float64, 0), _Buf(nb * vol, torch.float64, 0)
        for kind in range(4):
            p.get_profile(kind)                                                      # (reading a kind clears its records)
        with ndwt.kernel_trace() as recs:
            p.dec_split(xr.ptr(), xi.ptr(), yr.ptr(), yi.ptr(), level, stream)
        torch.cuda.synchronize()
        fams = {r.family for r in recs}
        assert fams <= (set(PER_AXIS) if generic else set(ONE_LEVEL_2D + FUSED_3D)), recs
        launches = sum(p.get_profile(kind)[1] for kind in range(4))
        assert launches == len(recs) and launches >= 2 * level, (launches, recs)
        got = coef(yr) + 1j * coef(yi)
        assert np.abs(got - want).max() <= tol * np.abs(want).max(), generic
        assert yr.clean_outside() and yi.clean_outside()
        or_, oi = _Buf(vol, torch.float64, 0), _Buf(vol, torch.float64, 0)
        p.rec_split(yr.ptr(), yi.ptr(), or_.ptr(), oi.ptr(), level, stream)
        torch.cuda.synchronize()
        back = np.transpose((or_.view + 1j * oi.view).cpu().numpy().reshape((K,) + tuple(reversed(dims))))
        assert np.abs(back - x).max() <= 20 * tol * np.abs(x).max(), generic
        assert or_.clean_outside() and oi.clean_outside()
        yr2 = _Buf(nb * vol, torch.float64, 0)
        p.dec_split(xr.ptr(), None, yr2.ptr(), None, level, stream)                 # real data: the imaginary pair left out
        torch.cuda.synchronize()
        assert torch.equal(yr2.view, yr.view)
        p.set_profiling(False)


def test_the_class_takes_a_stack():
    """nd_dwt_2D(wname, [n1, n2], 'stack', K): [n1, n2, K] in, [n1, n2, K, bands] out, numpy and device tensors, equal to K calls"""
    n1, n2, K, level = 64, 40, 3, 2
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n1, n2, K))
    one = ndwt.nd_dwt_2D("db4", [n1, n2], "pres_l2_norm", 1)
    ws = ndwt.nd_dwt_2D("db4", [n1, n2], "stack", K, "pres_l2_norm", 1, "band_pitch", "auto")
    xg = torch.from_numpy(np.ascontiguousarray(np.transpose(x))).cuda().permute(2, 1, 0)      # (K, n2, n1) in memory
    each = torch.stack([one.dec(xg[:, :, j].contiguous(), level) for j in range(K)], dim=2)
    with ndwt.kernel_trace() as recs:
        y = ws.dec(xg, level)
    nb = 1 + 3 * level
    assert [r.family for r in recs] == ["Fwd2S"] * level and tuple(y.shape) == (n1, n2, K, nb) and tuple(each.shape) == (n1, n2, K, nb)
    assert y.permute(3, 2, 1, 0).stride(0) == n1 * n2 * K + 32                    # 'band_pitch', 'auto': prod(dims) + 256 bytes
    assert torch.equal(y, each)
    r = ws.rec(y)
    assert tuple(r.shape) == (n1, n2, K) and float((r - xg).abs().max()) <= 20 * TOL["double"] * float(xg.abs().max())
    r_each = torch.stack([one.rec(each[:, :, j, :].contiguous()) for j in range(K)], dim=2)
    assert float((r - r_each).abs().max()) <= 2 * TOL["double"] * float(y.abs().max())
    d = ws.denoise(xg, level, 0.5)
    d_each = torch.stack([one.denoise(xg[:, :, j].contiguous(), level, 0.5) for j in range(K)], dim=2)
    assert tuple(d.shape) == (n1, n2, K) and float((d - d_each).abs().max()) <= 4 * TOL["double"] * float(xg.abs().max())
    s = ws.shrink(y, 0.5, "hard")
    assert tuple(s.shape) == tuple(y.shape) and torch.equal(s[..., 0], y[..., 0]) and float(s[..., 1:].abs()[s[..., 1:] != 0].min()) > 0.5
    # host arrays (hip_off), single precision, complex; a stack of volumes
    wh = ndwt.nd_dwt_2D("db2", [n1, n2], "stack", K, "compute", "hip_off", "precision", "single", "pres_l2_norm", 1)
    xc = (x + 1j * rng.standard_normal((n1, n2, K))).astype(np.complex64)
    yh = wh.dec(xc, level)
    assert isinstance(yh, np.ndarray) and yh.shape == (n1, n2, K, nb) and yh.dtype == np.complex64
    want = np.stack([orc_c.spatial_dec(xc[:, :, j].astype(np.complex128), ["db2", "db2"], level, 1) for j in range(K)], axis=2)
    assert np.abs(yh - want).max() <= TOL["single"] * np.abs(want).max()
    rh = wh.rec(yh)
    assert rh.shape == (n1, n2, K) and np.abs(rh - xc).max() <= 20 * TOL["single"] * np.abs(xc).max()
    wv = ndwt.nd_dwt_3D("db2", [24, 20, 18], "stack", 2, "compute", "hip_off", "pres_l2_norm", 1)
    xv = rng.standard_normal((24, 20, 18, 2))
    yv = wv.dec(xv, 1)
    want = np.stack([orc_c.spatial_dec(xv[..., j], ["db2"] * 3, 1, 1) for j in range(2)], axis=3)
    assert yv.shape == (24, 20, 18, 2, 8) and np.abs(yv - want).max() <= TOL["double"] * np.abs(want).max()
    assert np.abs(wv.rec(yv) - xv).max() <= 20 * TOL["double"] * np.abs(xv).max()
    with pytest.raises(ValueError, match="does not match"):
        ws.dec(xg[:, :, :2], level)


def test_an_unbatched_image_runs_what_it_always_ran():
    """ndwt_plan_create is untouched: 4096 x 2048 float, db4, 3 levels traces the launches and grids of the build before there were stacks
    (cascade2_launch on 256 CUs: 19 tiles x 98 chunks of 21 rows, 19 x 53 chunks of 39 rows)"""
    if cus() != 256:
        pytest.skip("the grids written down here are those of 256 CUs")
    p = ndwt.Plan([4096, 2048], ["db4", "db4"], torch.float32, max_level=3)
    assert p.describe() == "fused2d"
    x = torch.randn(4096 * 2048, dtype=torch.float32, device="cuda")
    y = torch.empty(10 * x.numel(), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    with ndwt.kernel_trace() as recs:
        p.dec(x.data_ptr(), y.data_ptr(), 3, stream)
        p.rec(y.data_ptr(), x.data_ptr(), 3, stream)
    torch.cuda.synchronize()
    got = [(r.family, r.params["T"], r.params["L"], r.params["NLEV"], r.params["EW"], r.grid, r.block) for r in recs]
    assert got == [("Fwd2C", "float", 8, 3, 1, (19 * 98, 1, 1), (64, 1, 1)), ("Inv2C", "float", 8, 3, 1, (19 * 53, 1, 1), (64, 1, 1))], recs
    assert recs[1].params["PD"] == 1
