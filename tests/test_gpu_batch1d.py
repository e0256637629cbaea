"""Batched 1-D plans (ndwt_plan_create_many): many signals per call, two to four levels per launch (Fwd1C / Inv1C, csrc/ndwt_device_1d.h).

Every row runs a few signals of a few hundred samples and checks, for dec, rec of random coefficients and the round trip:

  * the launch trace: Fwd1C / Inv1C with the row's T, L, NLEV, EW in the split 4, 3, 2 then one launch per level, each on a grid of
    ceil(K nseg / 4) workgroups of 256 threads;
  * the fp64 oracle (oracle/ndwt_spatial.c), signal by signal, within TOL of tests/test_gpu_parity.py (dec) and 2 TOL max(|want|, |c|) (rec);
  * one launch per level (variant 9): dec bit for bit; rec within 2 TOL (whether it is bit-identical is printed);
  * guard elements before and after every output.

Fallback rows (odd n, an offset pointer, a pitch that breaks the 4-scalar alignment, db5, a-trous dilation, variant 9) must run one
per-axis launch per level and still agree with the oracle.  The last test is the coverage gate over the 96 instances of the table.
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
CASCADE = ("Fwd1C", "Inv1C")
PER_AXIS = ("AxisX", "AxisMarch", "axis_analysis_kernel", "axis_synthesis_kernel")
# the instance table (csrc/ndwt_fused_list.h: NDWT_LIST_*1C): (family, T, EW, L, NLEV)
INSTANCES = {(fam, T, ew, L, nlev) for fam in CASCADE for T in ("float", "double") for ew in (1, 2) for L in (2, 4, 6, 8) for nlev in (2, 3, 4)}


def tile_width(kind, L, nlev):
    """Fwd1C::WX = Inv1C::WX (the two halves of the filter swap sides): the lanes valid at every level, in whole 128-byte lines"""
    prec, cplx = KINDS[kind]
    ew, lpl = (2 if cplx else 1), (8 if prec == "single" else 4)
    return 4 * ((64 - nlev * (((L // 2 - 1) * ew + 3) // 4 + ((L // 2) * ew + 3) // 4)) // lpl * lpl)


def split(level):
    """launches of a `level`-level transform: cascades of 4, 3, 2 levels, then one launch per level"""
    out, left = [], level
    while left >= 2:
        out.append(min(left, 4))
        left -= out[-1]
    return out, left


def R(rid, kind, wn, level, K=3, row=None, layout="packed", dilation="reference", variant=None, denoise=False, fallback=False):
    return pytest.param(dict(kind=kind, wn=wn, level=level, K=K, row=row, layout=layout, dilation=dilation, variant=variant, denoise=denoise,
                             fallback=fallback), id=rid)


# row = scalars per signal (n comp); None: WX + 32 of the row's first cascade -- two segments, the second partial and wrapping
ROWS = [R(f"{k}-db{L // 2}-l{lev}", k, f"db{L // 2}", lev, denoise=(L == 8 and lev == 3)) for k in KINDS for L in (2, 4, 6, 8) for lev in (2, 3, 4)]
MORE_ROWS = [R("f32-db4-l5", "f32", "db4", 5), R("c64-db2-l7", "c64", "db2", 7), R("f64-db3-l9", "f64", "db3", 9, denoise=True),
             R("f32-one-signal", "f32", "db4", 4, K=1), R("c128-one-signal", "c128", "db2", 3, K=1),
             R("f32-five-signals-one-segment", "f32", "db2", 3, K=5, row=96), R("f64-five-signals-one-segment", "f64", "db4", 2, K=5, row=128),
             R("f32-short-row-db4", "f32", "db4", 4, K=2, row=64, denoise=True), R("c64-short-row-db4", "c64", "db4", 3, K=2, row=64),
             R("f32-pitched", "f32", "db4", 4, layout="pitch", denoise=True), R("c128-pitched", "c128", "db3", 3, layout="pitch")]
FALLBACK_ROWS = [R("f32-n-1001", "f32", "db4", 3, row=1001, fallback=True), R("f64-n-1001", "f64", "db2", 2, row=1001, fallback=True),
                 R("f32-offset", "f32", "db4", 3, layout="offset", fallback=True), R("c128-offset", "c128", "db4", 3, layout="offset", fallback=True),
                 R("f32-bad-pitch", "f32", "db4", 3, layout="badpitch", fallback=True), R("c64-bad-pitch", "c64", "db2", 4, layout="badpitch", fallback=True),
                 R("f32-db5", "f32", "db5", 3, row=256, fallback=True), R("c64-db5", "c64", "db5", 2, row=256, fallback=True),
                 R("f32-atrous", "f32", "db2", 3, row=256, dilation="atrous", fallback=True, denoise=True),
                 R("f64-atrous", "f64", "db4", 3, row=256, dilation="atrous", fallback=True),
                 R("f32-variant-9", "f32", "db4", 4, variant=9, fallback=True), R("c128-variant-9", "c128", "db3", 3, variant=9, fallback=True)]


def _np_shrink(c, t, hard):
    m = np.abs(c)
    out = c * (np.where(m > t, 1.0, 0.0) if hard else np.where(m > t, (m - t) / np.where(m > 0, m, 1.0), 0.0))
    out[..., 0] = c[..., 0]
    return out


class _Buf:
    GUARD = 8

    def __init__(self, n, tdt, off):
        self.t = torch.zeros(n + self.GUARD, dtype=tdt, device="cuda")
        self.off, self.n, self.view = off, n, self.t[off:off + n]

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


_RECS = {}          # row id -> cascade launch records of a row that passed


def run_row(rid, row):
    kind, wn, level, K, dil = row["kind"], row["wn"], row["level"], row["K"], row["dilation"]
    prec, cplx = KINDS[kind]
    L, tol, comp = 2 * int(wn[2:]), TOL[prec], 2 if cplx else 1
    rdt = torch.float32 if prec == "single" else torch.float64
    ndt = (np.complex64 if prec == "single" else np.complex128) if cplx else (np.float32 if prec == "single" else np.float64)
    tdt = (torch.complex64 if prec == "single" else torch.complex128) if cplx else rdt
    T = "float" if prec == "single" else "double"
    casc, left = split(level)
    scal = row["row"] or tile_width(kind, min(L, 8), casc[0]) + 32
    n = scal // comp if scal % comp == 0 else scal             # (odd n: real kinds only)
    assert n * comp == scal or not cplx
    scal = n * comp
    rng = np.random.default_rng(zlib.crc32(repr((rid, n, K, wn, level)).encode()))
    x = rng.standard_normal((n, K)) + (1j * rng.standard_normal((n, K)) if cplx else 0)
    x = x.astype(ndt).astype(np.complex128 if cplx else np.float64)
    nb, vol = 1 + level, n * K
    off = 1 if row["layout"] == "offset" else 0
    fallback, vset = row["fallback"], row["variant"]
    stream = torch.cuda.current_stream().cuda_stream

    def plan(vf, vi):
        p = ndwt.Plan([n], [wn], rdt, cplx, True, dil, max_level=level, howmany=K)
        p.set_variant(fwd=vf, inv=vi)
        return p

    p9 = plan(9, 9)
    pc = plan(vset or 0, vset or 0)
    if row["layout"] == "pitch":
        pitch = pc.band_pitch()
        assert pitch == vol + 256 // (comp * (4 if prec == "single" else 8))       # howmany n plus the usual skew
    elif row["layout"] == "badpitch":
        pitch = vol + (1 if vol % 4 == 0 else 0) + (2 if vol % 4 in (1, 3) else 0)
        assert (pitch * comp) % 4 != 0
    else:
        pitch = vol
    bp = 0 if pitch == vol else pitch
    bands = [(k * pitch, k * pitch + vol) for k in range(nb)]

    def to_dev(a, n_bands=None):
        if n_bands is None:
            b = _Buf(vol, tdt, off)
            b.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(a)).astype(ndt).reshape(-1)).cuda())
            return b
        ck = np.ascontiguousarray(np.transpose(a)).astype(ndt).reshape(n_bands, vol)
        b = _Buf((n_bands - 1) * pitch + vol, tdt, off)
        for k in range(n_bands):
            b.view[k * pitch:k * pitch + vol] = torch.from_numpy(ck[k]).cuda()
        return b

    def coef(b):
        ck = torch.stack([b.view[k * pitch:k * pitch + vol] for k in range(nb)]).cpu().numpy().reshape(nb, K, n)
        return np.transpose(ck)

    def signals(b):
        return np.transpose(b.view.cpu().numpy().reshape(K, n))

    def per_signal(f, a):
        return np.stack([f(a[:, k]) for k in range(K)], axis=1)

    def check_launches(recs, inverse, what):
        fam = "Inv1C" if inverse else "Fwd1C"
        cas = [r for r in recs if r.family in CASCADE]
        if fallback:
            assert not cas and len(recs) == level and all(r.family in PER_AXIS for r in recs), f"{what}: expected one per-axis launch per level: {recs}"
            return []
        got = [(r.family, r.params["T"], r.params["L"], r.params["NLEV"], r.params["EW"]) for r in cas]
        assert got == [(fam, T, L, nl, comp) for nl in casc], f"{what}: cascade launches {cas}, expected {fam} x {casc}"
        assert len(recs) == len(casc) + left and all(r.family == "AxisX" for r in recs if r not in cas), f"{what}: {recs}"
        for r, nl in zip(cas, casc):
            nseg = -(-scal // tile_width(kind, L, nl))
            assert r.grid == (-(-K * nseg // 4), 1, 1) and r.block == (256, 1, 1), f"{what}: {r!r}, expected ceil({K} x {nseg} / 4) workgroups of 256"
            assert (r.family, T, comp, L, nl) in INSTANCES
        return cas

    launched = []
    xb = to_dev(x)
    # ---- dec: the oracle signal by signal, and bit for bit one launch per level
    want = per_signal(lambda v: orc_c.spatial_dec(v, [wn], level, 1, dil), x)
    y9, yb = _Buf((nb - 1) * pitch + vol, tdt, off), _Buf((nb - 1) * pitch + vol, tdt, off)
    p9.dec(xb.ptr(), y9.ptr(), level, stream, band_pitch=bp)
    with ndwt.kernel_trace() as recs:
        pc.dec(xb.ptr(), yb.ptr(), level, stream, band_pitch=bp)
    torch.cuda.synchronize()
    launched += check_launches(recs, False, f"dec {rid}")
    err = np.abs(coef(yb) - want).max() / np.abs(want).max()
    print(f"{rid}: n {n} x {K} signals, dec error {err:.3g} (bound {tol:.3g})")
    assert err <= tol, (rid, "dec", err)
    assert torch.equal(yb.view.view(rdt), y9.view.view(rdt)), f"{rid}: dec differs from one launch per level"
    assert yb.clean_outside(bands), f"{rid}: dec wrote outside its bands"
    # ---- rec of random coefficients
    c = rng.standard_normal(want.shape) + (1j * rng.standard_normal(want.shape) if cplx else 0)
    c = c.astype(ndt).astype(want.dtype)
    want_r = per_signal(lambda v: orc_c.spatial_rec(v, [wn], 1, dil), c)
    scale = max(np.abs(want_r).max(), np.abs(c).max())
    cb = to_dev(c, nb)
    r9, rb = _Buf(vol, tdt, off), _Buf(vol, tdt, off)
    p9.rec(cb.ptr(), r9.ptr(), level, stream, band_pitch=bp)
    with ndwt.kernel_trace() as recs:
        pc.rec(cb.ptr(), rb.ptr(), level, stream, band_pitch=bp)
    torch.cuda.synchronize()
    launched += check_launches(recs, True, f"rec {rid}")
    err, d9 = np.abs(signals(rb) - want_r).max() / scale, np.abs(signals(rb) - signals(r9)).max() / scale
    same = torch.equal(rb.view.view(rdt), r9.view.view(rdt))
    print(f"{rid}: rec error {err:.3g}, against one launch per level {d9:.3g} (bound {2 * tol:.3g}); bit-identical: {same}")
    assert err <= 2 * tol, (rid, "rec", err)
    assert d9 <= 2 * tol, (rid, "rec against per-level", d9)
    assert rb.clean_outside(), f"{rid}: rec wrote outside its output"
    # ---- round trip
    pc.rec(yb.ptr(), rb.ptr(), level, stream, band_pitch=bp)
    torch.cuda.synchronize()
    err = np.abs(signals(rb) - x).max() / np.abs(x).max()
    assert err <= 20 * tol, (rid, "round trip", err)
    if not row["denoise"]:
        return launched
    # ---- shrink and denoise, soft and hard: the oracle with the magnitude shrunk (complex: |re + i im|), and one launch per level
    thr = float(np.median(np.abs(want[..., 1:])))
    for hard in (False, True):
        sb = to_dev(want, nb)
        with ndwt.kernel_trace() as recs:
            pc.shrink(sb.ptr(), level, thr, hard, stream, band_pitch=bp)
        torch.cuda.synchronize()
        assert recs and all(r.family == "shrink_kernel" for r in recs), recs
        ws = _np_shrink(want.astype(ndt).astype(want.dtype), thr, hard)
        if not hard:                                          # (hard: a coefficient within rounding of the threshold may fall either side)
            assert np.abs(coef(sb) - ws).max() / np.abs(want).max() <= 20 * tol, (rid, "shrink")
        assert sb.clean_outside(bands)
        o9, ob = _Buf(vol, tdt, off), _Buf(vol, tdt, off)
        p9.denoise(xb.ptr(), o9.ptr(), level, thr, hard, stream)
        with ndwt.kernel_trace() as recs:
            pc.denoise(xb.ptr(), ob.ptr(), level, thr, hard, stream)
        torch.cuda.synchronize()
        fams = [r.family for r in recs]
        # (the coefficients of a denoise live in the plan's own scratch at its own pitch: a caller's layout does not reach them, only x's does)
        if not fallback:
            assert "shrink_kernel" in fams and "Fwd1C" in fams and "Inv1C" in fams, f"denoise {rid}: {recs}"      # no fused thresholding here
        want_x = per_signal(lambda v: orc_c.spatial_rec(v, [wn], 1, dil), _np_shrink(want, thr, hard))
        d9 = np.abs(signals(ob) - signals(o9)).max() / max(np.abs(signals(o9)).max(), 1.0)
        print(f"{rid}: {'hard' if hard else 'soft'} denoise against one launch per level {d9:.3g} (bound {4 * tol:.3g})")
        assert d9 <= 4 * tol, (rid, "denoise against per-level", hard, d9)
        if not hard:
            err = np.abs(signals(ob) - want_x).max() / max(np.abs(want_x).max(), 1.0)
            assert err <= 20 * tol, (rid, "soft denoise against the oracle", err)
        assert ob.clean_outside()
    return launched


def cascade_records(rid, row):
    if rid not in _RECS:
        _RECS[rid] = run_row(rid, row)
    return _RECS[rid]


@pytest.mark.parametrize("row", ROWS + MORE_ROWS)
def test_batched_row_cascades(row, request):
    assert cascade_records(request.node.callspec.id, row)


@pytest.mark.parametrize("row", FALLBACK_ROWS)
def test_fallback_row_runs_one_launch_per_level(row, request):
    assert run_row(request.node.callspec.id, row) == []


def test_an_unbatched_plan_runs_what_it_always_ran():
    """ndwt_plan_create is untouched: a 1-D plan, even asked for cascades (variant 11), traces AxisX only, one launch per level"""
    n, level = 512, 4
    stream = torch.cuda.current_stream().cuda_stream
    for rdt, cplx in ((torch.float32, False), (torch.float64, True)):
        p = ndwt.Plan([n], ["db4"], rdt, cplx, True, "reference", max_level=level)
        p.set_variant(fwd=11, inv=11)
        assert p.describe() == "axis"
        x = torch.randn(n * (2 if cplx else 1), dtype=rdt, device="cuda")
        y = torch.empty((1 + level) * x.numel(), dtype=rdt, device="cuda")
        with ndwt.kernel_trace() as recs:
            p.dec(x.data_ptr(), y.data_ptr(), level, stream)
            p.rec(y.data_ptr(), x.data_ptr(), level, stream)
        torch.cuda.synchronize()
        assert len(recs) == 2 * level and all(r.family == "AxisX" and r.params["VEC4"] is True for r in recs), recs


def test_describe_names_the_batched_route():
    assert ndwt.Plan([512], ["db4"], torch.float32, howmany=3).describe() == "batched1d cascade"
    assert ndwt.Plan([512], ["db5"], torch.float32, howmany=3).describe() == "batched1d axis"
    assert ndwt.Plan([512], ["db4"], torch.float32, dilation="atrous", howmany=3).describe() == "batched1d axis"


def test_refused_entry_points_say_so():
    """whatever sizes a buffer by one array's dimensions refuses a batched plan: NDWT_ERR_UNSUPPORTED with a message, nothing launched"""
    lib = ndwt.lib()
    p = ndwt.Plan([64], ["db2"], torch.float64, howmany=3, max_level=2)
    h = p._h
    host = np.zeros(3 * 64 * 4)
    hp = host.ctypes.data_as(ctypes.c_void_p)
    dev = torch.zeros(3 * 64 * 4, dtype=torch.float64, device="cuda")
    dp = ctypes.c_void_p(dev.data_ptr())
    pp = (ctypes.c_void_p * 8)(*[dev.data_ptr()] * 8)
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


def test_the_class_takes_a_batch():
    """nd_dwt_1D(wname, n, 'batch', K): [n, K] in, [n, K, bands] out, numpy and device tensors, equal to K calls on nd_dwt_1D(wname, n)"""
    n, K, level = 384, 4, 3
    rng = np.random.default_rng(7)
    x = rng.standard_normal((n, K))
    one = ndwt.nd_dwt_1D("db4", n, "pres_l2_norm", 1)
    wb = ndwt.nd_dwt_1D("db4", n, "batch", K, "pres_l2_norm", 1)
    xk = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()              # (K, n) contiguous: column k of xk.T is signal k, used where it lies
    xg = xk.T
    each = torch.stack([one.dec(xg[:, k].contiguous(), level) for k in range(K)], dim=1)
    with ndwt.kernel_trace() as recs:
        y = wb.dec(xg, level)
    assert [r.family for r in recs] == ["Fwd1C"] and tuple(y.shape) == (n, K, 1 + level) and tuple(each.shape) == (n, K, 1 + level)
    assert torch.equal(y, each)                                          # the cascade, K calls of AxisX: the same bits
    w9 = ndwt.nd_dwt_1D("db4", n, "batch", K, "pres_l2_norm", 1)
    w9._plan(False, level, torch.device("cuda", torch.cuda.current_device())).set_variant(fwd=9, inv=9)
    with ndwt.kernel_trace() as recs:
        y9 = w9.dec(xg, level)
    assert [r.family for r in recs] == ["AxisX"] * level and torch.equal(y9, each)
    r = wb.rec(y)
    assert tuple(r.shape) == (n, K) and float((r - xg).abs().max()) <= 20 * TOL["double"] * float(xg.abs().max())
    r_each = torch.stack([one.rec(y[:, k, :].contiguous()) for k in range(K)], dim=1)
    assert float((r - r_each).abs().max()) <= 2 * TOL["double"] * float(y.abs().max())
    d = wb.denoise(xg, level, 0.5)
    d_each = torch.stack([one.denoise(xg[:, k].contiguous(), level, 0.5) for k in range(K)], dim=1)
    assert tuple(d.shape) == (n, K) and float((d - d_each).abs().max()) <= 4 * TOL["double"] * float(xg.abs().max())
    s = wb.shrink(y, 0.5, "hard")
    assert tuple(s.shape) == tuple(y.shape) and torch.equal(s[..., 0], y[..., 0]) and float(s[..., 1:].abs()[s[..., 1:] != 0].min()) > 0.5
    # host arrays (hip_off), single precision, complex
    wh = ndwt.nd_dwt_1D("db2", n, "batch", K, "compute", "hip_off", "precision", "single", "pres_l2_norm", 1)
    xc = (x + 1j * rng.standard_normal((n, K))).astype(np.complex64)
    yh = wh.dec(xc, level)
    assert isinstance(yh, np.ndarray) and yh.shape == (n, K, 1 + level) and yh.dtype == np.complex64
    want = np.stack([orc_c.spatial_dec(xc[:, k].astype(np.complex128), ["db2"], level, 1) for k in range(K)], axis=1)
    assert np.abs(yh - want).max() <= TOL["single"] * np.abs(want).max()
    rh = wh.rec(yh)
    assert rh.shape == (n, K) and np.abs(rh - xc).max() <= 20 * TOL["single"] * np.abs(xc).max()
    with pytest.raises(ValueError, match="does not match"):
        wb.dec(xg[:, :2], level)


def test_every_instance_of_the_table_was_launched():
    """the coverage gate: each of the 96 entries of INSTANCES ran in some row above (each of which agreed with the oracle)"""
    assert len(INSTANCES) == 96
    recs = [r for p in ROWS + MORE_ROWS for r in cascade_records(p.id, p.values[0])]
    ran = {(r.family, r.params["T"], r.params["EW"], r.params["L"], r.params["NLEV"]) for r in recs}
    assert not (INSTANCES - ran), f"never launched: {sorted(INSTANCES - ran)}"
