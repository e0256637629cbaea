"""Plans over interleaved samples (ndwt_plan_create_interleaved): the array is [inner, dims.., howmany], every filtered axis strided.

The oracle is the numpy restatement (oracle/ndwt_oracle.py: spatial_dec / spatial_rec) applied to every item and every inner index on
its own: slice, transform, compare.  Tolerances are those of tests/test_gpu_parity.py: dec 1e-12 (double) / 2e-6 (single) relative to
max |c|, rec 2 TOL max(|want|, |c|).

  * the cascaded march (FwdMC / InvMC, csrc/ndwt_device_axis.h), forced with variants 11 / 11: the trace shows one FwdMC and one InvMC
    launch with the expected NLEV and grid (the double 8-tap synthesis: InvMC of two levels and one AxisMarch launch -- the table has no
    three-level instance); the oracle per column; dec bit for bit equal to one launch per level (variants 9 / 9), rec within the rec
    tolerance of it (the compiler fuses the two products of a synthesis tap differently in the two kernels); a NaN in
    one item, and in one inner index, stays there; guard words on both sides of every output;
  * what falls back to one launch per level: a pointer off by one scalar, comp * inner = 6, db5, an a-trous plan;
  * the per-axis routes of ndim >= 2 (RGB: inner = 3), reference and a-trous, with a round trip;
  * inner = 1 equals ndwt_plan_create_axes bit for bit; shrink, denoise, the pitched and the split-complex entry points; the refused
    entry points; the classes' 'inner' option; and every instance of the table launched once.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
import ndwt_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {"double": 1e-12, "single": 2e-6}                       # tests/test_gpu_parity.py
KINDS = {"f32": ("single", False), "c64": ("single", True), "f64": ("double", False), "c128": ("double", True)}
CASCADE = ("FwdMC", "InvMC")
PER_AXIS = ("AxisMarch", "AxisX", "axis_analysis_kernel", "axis_synthesis_kernel")
GUARD = 8


def instantiated(fam, T, L, nlev):
    """csrc/ndwt_fused_list.h: the CascadeMInstance table"""
    return L in (2, 4, 6, 8) and 2 <= nlev <= 4 and not (fam == "InvMC" and T == "double" and L == 8 and nlev >= 3)


INSTANCES = {(fam, T, L, nlev) for fam in CASCADE for T in ("float", "double") for L in (2, 4, 6, 8) for nlev in (2, 3, 4) if instantiated(fam, T, L, nlev)}
_LAUNCHED = set()


def types(kind):
    prec, cplx = KINDS[kind]
    rdt = torch.float32 if prec == "single" else torch.float64
    ndt = (np.complex64 if prec == "single" else np.complex128) if cplx else (np.float32 if prec == "single" else np.float64)
    tdt = (torch.complex64 if prec == "single" else torch.complex128) if cplx else rdt
    return prec, cplx, rdt, ndt, tdt


class _Buf:
    """n elements on the device with GUARD zero elements on both sides (off: elements the payload is shifted by, up to GUARD)"""

    def __init__(self, n, tdt, off=0):
        self.t = torch.zeros(n + 2 * GUARD, dtype=tdt, device="cuda")
        self.lo, self.n = GUARD + off, n
        self.view = self.t[self.lo:self.lo + n]

    def ptr(self):
        return self.view.data_ptr()

    def put(self, a_mat):
        """MATLAB-shaped array -> kernel order (the transpose, C-contiguous)"""
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(a_mat)).reshape(-1)).cuda())
        return self

    def get(self, shape_mat):
        return np.transpose(self.view.cpu().numpy().reshape(tuple(reversed(shape_mat))))

    def clean_outside(self, written=None):
        """zeros before and after the payload and -- `written`: [(start, stop)] -- between the runs that were to be written"""
        ok = float(self.t[:self.lo].abs().sum()) == 0 and float(self.t[self.lo + self.n:].abs().sum()) == 0
        if written:
            edges = [0] + [e for run in written for e in run] + [self.n]
            for a, b in zip(edges[0::2], edges[1::2]):
                ok = ok and (a == b or float(self.view[a:b].abs().sum()) == 0)
        return ok


def _per_part(f, a):
    return f(a.real) + 1j * f(a.imag) if np.iscomplexobj(a) else f(a)


def oracle(a, nd, wn, level, dilation, inverse):
    """a: [ne, dims.., K] (inverse: + bands last).  The oracle on every (inner index, item) slice on its own."""
    ne, K = a.shape[0], a.shape[1 + nd]
    one = (lambda v: orc.spatial_rec(v, wn, 1, dilation)) if inverse else (lambda v: orc.spatial_dec(v, wn, level, 1, dilation))
    out = None
    for c in range(ne):
        for k in range(K):
            idx = (c,) + (slice(None),) * nd + (k,)
            r = _per_part(one, a[idx])
            if out is None:
                out = np.zeros(a.shape[:2 + nd] + r.shape[nd:], dtype=a.dtype)
            out[idx] = r
    return out


_CASES = {}


def make_case(cid, kind, inner, dims, K, wn, level, dilation="reference"):
    """(x [ne, dims, K], dec(x), random coefficients c, rec(c)) -- computed once per case id, never modified"""
    if cid not in _CASES:
        prec, cplx, rdt, ndt, tdt = types(kind)
        nd = len(dims)
        wns = [wn] * nd if isinstance(wn, str) else list(wn)
        nb = int(ndwt.num_bands(nd, level))
        rng = np.random.default_rng(zlib.crc32(repr((cid, kind, inner, dims, K, wn, level, dilation)).encode()))

        def rnd(shape):
            a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
            return a.astype(ndt).astype(np.complex128 if cplx else np.float64)
        x = rnd((inner,) + tuple(dims) + (K,))
        c = rnd((inner,) + tuple(dims) + (K, nb))
        _CASES[cid] = (x, oracle(x, nd, wns, level, dilation, False), c, oracle(c, nd, wns, level, dilation, True))
    return _CASES[cid]


def chunks(groups, K, n, L, nlev, force=0):
    """cascadem_run's rule: about 4096 workgroups, chunks of at least 4 nlev (L - 1) planes, at most the axis"""
    iblocks = (groups * K + 255) // 256
    want = max(1, (4096 + iblocks - 1) // iblocks)
    chunk = max((n + want - 1) // want, 4 * nlev * (L - 1))
    if force:
        chunk = force
    chunk = min(chunk, n)
    return iblocks, (n + chunk - 1) // chunk


def make_plan(kind, inner, dims, K, wn, level, vf, vi, dilation="reference", force_zchunk=0):
    prec, cplx, rdt, ndt, tdt = types(kind)
    wns = [wn] * len(dims) if isinstance(wn, str) else list(wn)
    p = ndwt.Plan(list(dims), wns, rdt, cplx, True, dilation, max_level=level, inner=inner, howmany=K)
    p.set_variant(fwd=vf, inv=vi)
    if force_zchunk:
        p.set_tuning(0, force_zchunk)
    return p


def run_dec(p, kind, x, nb, level, off=0, pitch=0):
    tdt = types(kind)[4]
    vol = x.size
    xb = _Buf(vol, tdt, off).put(x)
    bs = pitch or vol
    yb = _Buf((nb - 1) * bs + vol, tdt, off)
    with ndwt.kernel_trace() as recs:
        p.dec(xb.ptr(), yb.ptr(), level, torch.cuda.current_stream().cuda_stream, band_pitch=pitch)
    torch.cuda.synchronize()
    assert yb.clean_outside([(b * bs, b * bs + vol) for b in range(nb)]) and xb.clean_outside()
    return yb, recs


def bands_of(yb, shape_x, nb, pitch=0):
    vol = int(np.prod(shape_x))
    bs = pitch or vol
    flat = yb.view.cpu().numpy()
    return np.stack([np.transpose(flat[b * bs:b * bs + vol].reshape(tuple(reversed(shape_x)))) for b in range(nb)], axis=-1)


def run_rec(p, kind, c, level, off=0, pitch=0):
    tdt = types(kind)[4]
    nb = c.shape[-1]
    vol = c[..., 0].size
    bs = pitch or vol
    yb = _Buf((nb - 1) * bs + vol, tdt, off)
    for b in range(nb):
        yb.view[b * bs:b * bs + vol].copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(c[..., b])).reshape(-1)).cuda())
    xb = _Buf(vol, tdt, off)
    with ndwt.kernel_trace() as recs:
        p.rec(yb.ptr(), xb.ptr(), level, torch.cuda.current_stream().cuda_stream, band_pitch=pitch)
    torch.cuda.synchronize()
    assert xb.clean_outside()
    return xb, recs


def check_dec(kind, got, want, what):
    tol = TOL[KINDS[kind][0]]
    err = np.abs(got - want).max()
    print(f"{what}: dec error {err:.3g} (bound {tol * np.abs(want).max():.3g})")
    assert err <= tol * np.abs(want).max(), what


def check_rec(kind, got, want, c, what):
    tol = TOL[KINDS[kind][0]]
    err, bound = np.abs(got - want).max(), 2 * tol * max(np.abs(want).max(), np.abs(c).max())
    print(f"{what}: rec error {err:.3g} (bound {bound:.3g})")
    assert err <= bound, what


# ------------------------------------------------------------------------------------------------ the cascaded march
# (id, kind, inner sizes, n, items, wavelet, forced planes per chunk); all 3 levels
CASCADE_ROWS = [
    ("f32-8x6-19-db2", "f32", (8, 6), 19, 1, "db2", 0),
    ("f32-4x1-8x3-db1", "f32", (4, 1), 8, 3, "db1", 0), ("f32-4x1-8x3-db2", "f32", (4, 1), 8, 3, "db2", 0),
    ("f32-4x1-8x3-db3", "f32", (4, 1), 8, 3, "db3", 0), ("f32-4x1-8x3-db4", "f32", (4, 1), 8, 3, "db4", 0),
    ("c64-6x1-16x3-db2", "c64", (6, 1), 16, 3, "db2", 0),
    ("f64-8x4-24x2-db4", "f64", (8, 4), 24, 2, "db4", 0),
    ("f32-64x64-32-db2", "f32", (64, 64), 32, 1, "db2", 0), ("f32-64x64-32-db2-chunk-12", "f32", (64, 64), 32, 1, "db2", 12),
]


@pytest.mark.parametrize("cid,kind,isz,n,K,wn,zc", CASCADE_ROWS, ids=[r[0] for r in CASCADE_ROWS])
def test_cascaded_march(cid, kind, isz, n, K, wn, zc):
    level = 3
    prec, cplx, rdt, ndt, tdt = types(kind)
    inner, comp, L = int(np.prod(isz)), 2 if cplx else 1, 2 * int(wn[2:])
    T = "float" if prec == "single" else "double"
    x, want, c, rwant = make_case(cid.replace("-chunk-12", ""), kind, inner, (n,), K, wn, level)
    nb = 1 + level
    pc, p9 = make_plan(kind, inner, (n,), K, wn, level, 11, 11, force_zchunk=zc), make_plan(kind, inner, (n,), K, wn, level, 9, 9)
    assert pc.describe() == "interleaved cascade" and p9.describe() == "interleaved axis"
    assert make_plan(kind, inner, (n,), K, wn, level, 0, 0).describe() == "interleaved axis"   # nothing is taken unasked
    groups = comp * inner // 4
    # ---- dec
    yb, recs = run_dec(pc, kind, x, nb, level)
    iblocks, nch = chunks(groups, K, n, L, 3, zc)
    got = [(r.family, r.params["T"], r.params["L"], r.params["NLEV"], r.grid, r.block) for r in recs]
    assert got == [("FwdMC", T, L, 3, (iblocks * nch, 1, 1), (256, 1, 1))], recs
    if zc:
        assert nch == 3                                        # 32 planes in chunks of 12: the last one partial
    _LAUNCHED.add(("FwdMC", T, L, 3))
    check_dec(kind, bands_of(yb, x.shape, nb), want, cid)
    y9, recs9 = run_dec(p9, kind, x, nb, level)
    assert [r.family for r in recs9] == ["AxisMarch"] * level and all(r.params["SYN"] is False for r in recs9)
    assert torch.equal(yb.view.view(rdt) if cplx else yb.view, y9.view.view(rdt) if cplx else y9.view), f"{cid}: dec differs from one launch per level"
    # ---- rec of random coefficients
    xb, recs = run_rec(pc, kind, c, level)
    nl = 3 if instantiated("InvMC", T, L, 3) else 2
    iblocks, nch = chunks(groups, K, n, L, nl, zc)
    got = [(r.family, r.params["T"], r.params["L"], r.params.get("NLEV"), r.grid) for r in recs]
    assert got[0] == ("InvMC", T, L, nl, (iblocks * nch, 1, 1)) and [g[0] for g in got[1:]] == ["AxisMarch"] * (3 - nl), recs
    _LAUNCHED.add(("InvMC", T, L, nl))
    check_rec(kind, xb.get(x.shape), rwant, c, cid)
    x9, recs9 = run_rec(p9, kind, c, level)
    assert [r.family for r in recs9] == ["AxisMarch"] * level and all(r.params["SYN"] is True for r in recs9)
    # (the compiler contracts lo a + hi d into an FMA around either product, and not the same one in InvMC as in
    # AxisMarch -- the synthesis is held to the rounding tolerance against one launch per level; whether the bits agree is printed)
    same = torch.equal(xb.view.view(rdt) if cplx else xb.view, x9.view.view(rdt) if cplx else x9.view)
    d9 = float((xb.view - x9.view).abs().max())
    print(f"{cid}: rec against one launch per level: max difference {d9:.3g}; bit-identical: {same}")
    assert d9 <= 2 * TOL[prec] * max(np.abs(rwant).max(), np.abs(c).max()), f"{cid}: rec differs from one launch per level"
    # ---- a NaN in one item and in one inner index stays there
    ci, ki = inner - 1, K - 1
    xn = x.copy()
    xn[ci, n // 2, ki] = np.nan
    gn = bands_of(run_dec(pc, kind, xn, nb, level)[0], x.shape, nb)
    bad = np.zeros(x.shape + (nb,), dtype=bool)
    bad[ci, :, ki, :] = True
    assert np.isnan(gn[bad]).any() and np.isfinite(gn[~bad]).all()
    assert np.array_equal(gn[~bad], bands_of(yb, x.shape, nb)[~bad])
    cn = c.copy()
    cn[ci, n // 2, ki, 1] = np.nan
    rn = run_rec(pc, kind, cn, level)[0].get(x.shape)
    assert np.isnan(rn[ci, :, ki]).any() and np.isfinite(rn[~bad[..., 0]]).all()
    assert np.array_equal(rn[~bad[..., 0]], xb.get(x.shape)[~bad[..., 0]])


# ------------------------------------------------------------------------------------------------ one launch per level instead
FALLBACK_ROWS = [
    # (id, kind, inner, n, items, wavelet, level, dilation, pointer offset in elements)
    ("f32-offset-pointer", "f32", 8, 19, 2, "db2", 3, "reference", 1),
    ("f64-offset-pointer", "f64", 8, 19, 2, "db4", 3, "reference", 1),
    ("f32-inner-6", "f32", 6, 19, 2, "db2", 3, "reference", 0),
    ("c64-inner-3", "c64", 3, 19, 2, "db2", 3, "reference", 0),
    ("f32-db5", "f32", 8, 19, 2, "db5", 3, "reference", 0),
    ("f32-atrous", "f32", 8, 32, 2, "db2", 3, "atrous", 0),
    ("c128-atrous", "c128", 4, 32, 2, "db2", 3, "atrous", 0),
]


@pytest.mark.parametrize("cid,kind,inner,n,K,wn,level,dilation,off", FALLBACK_ROWS, ids=[r[0] for r in FALLBACK_ROWS])
def test_what_cannot_cascade_runs_one_launch_per_level(cid, kind, inner, n, K, wn, level, dilation, off):
    x, want, c, rwant = make_case(cid, kind, inner, (n,), K, wn, level, dilation)
    nb = 1 + level
    p = make_plan(kind, inner, (n,), K, wn, level, 11, 11, dilation)
    yb, recs = run_dec(p, kind, x, nb, level, off=off)
    assert len(recs) == level and all(r.family in PER_AXIS and r.family != "AxisX" for r in recs), recs
    check_dec(kind, bands_of(yb, x.shape, nb), want, cid)
    xb, recs = run_rec(p, kind, c, level, off=off)
    assert len(recs) == level and all(r.family in PER_AXIS and r.family != "AxisX" for r in recs), recs
    check_rec(kind, xb.get(x.shape), rwant, c, cid)
    if "offset" in cid or "inner" in cid:                      # no whole groups of 4 scalars: the element-wise kernels
        assert {r.family for r in recs} == {"axis_synthesis_kernel"}
    if cid == "f32-db5":
        assert {r.family for r in recs} == {"AxisMarch"} and p.describe() == "interleaved axis"


# ------------------------------------------------------------------------------------------------ two and three filtered axes
def _nd_rows():
    rows = []
    for kind in ("f32", "c128"):
        for wn in ("db2", "db4"):
            for dilation in ("reference", "atrous"):
                rows.append((f"{kind}-4-24x20-3-{wn}-{dilation}", kind, 4, (24, 20), 3, wn, 2, dilation))
                rows.append((f"{kind}-rgb-24x20-2-{wn}-{dilation}", kind, 3, (24, 20), 2, wn, 2, dilation))
    rows.append(("f32-4-12x10x9-2-db2", "f32", 4, (12, 10, 9), 2, "db2", 2, "reference"))
    return rows


@pytest.mark.parametrize("cid,kind,inner,dims,K,wn,level,dilation", _nd_rows(), ids=[r[0] for r in _nd_rows()])
def test_per_axis_routes_of_images_and_volumes(cid, kind, inner, dims, K, wn, level, dilation):
    nd = len(dims)
    x, want, c, rwant = make_case(cid, kind, inner, dims, K, wn, level, dilation)
    nb = int(ndwt.num_bands(nd, level))
    p = make_plan(kind, inner, dims, K, wn, level, 11, 11, dilation)
    assert p.describe() == "interleaved axis"
    yb, recs = run_dec(p, kind, x, nb, level)
    assert len(recs) == level * ((1 << nd) - 1) and all(r.family in ("AxisMarch", "axis_analysis_kernel") for r in recs), recs
    if (inner * (2 if KINDS[kind][1] else 1)) % 4 == 0:       # samples of whole groups of 4 scalars: the register-window march on every axis
        assert {r.family for r in recs} == {"AxisMarch"}
    else:                                                      # RGB: axis 0 element-wise (3 or 6 scalars), axis 1 marches 24 samples' worth
        assert {r.family for r in recs} == {"AxisMarch", "axis_analysis_kernel"}
    got = bands_of(yb, x.shape, nb)
    check_dec(kind, got, want, cid)
    xb, recs = run_rec(p, kind, c, level)
    assert len(recs) == level * ((1 << nd) - 1) and all(r.family in ("AxisMarch", "axis_synthesis_kernel") for r in recs), recs
    check_rec(kind, xb.get(x.shape), rwant, c, cid)
    back = run_rec(p, kind, got, level)[0].get(x.shape)        # the round trip
    assert np.abs(back - x).max() <= 20 * TOL[KINDS[kind][0]] * np.abs(x).max()


# ------------------------------------------------------------------------------------------------ everything else
def test_inner_one_is_the_stack_plan_bit_for_bit():
    dims, K, level = (64, 40), 3, 3
    x = torch.randn(K * 40 * 64, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for p in (ndwt.Plan(list(dims), ["db4", "db2"], torch.float32, max_level=level, inner=1, howmany=K),
              ndwt.Plan(list(dims) + [K], ["db4", "db2", None], torch.float32, max_level=level, axes=(0, 1))):
        y = torch.zeros(10 * x.numel(), dtype=torch.float32, device="cuda")
        r = torch.zeros_like(x)
        with ndwt.kernel_trace() as recs:
            p.dec(x.data_ptr(), y.data_ptr(), level, stream)
            p.rec(y.data_ptr(), r.data_ptr(), level, stream)
        torch.cuda.synchronize()
        outs.append((p.describe(), [(q.text, q.grid, q.block) for q in recs], y, r, p.band_pitch()))
    assert outs[0][0] == outs[1][0] == "stack2d fused" and outs[0][1] == outs[1][1] and outs[0][4] == outs[1][4]
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][3], outs[1][3])


def _np_shrink(c, t, hard):
    m = np.abs(c)
    out = c * (np.where(m > t, 1.0, 0.0) if hard else np.where(m > t, (m - t) / np.where(m > 0, m, 1.0), 0.0))
    out[..., 0] = c[..., 0]
    return out


SERVED_ROWS = [("served-cascade", "c64", 6, (16,), 3, "db2", 3, 11), ("served-images", "f64", 3, (24, 20), 2, "db2", 2, 0)]


@pytest.mark.parametrize("cid,kind,inner,dims,K,wn,level,v", SERVED_ROWS, ids=[r[0] for r in SERVED_ROWS])
def test_shrink_denoise_pitched_and_split_entry_points(cid, kind, inner, dims, K, wn, level, v):
    prec, cplx, rdt, ndt, tdt = types(kind)
    tol, nd = TOL[prec], len(dims)
    x, want, c, rwant = make_case(cid, kind, inner, dims, K, wn, level)
    nb, vol = int(ndwt.num_bands(nd, level)), x.size
    p = make_plan(kind, inner, dims, K, wn, level, v, v)
    stream = torch.cuda.current_stream().cuda_stream
    # pitched at ndwt_band_pitch: the layout of the issue -- inner prod(dims) howmany plus the usual skew
    pitch = p.band_pitch()
    assert pitch == vol + 256 // ((2 if cplx else 1) * (4 if prec == "single" else 8))
    yb, recs = run_dec(p, kind, x, nb, level, pitch=pitch)
    if v == 11:
        assert [r.family for r in recs] == ["FwdMC"]
    got = bands_of(yb, x.shape, nb, pitch)
    check_dec(kind, got, want, cid + " pitched")
    xb, recs = run_rec(p, kind, c, level, pitch=pitch)
    if v == 11:
        assert [r.family for r in recs] == ["InvMC"]
    check_rec(kind, xb.get(x.shape), rwant, c, cid + " pitched")
    # shrink in place, packed and pitched
    for hard in (False, True):
        for pt in (0, pitch):
            bs = pt or vol
            sb = _Buf((nb - 1) * bs + vol, tdt)
            for b in range(nb):
                sb.view[b * bs:b * bs + vol].copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(want[..., b]).astype(ndt)).reshape(-1)).cuda())
            with ndwt.kernel_trace() as recs:
                p.shrink(sb.ptr(), level, 0.5, hard, stream, band_pitch=pt)
            torch.cuda.synchronize()
            assert {r.family for r in recs} == {"shrink_kernel"}
            assert sb.clean_outside([(b * bs, b * bs + vol) for b in range(nb)])
            ref = _np_shrink(want.astype(ndt).astype(want.dtype), 0.5, hard)
            near = np.abs(np.abs(want[..., 1:]) - 0.5) < 1e-4   # (a magnitude at the threshold may fall either way in single precision)
            d = np.abs(bands_of(sb, x.shape, nb, pt) - ref)
            d[..., 1:][near] = 0
            assert d.max() <= 4 * tol * np.abs(want).max(), (hard, pt)
    # denoise = dec, the shrink pass, rec (no kernel thresholds interleaved samples on load)
    ob = _Buf(vol, tdt)
    xin = _Buf(vol, tdt).put(x)
    with ndwt.kernel_trace() as recs:
        p.denoise(xin.ptr(), ob.ptr(), level, 0.25, False, stream)
    torch.cuda.synchronize()
    assert "shrink_kernel" in {r.family for r in recs} and ob.clean_outside()
    wns = [wn] * nd
    dwant = oracle(_np_shrink(want, 0.25, False), nd, wns, level, "reference", True)
    assert np.abs(ob.get(x.shape) - dwant).max() <= 20 * tol * np.abs(x).max()
    # split complex on a real plan of the same shape: each part is the real transform
    pr = make_plan("f32" if prec == "single" else "f64", inner, dims, K, wn, level, v, v)
    xc = x if cplx else x + 1j * np.roll(x, 1, axis=1)
    wc = want if cplx else want + 1j * np.roll(want, 1, axis=1)
    xr, xi = _Buf(vol, rdt).put(xc.real), _Buf(vol, rdt).put(xc.imag)
    yr, yi = _Buf(nb * vol, rdt), _Buf(nb * vol, rdt)
    pr.dec_split(xr.ptr(), xi.ptr(), yr.ptr(), yi.ptr(), level, stream)
    torch.cuda.synchronize()
    gs = bands_of(yr, x.shape, nb) + 1j * bands_of(yi, x.shape, nb)
    assert np.abs(gs - wc).max() <= tol * np.abs(wc).max() and yr.clean_outside() and yi.clean_outside()
    br, bi = _Buf(vol, rdt), _Buf(vol, rdt)
    pr.rec_split(yr.ptr(), yi.ptr(), br.ptr(), bi.ptr(), level, stream)
    torch.cuda.synchronize()
    back = br.get(x.shape) + 1j * bi.get(x.shape)
    assert np.abs(back - xc).max() <= 20 * tol * np.abs(xc).max() and br.clean_outside() and bi.clean_outside()


def test_refused_entry_points_say_so():
    """whatever sizes a buffer by one array's dimensions refuses these plans with the batched-plan message: nothing launched"""
    lib = ndwt.lib()
    for dims, inner, K in (([19], 8, 2), ([24, 20], 3, 1)):
        p = ndwt.Plan(dims, ["db2"] * len(dims), torch.float64, max_level=2, inner=inner, howmany=K)
        h = p._h
        n = int(np.prod(dims)) * inner * K * 16
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


def test_the_classes_take_inner():
    """nd_dwt_1D(wname, n, 'inner', [a, b], 'batch', K): [a, b, n, K] in, [a, b, n, K, bands] out; nd_dwt_2D with RGB samples"""
    rng = np.random.default_rng(3)
    a, b, n, K, level = 4, 2, 19, 3, 3
    x = rng.standard_normal((a, b, n, K))
    w = ndwt.nd_dwt_1D("db2", n, "inner", [a, b], "batch", K, "pres_l2_norm", 1)
    xg = torch.from_numpy(np.ascontiguousarray(np.transpose(x))).cuda().permute(3, 2, 1, 0)
    with ndwt.kernel_trace() as recs:
        y = w.dec(xg, level)
    assert tuple(y.shape) == (a, b, n, K, 1 + level) and [r.family for r in recs] == ["AxisMarch"] * level
    want = oracle(x.reshape(a * b, n, K, order="F"), 1, ["db2"], level, "reference", False).reshape((a, b, n, K, 1 + level), order="F")
    assert np.abs(y.cpu().numpy() - want).max() <= TOL["double"] * np.abs(want).max()
    r = w.rec(y)
    assert tuple(r.shape) == (a, b, n, K) and float((r - xg).abs().max()) <= 20 * TOL["double"] * float(xg.abs().max())
    d = w.denoise(xg, level, 0.5)
    s = w.rec(w.shrink(y, 0.5))
    assert tuple(d.shape) == (a, b, n, K) and float((d - s).abs().max()) <= 4 * TOL["double"] * float(xg.abs().max())
    wh = ndwt.nd_dwt_2D("db2", [24, 20], "inner", 3, "compute", "hip_off", "precision", "single", "pres_l2_norm", 1)
    xc = (rng.standard_normal((3, 24, 20)) + 1j * rng.standard_normal((3, 24, 20))).astype(np.complex64)
    yh = wh.dec(xc, 2)
    assert isinstance(yh, np.ndarray) and yh.shape == (3, 24, 20, 7) and yh.dtype == np.complex64
    want = oracle(xc.astype(np.complex128)[..., None], 2, ["db2", "db2"], 2, "reference", False)[:, :, :, 0, :]
    assert np.abs(yh - want).max() <= TOL["single"] * np.abs(want).max()
    assert np.abs(wh.rec(yh) - xc).max() <= 20 * TOL["single"] * np.abs(xc).max()
    with pytest.raises(ValueError, match="does not match"):
        w.dec(xg[:, :, :, :2], level)


def test_every_instance_of_the_table_was_launched():
    """the coverage gate: the rows above launched some instances; the rest run here on [4 scalars, L planes, 1 item] -- the smallest
    array an instance takes -- against the oracle.  Every instance of the table, and nothing outside it."""
    for fam, T, L, nlev in sorted(INSTANCES - _LAUNCHED):
        kind = "f32" if T == "float" else "f64"
        wn = f"db{L // 2}"
        cid = f"gate-{T}-{L}-{nlev}"
        x, want, c, rwant = make_case(cid, kind, 4, (L,), 1, wn, nlev)
        p = make_plan(kind, 4, (L,), 1, wn, nlev, 11, 11)
        if fam == "FwdMC":
            yb, recs = run_dec(p, kind, x, 1 + nlev, nlev)
            check_dec(kind, bands_of(yb, x.shape, 1 + nlev), want, cid)
        else:
            xb, recs = run_rec(p, kind, c, nlev)
            check_rec(kind, xb.get(x.shape), rwant, c, cid)
        assert [(r.family, r.params["T"], r.params["L"], r.params["NLEV"]) for r in recs] == [(fam, T, L, nlev)], (cid, recs)
        _LAUNCHED.add((fam, T, L, nlev))
    assert _LAUNCHED == INSTANCES
