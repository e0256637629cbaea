"""Per-band thresholds on the device: ndwt_shrink_bands / ndwt_denoise_bands on every plan kind, and the one-launch route of a batched 1-D
plan (Den1C, csrc/ndwt_device_1d.h), asked for with variant 11 / 11.

  * route and grid: one launch, family Den1C with the row's T, L, NLEV, EW on ceil(K nseg / 4) workgroups of 256; variant 9 runs dec,
    one shrink_kernel per non-zero band, rec;
  * values: the shapes of tests/test_emulated_den1c.py against the fp64 oracle (soft: 20 TOL, the bound of tests/test_gpu_batch1d.py)
    and against the general route of the same build (4 TOL max|x|, both modes); hard thresholds sit in the widest gap of the oracle's
    |c| around each band's median (the gap is asserted >= 200 TOL max|c|), so no coefficient is within rounding of its threshold;
  * guard elements around `out`, a NaN signal that must not reach its neighbours, a pitched caller layout for shrink_bands;
  * the silent fallbacks (x == out, out off by 4 bytes, level 5, a-trous, odd n, db5, an unbatched plan), by trace and by value;
  * shrink_bands with equal thresholds bit-identical to ndwt_shrink, all-zero thresholds launching nothing;
  * the general route on a 2-D plan, a 3-D complex plan, a stack and interleaved samples, against numpy;
  * the classes; the coverage gate over the instance table; ndwt_denoise with a scalar keeps its three-kernel route (Fwd1C, shrink_kernel, Inv1C).
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
import ndwt_oracle as orc
import ndwt_spatial as orc_c

pytestmark = pytest.mark.gpu

TOL = {"double": 1e-12, "single": 2e-6}                       # tests/test_gpu_parity.py
KINDS = {"f32": ("single", False), "c64": ("single", True), "f64": ("double", False), "c128": ("double", True)}
# the instance table (csrc/ndwt_fused_list.h: NDWT_LIST_*DEN1): (T, EW, L, NLEV), less the three complex128 instances that spill
SPILL = {("double", 2, 6, 4), ("double", 2, 8, 3), ("double", 2, 8, 4)}
INSTANCES = {(T, ew, L, nlev) for T in ("float", "double") for ew in (1, 2) for L in (2, 4, 6, 8) for nlev in (1, 2, 3, 4)} - SPILL
GENERAL = ("Fwd1C", "Inv1C", "AxisX", "AxisMarch", "axis_analysis_kernel", "axis_synthesis_kernel", "shrink_kernel")
GUARD = 4                                                     # elements before and after a buffer (16 / 32 bytes: the alignment stays)


def types(kind):
    prec, cplx = KINDS[kind]
    rdt = torch.float32 if prec == "single" else torch.float64
    ndt = (np.complex64 if prec == "single" else np.complex128) if cplx else (np.float32 if prec == "single" else np.float64)
    tdt = (torch.complex64 if prec == "single" else torch.complex128) if cplx else rdt
    return prec, cplx, rdt, ndt, tdt, ("float" if prec == "single" else "double"), (2 if cplx else 1), TOL[prec]


def tile_width(kind, L, nlev):
    """Den1C::WX: the lanes valid after nlev analysis and nlev synthesis levels, in whole 128-byte lines"""
    prec, cplx = KINDS[kind]
    ew, lpl = (2 if cplx else 1), (8 if prec == "single" else 4)
    GLa, GRa = ((L // 2 - 1) * ew + 3) // 4, ((L // 2) * ew + 3) // 4
    return 4 * ((64 - nlev * 2 * (GLa + GRa)) // lpl * lpl)


def stream():
    return torch.cuda.current_stream().cuda_stream


def np_shrink_bands(c, thr, hard):
    """band b of c[..., b] shrunk by thr[b] (complex: the magnitude); 0 leaves the band as it is"""
    out = c.copy()
    for b, t in enumerate(thr):
        if t == 0:
            continue
        cb = c[..., b]
        m = np.abs(cb)
        out[..., b] = cb * (np.where(m > t, 1.0, 0.0) if hard else np.where(m > t, (m - t) / np.where(m > 0, m, 1.0), 0.0))
    return out


def gap_thresholds(c, tol, band0=False):
    """per band the middle of the widest gap among the 40 order statistics of the oracle's |c| around the median; the gap must be wide"""
    thr = np.zeros(c.shape[-1])
    for b in range(0 if band0 else 1, c.shape[-1]):
        m = np.sort(np.abs(c[..., b]).reshape(-1))
        w = m[max(m.size // 2 - 20, 0):m.size // 2 + 20]
        gaps = np.diff(w)
        i = int(np.argmax(gaps))
        assert gaps[i] >= 200 * tol * m.max(), f"band {b}: widest gap {gaps[i]:.3g} < {200 * tol * m.max():.3g}: choose another seed"
        thr[b] = 0.5 * (w[i] + w[i + 1])
    return thr


class Buf:
    """n elements with GUARD zero elements before and after (off: where the buffer starts inside the allocation)"""

    def __init__(self, n, tdt, off=GUARD):
        self.t = torch.zeros(n + off + GUARD, dtype=tdt, device="cuda")
        self.off, self.n, self.view = off, n, self.t[off:off + n]

    def ptr(self):
        return self.view.data_ptr()

    def clean_outside(self):
        return float(self.t[:self.off].abs().sum()) == 0 and float(self.t[self.off + self.n:].abs().sum()) == 0


def signals(kind, n, K, seed):
    prec, cplx, rdt, ndt, tdt, T, comp, tol = types(kind)
    rng = np.random.default_rng(zlib.crc32(repr(seed).encode()))
    x = rng.standard_normal((n, K)) + (1j * rng.standard_normal((n, K)) if cplx else 0)
    return x.astype(ndt).astype(np.complex128 if cplx else np.float64)


def to_dev(x, kind, off=GUARD):
    ndt, tdt = types(kind)[3], types(kind)[4]
    b = Buf(x.size, tdt, off)
    b.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(x)).astype(ndt).reshape(-1)).cuda())
    return b


def from_dev(b, shape):
    return np.transpose(b.view.cpu().numpy().reshape(tuple(reversed(shape))))


def oracle_coefs(x, wn, level, dil="reference"):
    return np.stack([orc_c.spatial_dec(x[:, k], [wn], level, 1, dil) for k in range(x.shape[1])], axis=1)          # [n, K, bands]


def oracle_rec(c, wn, dil="reference"):
    return np.stack([orc_c.spatial_rec(c[:, k], [wn], 1, dil) for k in range(c.shape[1])], axis=1)


def plan(kind, n, wn, level, K, variant, dil="reference"):
    prec, cplx, rdt = types(kind)[:3]
    p = ndwt.Plan([n], [wn], rdt, cplx, True, dil, max_level=level, howmany=K)
    p.set_variant(fwd=variant, inv=variant)
    return p


def check_den1c(recs, kind, L, level, K, row, what):
    prec, cplx, rdt, ndt, tdt, T, comp, tol = types(kind)
    assert len(recs) == 1 and recs[0].family == "Den1C", f"{what}: expected one Den1C launch, got {recs}"
    r = recs[0]
    assert (r.params["T"], r.params["L"], r.params["NLEV"], r.params["EW"]) == (T, L, level, comp), f"{what}: {r!r}"
    nseg = -(-row // tile_width(kind, L, level))
    assert r.grid == (-(-K * nseg // 4), 1, 1) and r.block == (256, 1, 1), f"{what}: {r!r}, expected ceil({K} x {nseg} / 4) workgroups of 256"
    return (T, comp, L, level)


def check_general(recs, thr, what):
    fams = [r.family for r in recs]
    assert "Den1C" not in fams and all(f in GENERAL for f in fams), f"{what}: {recs}"
    assert fams.count("shrink_kernel") == int(np.count_nonzero(thr)), f"{what}: one shrink pass per non-zero band: {recs}"
    assert fams[0] != "shrink_kernel" and fams[-1] != "shrink_kernel", f"{what}: dec, the shrink passes, rec: {recs}"


# (id, wavelet, levels, signals, scalars per row or None = WX + 32 of the kind, thresholds: "details" | "zero" | "all")
SHAPES = [
    ("two-segments-db4-3", "db4", 3, 3, None, "details"),
    ("shortest-row-db4-4", "db4", 4, 2, 64, "details"),
    ("idle-waves-db2-2", "db2", 2, 5, 96, "details"),
    ("one-level-db1", "db1", 1, 2, None, "details"),
    ("four-levels-db3", "db3", 4, 2, None, "details"),
    ("all-zero-db4-3", "db4", 3, 3, None, "zero"),
    ("band0-too-db2-2", "db2", 2, 5, 96, "all"),
]
CASES = [pytest.param(kind, wn, nlev, K, row, which, id=f"{kind}-{sid}") for kind in KINDS for sid, wn, nlev, K, row, which in SHAPES]


@pytest.mark.parametrize("kind,wn,level,K,row,which", CASES)
def test_one_launch_route_grid_and_values(kind, wn, level, K, row, which, request):
    prec, cplx, rdt, ndt, tdt, T, comp, tol = types(kind)
    L = 2 * int(wn[2:])
    row = row or tile_width(kind, L, level) + 32
    n = row // comp
    rid = request.node.callspec.id
    x = signals(kind, n, K, (rid, n, K))
    c = oracle_coefs(x, wn, level)
    p11, p9 = plan(kind, n, wn, level, K, 11), plan(kind, n, wn, level, K, 9)
    xb = to_dev(x, kind)
    for hard in (False, True):
        if which == "zero":
            thr = np.zeros(1 + level)
        elif hard:
            thr = gap_thresholds(c, tol, band0=(which == "all"))
        else:
            thr = 1.5 * ndwt.band_gains([n], wn, level, pres_l2_norm=1)
            if which != "all":
                thr[0] = 0.0
        want = oracle_rec(np_shrink_bands(c, thr, hard), wn)
        ob, og = Buf(n * K, tdt), Buf(n * K, tdt)
        ob.view.fill_(float("nan"))
        with ndwt.kernel_trace() as recs:
            p11.denoise_bands(xb.ptr(), ob.ptr(), level, thr, hard, stream())
        with ndwt.kernel_trace() as recs9:
            p9.denoise_bands(xb.ptr(), og.ptr(), level, thr, hard, stream())
        torch.cuda.synchronize()
        what = f"{rid} {'hard' if hard else 'soft'}"
        if (T, comp, L, level) in INSTANCES:
            check_den1c(recs, kind, L, level, K, row, what)
        else:                                                 # complex128 db4 at 3 / 4 levels left the table (spills): the general route
            check_general(recs, thr, what)
        check_general(recs9, thr, what)
        got, gen = from_dev(ob, (n, K)), from_dev(og, (n, K))
        assert np.isfinite(got).all(), f"{what}: an element of out was not written"
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1.0)
        dg = np.abs(got - gen).max()
        same = torch.equal(ob.view.view(rdt), og.view.view(rdt))
        print(f"{what}: row {row} x {K}, against the oracle {err:.3g} (bound {20 * tol:.3g}), against the general route {dg:.3g} "
              f"(bound {4 * tol * np.abs(x).max():.3g}); bit-identical: {same}")
        if not hard:
            assert err <= 20 * tol, (what, "oracle", err)
        assert dg <= 4 * tol * np.abs(x).max(), (what, "general route", dg)
        assert ob.clean_outside() and og.clean_outside(), f"{what}: wrote outside out"


def test_variant_nine_runs_dec_the_shrink_passes_and_rec():
    n, K, level = 512, 3, 4
    x = signals("f32", n, K, "variant-9")
    thr = 1.5 * ndwt.band_gains([n], "db4", level, pres_l2_norm=1)
    xb, ob = to_dev(x, "f32"), Buf(n * K, torch.float32)
    with ndwt.kernel_trace() as recs:
        plan("f32", n, "db4", level, K, 9).denoise_bands(xb.ptr(), ob.ptr(), level, thr, False, stream())
    torch.cuda.synchronize()
    assert [r.family for r in recs] == ["AxisX"] * level + ["shrink_kernel"] * 5 + ["AxisX"] * level, recs
    p0 = plan("f32", n, "db4", level, K, 0)
    with ndwt.kernel_trace() as recs:
        p0.denoise_bands(xb.ptr(), ob.ptr(), level, thr, False, stream())
    torch.cuda.synchronize()
    fams = [r.family for r in recs]
    assert fams in (["Den1C"], ["Fwd1C"] + ["shrink_kernel"] * 5 + ["Inv1C"]), recs      # the data kind's default, whichever it is


def test_scalar_denoise_on_a_batched_plan_keeps_its_three_kernel_route():
    n, K, level = 512, 3, 4
    x = signals("f32", n, K, "scalar")
    xb, ob = to_dev(x, "f32"), Buf(n * K, torch.float32)
    for v in (0, 11):
        with ndwt.kernel_trace() as recs:
            plan("f32", n, "db4", level, K, v).denoise(xb.ptr(), ob.ptr(), level, 0.3, False, stream())
        torch.cuda.synchronize()
        # (the coefficients of a denoise are pitched: one shrink pass per detail band)
        assert [r.family for r in recs] == ["Fwd1C"] + ["shrink_kernel"] * level + ["Inv1C"], (v, recs)


def test_a_nan_signal_stays_in_its_own_rows():
    n, K, level = 256, 3, 3
    x = signals("f32", n, K, "nan")
    x[17, 1] = np.nan
    thr = 1.5 * ndwt.band_gains([n], "db4", level, pres_l2_norm=1)
    thr[0] = 0.0                                              # (a thresholded band turns NaN into 0: |NaN| > t is false; band 0 keeps it)
    xb, ob = to_dev(x, "f32"), Buf(n * K, torch.float32)
    with ndwt.kernel_trace() as recs:
        plan("f32", n, "db4", level, K, 11).denoise_bands(xb.ptr(), ob.ptr(), level, thr, False, stream())
    torch.cuda.synchronize()
    assert [r.family for r in recs] == ["Den1C"]
    got = from_dev(ob, (n, K))
    assert np.isfinite(got[:, 0]).all() and np.isfinite(got[:, 2]).all() and np.isnan(got[:, 1]).any()
    assert ob.clean_outside()


FALLBACKS = [
    pytest.param(dict(same=True), id="x-is-out"),
    pytest.param(dict(off=GUARD + 1), id="out-off-by-4-bytes"),
    pytest.param(dict(level=5), id="level-5"),
    pytest.param(dict(dil="atrous"), id="atrous"),
    pytest.param(dict(n=255), id="n-odd"),
    pytest.param(dict(wn="db5"), id="db5"),
    pytest.param(dict(K=None), id="unbatched"),
]


@pytest.mark.parametrize("f", FALLBACKS)
def test_silent_fallback_to_the_general_route(f, request):
    kind, tol = "f32", TOL["single"]
    n, K, level, wn, dil = f.get("n", 256), f.get("K", 3), f.get("level", 3), f.get("wn", "db4"), f.get("dil", "reference")
    x = signals(kind, n, K or 1, request.node.callspec.id)
    thr = 1.5 * ndwt.band_gains([n], wn, level, pres_l2_norm=1, dilation=dil)
    thr[0] = 0.0
    want = oracle_rec(np_shrink_bands(oracle_coefs(x, wn, level, dil), thr, False), wn, dil)
    p = ndwt.Plan([n], [wn], torch.float32, False, True, dil, max_level=level, howmany=K)
    p.set_variant(fwd=11, inv=11)
    xb = to_dev(x, kind)
    ob = xb if f.get("same") else Buf(x.size, torch.float32, f.get("off", GUARD))
    with ndwt.kernel_trace() as recs:
        p.denoise_bands(xb.ptr(), ob.ptr(), level, thr, False, stream())
    torch.cuda.synchronize()
    check_general(recs, thr, request.node.callspec.id)
    got = from_dev(ob, x.shape)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1.0)
    print(f"{request.node.callspec.id}: {[r.family for r in recs]}, against the oracle {err:.3g} (bound {20 * tol:.3g})")
    assert err <= 20 * tol and ob.clean_outside()


@pytest.mark.parametrize("kind", ["f32", "c128"])
def test_shrink_bands_with_equal_thresholds_is_ndwt_shrink_bit_for_bit(kind):
    prec, cplx, rdt, ndt, tdt, T, comp, tol = types(kind)
    n, K, level, t = 256, 3, 3, 0.7
    nb, vol = 1 + level, n * K
    p = plan(kind, n, "db4", level, K, 0)
    for pitch in (vol, p.band_pitch()):
        y = torch.zeros((nb - 1) * pitch + vol, dtype=tdt, device="cuda")
        for b in range(nb):
            y[b * pitch:b * pitch + vol] = torch.randn(vol, dtype=tdt, device="cuda")
        y0, y1, y2 = y.clone(), y.clone(), y.clone()
        bp = 0 if pitch == vol else pitch
        p.shrink(y1.data_ptr(), level, t, False, stream(), band_pitch=bp)
        with ndwt.kernel_trace() as recs:
            p.shrink_bands(y2.data_ptr(), level, [0.0] + [t] * level, False, stream(), band_pitch=bp)
        torch.cuda.synchronize()
        assert [r.family for r in recs] == ["shrink_kernel"] * level
        assert torch.equal(y1.view(rdt), y2.view(rdt)) and not torch.equal(y1.view(rdt), y0.view(rdt)), (kind, pitch)
        # distinct thresholds, band 0 too, hard: against numpy, band by band (the gaps between pitched bands stay zero)
        thr = np.array([0.3, 0.5, 0.0, 0.9])
        p.shrink_bands(y.data_ptr(), level, thr, True, stream(), band_pitch=bp)
        got = np.stack([y[b * pitch:b * pitch + vol].cpu().numpy() for b in range(nb)], axis=-1)
        src = np.stack([y0[b * pitch:b * pitch + vol].cpu().numpy() for b in range(nb)], axis=-1)
        assert np.array_equal(got, np_shrink_bands(src, thr.astype(ndt().real.dtype), True).astype(got.dtype))
        for b in range(nb - 1):
            assert float(y[b * pitch + vol:(b + 1) * pitch].abs().sum()) == 0
        # all zero: nothing is launched, nothing changes
        with ndwt.kernel_trace() as recs:
            p.shrink_bands(y2.data_ptr(), level, [0.0] * nb, True, stream(), band_pitch=bp)
        torch.cuda.synchronize()
        assert recs == [] and torch.equal(y1.view(rdt), y2.view(rdt))


def test_bad_thresholds_are_refused_and_name_the_band():
    p = plan("f32", 256, "db4", 3, 2, 0)
    x = torch.zeros(512, dtype=torch.float32, device="cuda")
    for thr, band in (([0.1, 0.1, -1.0, 0.1], 2), ([0.1, float("nan"), 0.1, 0.1], 1)):
        with pytest.raises(ndwt.NdwtError, match=f"band {band}") as e:
            p.denoise_bands(x.data_ptr(), x.data_ptr(), 3, thr, False, stream())
        assert e.value.code == 1
    with pytest.raises(ValueError, match="4 thresholds expected"):
        p.shrink_bands(x.data_ptr(), 3, [0.1] * 3)


def _nd_oracle(x, wnames, level, thr, hard=False):
    one = lambda v: orc.spatial_rec(np_shrink_bands(orc.spatial_dec(v, wnames, level, 1), thr, hard), wnames, 1)   # noqa: E731
    if not np.iscomplexobj(x):
        return one(x)
    c = orc.spatial_dec(x.real, wnames, level, 1) + 1j * orc.spatial_dec(x.imag, wnames, level, 1)
    cs = np_shrink_bands(c, thr, hard)
    return orc.spatial_rec(cs.real, wnames, 1) + 1j * orc.spatial_rec(cs.imag, wnames, 1)


def test_general_route_on_the_other_plan_kinds_against_numpy():
    rng = np.random.default_rng(11)
    s, tol = stream(), TOL["single"]

    def run(p, x, ndt, tdt, level, thr, nbands_nonzero):
        xd = torch.from_numpy(np.ascontiguousarray(np.transpose(x)).astype(ndt).reshape(-1)).cuda()
        od = torch.empty_like(xd)
        with ndwt.kernel_trace() as recs:
            p.denoise_bands(xd.data_ptr(), od.data_ptr(), level, thr, False, s)
        torch.cuda.synchronize()
        fams = [r.family for r in recs]
        assert "Den1C" not in fams and fams.count("shrink_kernel") == nbands_nonzero, recs
        return np.transpose(od.cpu().numpy().reshape(tuple(reversed(x.shape))))

    def close(got, want, what):
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1.0)
        print(f"{what}: against numpy {err:.3g} (bound {20 * tol:.3g})")
        assert err <= 20 * tol, (what, err)

    # 2-D [32, 32] float db2 at 2 levels
    x = rng.standard_normal((32, 32)).astype(np.float32).astype(np.float64)
    thr = 1.5 * ndwt.band_gains([32, 32], "db2", 2, pres_l2_norm=1)
    thr[0] = 0.0
    p = ndwt.Plan([32, 32], ["db2", "db2"], torch.float32, False, True, "reference", max_level=2)
    close(run(p, x, np.float32, torch.float32, 2, thr, 6), _nd_oracle(x, ["db2", "db2"], 2, thr), "2-D")
    # a stack [32, 32, 3] of such images, band 0 thresholded too
    xs = rng.standard_normal((32, 32, 3)).astype(np.float32).astype(np.float64)
    thr0 = 1.5 * ndwt.band_gains([32, 32], "db2", 2, pres_l2_norm=1)
    p = ndwt.Plan([32, 32, 3], ["db2", "db2", None], torch.float32, False, True, "reference", max_level=2, axes=(0, 1))
    want = np.stack([_nd_oracle(xs[:, :, j], ["db2", "db2"], 2, thr0) for j in range(3)], axis=-1)
    close(run(p, xs, np.float32, torch.float32, 2, thr0, 7), want, "stack")
    # 3-D [16, 16, 16] complex64 db1 at 2 levels
    xc = (rng.standard_normal((16, 16, 16)) + 1j * rng.standard_normal((16, 16, 16))).astype(np.complex64).astype(np.complex128)
    thr3 = 1.5 * ndwt.band_gains([16, 16, 16], "db1", 2, pres_l2_norm=1)
    thr3[0] = 0.0
    p = ndwt.Plan([16, 16, 16], ["db1"] * 3, torch.float32, True, True, "reference", max_level=2)
    close(run(p, xc, np.complex64, torch.complex64, 2, thr3, 14), _nd_oracle(xc, ["db1"] * 3, 2, thr3), "3-D complex64")
    # interleaved samples [4, 64, 2]: 4 channels together, 64 samples filtered, 2 items
    xi = rng.standard_normal((4, 64, 2)).astype(np.float32).astype(np.float64)
    thr1 = 1.5 * ndwt.band_gains([64], "db2", 2, pres_l2_norm=1)
    thr1[0] = 0.0
    p = ndwt.Plan([64], ["db2"], torch.float32, False, True, "reference", max_level=2, inner=4, howmany=2)
    want = np.zeros_like(xi)
    for ch in range(4):
        for j in range(2):
            want[ch, :, j] = _nd_oracle(xi[ch, :, j], ["db2"], 2, thr1)
    close(run(p, xi, np.float32, torch.float32, 2, thr1, 2), want, "interleaved")


def test_the_classes_take_a_threshold_per_band():
    n, K, level = 384, 4, 3
    x = signals("f64", n, K, "classes")
    w = ndwt.nd_dwt_1D("db4", n, "batch", K, "pres_l2_norm", 1)
    g = w.band_gains(level)
    assert g.shape == (1 + level,) and np.allclose(g, ndwt.band_gains([n], "db4", level, pres_l2_norm=1))
    thr = 1.5 * g
    thr[0] = 0.0
    xg = torch.from_numpy(np.ascontiguousarray(x.T)).cuda().T
    c = oracle_coefs(x, "db4", level)
    with ndwt.kernel_trace() as recs:
        d = w.denoise(xg, level, thr)
    fams = [r.family for r in recs]
    assert fams == ["Den1C"] or fams.count("shrink_kernel") == level, recs
    want = oracle_rec(np_shrink_bands(c, thr, False), "db4")
    assert tuple(d.shape) == (n, K) and np.abs(d.cpu().numpy() - want).max() <= 20 * TOL["double"] * max(np.abs(want).max(), 1.0)
    y = w.dec(xg, level)
    with ndwt.kernel_trace() as recs:
        s = w.shrink(y, torch.from_numpy(thr), "soft")
    assert [r.family for r in recs] == ["shrink_kernel"] * level
    assert tuple(s.shape) == (n, K, 1 + level) and np.abs(s.cpu().numpy() - np_shrink_bands(c, thr, False)).max() <= 20 * TOL["double"] * np.abs(c).max()
    assert torch.equal(s[..., 0], y[..., 0])
    with ndwt.kernel_trace() as recs:                         # a scalar takes exactly today's call
        w.denoise(xg, level, 0.5)
    assert [r.family for r in recs] == ["Fwd1C"] + ["shrink_kernel"] * level + ["Inv1C"]
    with pytest.raises(ValueError, match="4 values, one per band"):
        w.denoise(xg, level, [0.1, 0.2])


@functools.lru_cache(maxsize=None)
def cover(kind):
    """every (L, NLEV) of the kind with K = 3 signals of WX + 32 scalars, asked for with 11 / 11: what ran, checked against the general route"""
    prec, cplx, rdt, ndt, tdt, T, comp, tol = types(kind)
    ran = set()
    for L in (2, 4, 6, 8):
        wn = f"db{L // 2}"
        for level in (1, 2, 3, 4):
            K, row = 3, tile_width(kind, L, level) + 32
            n = row // comp
            x = signals(kind, n, K, ("cover", kind, L, level))
            thr = 1.5 * ndwt.band_gains([n], wn, level, pres_l2_norm=1)
            xb, ob, og = to_dev(x, kind), Buf(n * K, tdt), Buf(n * K, tdt)
            with ndwt.kernel_trace() as recs:
                plan(kind, n, wn, level, K, 11).denoise_bands(xb.ptr(), ob.ptr(), level, thr, False, stream())
            plan(kind, n, wn, level, K, 9).denoise_bands(xb.ptr(), og.ptr(), level, thr, False, stream())
            torch.cuda.synchronize()
            if (T, comp, L, level) in INSTANCES:
                ran.add(check_den1c(recs, kind, L, level, K, row, f"cover {kind} L {L} x {level}"))
            else:                                             # an instance that left the table: the general route, silently
                check_general(recs, thr, f"cover {kind} L {L} x {level}")
            dg = np.abs(from_dev(ob, (n, K)) - from_dev(og, (n, K))).max()
            assert dg <= 4 * tol * np.abs(x).max(), (kind, L, level, dg)
            assert ob.clean_outside()
    return frozenset(ran)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_instance_of_the_kind_runs_and_agrees_with_the_general_route(kind):
    assert cover(kind)


def test_every_instance_of_the_table_was_launched():
    """the coverage gate: each of the 61 entries of INSTANCES ran (and agreed with the general route)"""
    assert len(INSTANCES) == 61
    ran = set().union(*[cover(kind) for kind in KINDS])
    assert not (INSTANCES - ran), f"never launched: {sorted(INSTANCES - ran)}"


@pytest.mark.parametrize("dims,vi,route", [([64, 48], 0, "Inv2"), ([32, 32, 16], 0, "Den3"), ([64, 48], 11, "Inv2C")],
                         ids=["2d", "3d-den3", "2d-inv2c"])
def test_rec_is_the_same_before_and_after_a_denoise_on_the_plan(dims, vi, route):
    """ndwt_denoise's thresholding in the synthesis loads is an argument of its own rec, not state of the plan: rec(y) of the same plan
    gives the same bits before a denoise, after one (soft and hard), and after one that was refused (a negative threshold).  db2 at 2
    levels on the smallest shapes that have each shrinking synthesis route: the one-level 2-D kernels, Inv3Y behind Den3, Inv2C
    (variant inv = 11)."""
    s, level, nb = stream(), 2, 1 + 2 * (2 ** len(dims) - 1)
    p = ndwt.Plan(dims, ["db2"] * len(dims), torch.float32, False, True, "reference", max_level=level)
    if vi:
        p.set_variant(inv=vi)
    g = torch.Generator(device="cpu").manual_seed(5)
    vol = int(np.prod(dims))
    x = torch.randn(vol, generator=g, dtype=torch.float32).cuda()
    y, out = torch.empty(vol * nb, dtype=torch.float32, device="cuda"), torch.empty(vol, dtype=torch.float32, device="cuda")
    p.dec(x.data_ptr(), y.data_ptr(), level, s)

    def rec():
        r = torch.empty(vol, dtype=torch.float32, device="cuda")
        p.rec(y.data_ptr(), r.data_ptr(), level, s)
        torch.cuda.synchronize()
        return r

    before = rec()
    assert float((before - x).abs().max()) <= 50 * TOL["single"] * float(x.abs().max())   # (it IS the reconstruction)
    for hard in (False, True):
        with ndwt.kernel_trace() as recs:
            p.denoise(x.data_ptr(), out.data_ptr(), level, 0.5, hard, s)
        fams = [r.family for r in recs]
        assert any(f.startswith(route) for f in fams) and "shrink_kernel" not in fams, recs   # the thresholding was in the loads
        assert float((out - x).abs().max()) > 0.1                                 # ... and it thresholded
        assert torch.equal(rec(), before), (dims, vi, hard)
    with pytest.raises(ndwt.NdwtError, match="threshold must be >= 0"):
        p.denoise(x.data_ptr(), out.data_ptr(), level, -1.0, False, s)
    assert torch.equal(rec(), before), (dims, vi, "refused")
