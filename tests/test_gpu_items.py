"""The per-item calls on the device: ndwt_band_select_items, ndwt_estimate_sigma*_items, ndwt_shrink_bands_items, ndwt_denoise_bands_items
and the classes' per_item options and 2-D thresholds.

A selection and a shrink need no transform: the coefficient array is ARBITRARY DATA written by the test (tests/items_cases.py: item j a
draw of its own scaled by j + 1, item 1 all-equal, item 2 with a NaN), the plan only supplies the sizes, the items and the data kind.
Every array lies between guard words, and what a call must not write is compared with its copy afterwards.

  select    batch 5 x 96, batch 5 x 37 (db1), batch 3 x 4096, stack 3 x (8 x 12), interleaved inner = 3 / howmany = 2 / n = 100, an
            unbatched 64 x 64 plan (one item: bit-equal to band_select), a band behind a pitch off the 16- / 32-byte groups; float,
            double, complex64, complex128; both forced routes (variant 9: the loop, 11: one launch).  Real values bit-equal to numpy per
            item and between the routes, complex values by the counting check.  Route 11 is exactly one ItemSelect launch on `items`
            workgroups with the expected COMP / VEC; route 9 is items x passes BandHist + BandPick pairs and nothing else
  sigma     estimate_sigma(x, per_item=True) on a batch of 8 x 256 and a 2-D stack of 4 x 32 x 32; float, double, complex64; db4
            (pres_l2_norm) and db1; item j's noise 0.1 (j + 1).  Reference: the formula of include/ndwt.h on the ORACLE's level-1 last band
            of item j; |sigma_j - ref_j| <= 2 TOL max|c_j| / (0.6745 g) (a median moves by no more than the coefficients do: the bound of
            tests/test_gpu_select.py); strictly increasing in j; the pooled estimate lies between the smallest and the largest
  shrink    shrink_bands_items against shrink_bands of the same plan with row j, on item j's blocks, bit for bit (shrink_kernel is
            element-wise: its values on a block do not depend on what else the launch covers); batch, 2-D stack, 3-D complex stack,
            interleaved; packed, the plan's pitch, a pitch off the groups.  One ShrinkItems launch; an all-zero table launches nothing;
            a zero entry leaves exactly its block alone
  denoise   one launch: a batched 1-D plan with variant 11 / 11 (and by default) runs ONE Den1C record with ROWTHR = True on
            ceil(K nseg / 4) workgroups, on the shapes of tests/test_emulated_den1r.py; row j bit-identical to denoise_bands(x, thr[j]) of
            the same plan (the uniform Den1C), soft and hard; soft against the fp64 oracle at 20 TOL (the bound of
            tests/test_gpu_denoise_bands.py); a NaN signal in row 1 does not reach rows 0 and 2; x == out, `out` off by 4 bytes, level 5,
            a-trous and db5 take the general route silently, by trace and by value
            general route: the trace of denoise_bands' general route with its shrink_kernel launches replaced by ONE ShrinkItems; item j
            bit-identical to denoise_bands(x, thr[j]) on the same route
  stream    two denoise_bands_items calls with different tables back to back on one stream, no synchronisation in between: each output
            is its own table's
  classes   universal_thresholds(per_item=True), denoise / shrink with a [K, bands] array, a [K + 1, bands] array raises, the scalar and
            1-D forms are what they were
  refusals  name the item and the band (or the argument), and launch nothing
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
import ndwt_oracle as orc
import ndwt_spatial as orc_c
from items_cases import build_items_shim, check_items, item_ranks, items_band
from select_cases import KINDS, build_shim

pytestmark = pytest.mark.gpu

TOL = {"double": 1e-12, "single": 2e-6}                       # tests/test_gpu_parity.py
GUARD = 8                                                     # scalars before and after an array (32 / 64 bytes: the alignment stays)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory)


@pytest.fixture(scope="module")
def ishim(tmp_path_factory):
    return build_items_shim(tmp_path_factory)


def stream():
    return torch.cuda.current_stream().cuda_stream


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def torch_real(kind):
    return torch.float32 if KINDS[kind][0] == np.float32 else torch.float64


def tname(kind):
    return "float" if KINDS[kind][0] == np.float32 else "double"


# (plan, items, elements of one item, filtered axes): the plan kinds of the per-item calls
def make_plan(kind, shape):
    rdt, cplx = torch_real(kind), KINDS[kind][1]
    if shape == "batch-5x96":
        return ndwt.Plan([96], ["db2"], rdt, cplx, max_level=3, howmany=5), 5, 96, 1
    if shape == "batch-5x37":
        return ndwt.Plan([37], ["db1"], rdt, cplx, max_level=3, howmany=5), 5, 37, 1
    if shape == "batch-3x4096":
        return ndwt.Plan([4096], ["db2"], rdt, cplx, max_level=2, howmany=3), 3, 4096, 1
    if shape == "stack-3x8x12":
        return ndwt.Plan([8, 12, 3], ["db1", "db1", None], rdt, cplx, max_level=2, axes=(0, 1)), 3, 96, 2
    if shape == "stack-3x16x16":
        return ndwt.Plan([16, 16, 3], ["db2", "db2", None], rdt, cplx, max_level=2, axes=(0, 1)), 3, 256, 2
    if shape == "stack-2x8x8x8":
        return ndwt.Plan([8, 8, 8, 2], ["db1", "db1", "db1", None], rdt, cplx, max_level=1, axes=(0, 1, 2)), 2, 512, 3
    if shape == "inner-3":
        return ndwt.Plan([100], ["db2"], rdt, cplx, max_level=3, inner=3, howmany=2), 2, 300, 1
    if shape == "one-64x64":
        return ndwt.Plan([64, 64], ["db2", "db2"], rdt, cplx, max_level=1), 1, 4096, 2
    raise ValueError(shape)


class Coefs:
    """`nb` bands of `vol` scalars at `bs` scalars from one to the next between GUARD scalars of filler; on the device, with its host copy"""

    def __init__(self, rdt, vol, nb, bs, seed, scale=100):
        self.bs, self.vol, self.nb = bs, vol, nb
        self.host = (np.random.default_rng(seed).standard_normal(GUARD + nb * bs + GUARD) * scale).astype(rdt)
        self.dev = None

    def band(self, b):
        return self.host[GUARD + b * self.bs:GUARD + b * self.bs + self.vol]

    def upload(self):
        self.dev = torch.from_numpy(self.host).cuda()
        self.ptr = self.dev.data_ptr() + GUARD * self.host.itemsize
        return self

    def band_addr(self, b):
        return self.ptr + b * self.bs * self.host.itemsize

    def now(self):
        return self.dev.cpu().numpy()

    def unchanged(self):
        return self.now().tobytes() == self.host.tobytes()


# ------------------------------------------------------------------------------------------------ select
# (id, plan shape, level, band, band pitch in elements or 0 = packed)
SELECT_SHAPES = [
    ("batch-5x96", "batch-5x96", 3, 1, 0),
    ("batch-5x37", "batch-5x37", 2, 1, 0),
    ("batch-3x4096", "batch-3x4096", 1, 1, 0),
    ("stack-3x8x12", "stack-3x8x12", 1, 3, 0),
    ("inner-3", "inner-3", 2, 2, 0),
    ("one-64x64", "one-64x64", 1, 3, 0),
    ("batch-5x96-pitched", "batch-5x96", 3, 1, 481),
]
SELECT_CASES = [(f"{kind}-{sid}", kind, sid, shape, level, band, pitch) for kind in KINDS for sid, shape, level, band, pitch in SELECT_SHAPES]


@pytest.mark.parametrize("cid,kind,sid,shape,level,band,pitch", SELECT_CASES, ids=[c[0] for c in SELECT_CASES])
def test_select_items_is_exact_per_item_on_both_routes(shim, cid, kind, sid, shape, level, band, pitch):
    rdt, cplx = KINDS[kind]
    comp, sb = (2 if cplx else 1), np.dtype(rdt).itemsize
    plan, items, N, axes = make_plan(kind, shape)
    assert plan.items == items
    data = items_band(kind, items, N, zlib.crc32(cid.encode()))
    nb = ndwt.num_bands(axes, level)
    c = Coefs(rdt, items * N * comp, nb, (pitch or items * N) * comp, 5)
    c.band(band)[:] = data.reshape(-1)
    c.upload()
    sets = item_ranks(N)
    vec = bool(shim.sel_select_vec(c.band_addr(band), N * comp, sb))
    assert vec == (sid in ("batch-5x96", "batch-3x4096", "stack-3x8x12", "inner-3", "one-64x64")), (sid, vec)
    passes = shim.sel_select_passes(int(sb == 8))
    got = {}
    for route in (11, 9):
        plan.set_variant(inv=route)
        with ndwt.kernel_trace() as recs:
            got[route] = [plan.band_select_items(c.ptr, level, band, ks, stream(), band_pitch=pitch) for ks in sets]
        for ks, g in zip(sets, got[route]):
            check_items(kind, data, ks, g, f"{cid} route {route}")
        if route == 11:
            assert len(recs) == len(sets), recs
            for r in recs:
                assert r.family == "ItemSelect" and r.params == {"T": tname(kind), "COMP": comp, "VEC": vec, "AGG": 2}, r
                assert r.grid == (items, 1, 1) and r.block == (256, 1, 1), r
        else:
            grid = int(shim.sel_select_grid(N * comp, comp, int(vec), cus(), 0))
            assert len(recs) == 2 * passes * items * len(sets), (len(recs), passes, items)
            for i, r in enumerate(recs):
                if i % 2 == 0:
                    assert r.family == "BandHist" and r.params == {"T": tname(kind), "COMP": comp, "VEC": vec, "AGG": 2}, r
                    assert r.grid == (grid, 1, 1) and r.block == (256, 1, 1), (r, grid)
                else:
                    assert r.family == "BandPick" and r.params == {"T": tname(kind)} and r.grid == (1, 1, 1), r
    if not cplx:                                                  # (complex: each kernel rounds its own magnitudes)
        for a, b in zip(got[11], got[9]):
            assert a.tobytes() == b.tobytes(), (a, b)
    if items == 1:                                                # an unbatched plan is one item: the band-wide call, bit for bit
        plan.set_variant(inv=0)
        for ks, g9, g11 in zip(sets, got[9], got[11]):
            one = plan.band_select(c.ptr, level, band, ks, stream(), band_pitch=pitch)
            assert one.tobytes() == g9[0].tobytes() and (cplx or one.tobytes() == g11[0].tobytes())
            assert plan.band_select_items(c.ptr, level, band, ks, stream(), band_pitch=pitch).tobytes() == g9.tobytes()   # (one item < CUs: the loop)
    assert c.unchanged()                                          # the band, its neighbours and the guard words


def test_select_items_by_default_takes_the_route_that_was_measured_to_win(ishim):
    """unasked (select_items_route): as many signals as the device has compute units, or 8 signals of up to 2^14 scalars:
    one ItemSelect launch; 7 signals, or 8 of one group of 4 more: the loop"""
    for items, n in ((cus(), 64), (8, 1 << 14), (7, 64), (8, (1 << 14) + 4)):
        plan = ndwt.Plan([n], ["db1"], torch.float32, False, max_level=1, howmany=items)
        data = items_band("f32", items, n, items + n)
        c = Coefs(np.float32, items * n, 2, items * n, 9)
        c.band(1)[:] = data.reshape(-1)
        c.upload()
        ks = item_ranks(n)[0]
        with ndwt.kernel_trace() as recs:
            got = plan.band_select_items(c.ptr, 1, 1, ks, stream())
        check_items("f32", data, ks, got, f"{items} x {n}")
        one = bool(ishim.sel_items_one_launch(n, items, cus(), 0))
        assert one == ((items, n) in ((cus(), 64), (8, 1 << 14)))
        if one:
            assert [r.family for r in recs] == ["ItemSelect"] and recs[0].grid == (items, 1, 1)
        else:
            assert len(recs) == 2 * 3 * items and {r.family for r in recs} == {"BandHist", "BandPick"}
        assert c.unchanged()


# ------------------------------------------------------------------------------------------------ sigma
SIGMA_OBJECTS = {
    "1d-batch-8x256": (lambda wn, l2, prec: ndwt.nd_dwt_1D(wn, 256, "batch", 8, "pres_l2_norm", l2, "precision", prec), [256], 8),
    "2d-stack-4x32x32": (lambda wn, l2, prec: ndwt.nd_dwt_2D(wn, [32, 32], "stack", 4, "pres_l2_norm", l2, "precision", prec), [32, 32], 4),
}
SIGMA_CASES = [(f"{obj}-{kind}-{wn}", obj, kind, wn, l2) for obj in SIGMA_OBJECTS for kind in ("f32", "f64", "c64") for wn, l2 in (("db4", 1), ("db1", 0))]
_SIGMA = {}


def sigma_case(cid, obj, kind, wn, l2):
    """(x in MATLAB shape at the kind's precision, the oracle's level-1 last band [.., K], its gain), made once.  A median of 256
    coefficients scatters by some 7 %, more than the step from 0.7 to 0.8: the draw is the first of the case's seeds whose REFERENCE
    medians (the oracle's, in double) increase from item to item by at least 1 % -- a margin the device's rounding cannot close"""
    if cid not in _SIGMA:
        rdt, cplx = KINDS[kind]
        _, sizes, K = SIGMA_OBJECTS[obj]
        grid = np.meshgrid(*[np.linspace(0, 1, n, endpoint=False) for n in sizes], indexing="ij")
        smooth = sum(np.sin(2 * np.pi * (a + 1) * g) for a, g in enumerate(grid))[..., None] * np.linspace(1, 2, K)
        noise = 0.1 * (np.arange(K) + 1)                          # item j's noise: 0.1 (j + 1), a draw of its own
        g = float(ndwt.band_gains(sizes, wn, 1, pres_l2_norm=l2)[-1])

        def last_band(v):
            d = lambda u: orc.spatial_dec(u, [wn] * len(sizes), 1, l2)[..., -1]
            return d(v.real) + 1j * d(v.imag) if cplx else d(v)
        for attempt in range(64):
            rng = np.random.default_rng(zlib.crc32(cid.encode()) + attempt)
            x = smooth + noise * rng.standard_normal(sizes + [K])
            if cplx:
                x = x + 1j * (0.5 * smooth + noise * rng.standard_normal(sizes + [K]))
            x = x.astype((np.complex64 if rdt == np.float32 else np.complex128) if cplx else rdt)
            xd = x.astype(np.complex128 if cplx else np.float64)
            c = np.stack([last_band(xd[..., j]) for j in range(K)], axis=-1)
            med = np.median(np.abs(c).reshape(-1, K), axis=0)
            if (np.diff(med) >= 0.01 * med[1:]).all():
                break
        else:
            raise AssertionError(f"{cid}: no draw with increasing medians")
        _SIGMA[cid] = (x, c, g)
    return _SIGMA[cid]


@pytest.mark.parametrize("cid,obj,kind,wn,l2", SIGMA_CASES, ids=[c[0] for c in SIGMA_CASES])
def test_sigma_per_item_is_the_formula_on_the_oracles_last_band_of_each_item(cid, obj, kind, wn, l2):
    rdt, cplx = KINDS[kind]
    prec = "single" if rdt == np.float32 else "double"
    x, c, g = sigma_case(cid, obj, kind, wn, l2)
    K = x.shape[-1]
    w = SIGMA_OBJECTS[obj][0](wn, l2, prec)
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda().permute(*reversed(range(x.ndim)))
    const = 1.1774100225154747 if cplx else 0.6744897501960817
    ref = np.array([float(np.median(np.abs(c[..., j]))) / const / g for j in range(K)])
    bound = np.array([2 * TOL[prec] * float(np.abs(c[..., j]).max()) / (0.6745 * g) for j in range(K)])
    s = w.estimate_sigma(xt, per_item=True)
    s_c = w.estimate_sigma_coef(w.dec(xt, 2), per_item=True)
    print(f"{cid}: per item {s!r}, from dec(x, 2) {s_c!r}, reference {ref!r}; bounds {bound!r}, gain {g:.6g}")
    assert s.shape == (K,) and s_c.shape == (K,)
    assert (np.abs(s - ref) <= bound).all() and (np.abs(s_c - ref) <= bound).all()
    assert (np.diff(s) > 0).all() and (np.diff(ref) > 0).all()   # item j's noise is 0.1 (j + 1)
    # the pooled estimate is what it was: the formula on all items' coefficients together, between the extremes
    pooled = w.estimate_sigma(xt)
    pref = float(np.median(np.abs(c))) / const / g
    assert isinstance(pooled, float) and abs(pooled - pref) <= 2 * TOL[prec] * float(np.abs(c).max()) / (0.6745 * g)
    assert s.min() < pooled < s.max()
    # band_median per item: the same medians, before the division
    y = w.dec(xt, 1)
    med = w.band_median(y, y.shape[-1] - 1, per_item=True)
    assert med.shape == (K,) and (np.abs(med - ref * const * g) <= 2 * TOL[prec] * np.abs(c).reshape(-1, K).max(axis=0)).all()
    # universal thresholds per item: sqrt(2 ln N) sigma_j gains, column 0 zero -- and denoise takes them as they are
    sizes = SIGMA_OBJECTS[obj][1]
    nb = ndwt.num_bands(len(sizes), 2)
    thr = w.universal_thresholds(xt, 2, per_item=True)
    want = np.sqrt(2 * np.log(float(np.prod(sizes)))) * np.outer(s, w.band_gains(2))
    want[:, 0] = 0.0
    assert thr.shape == (K, nb) and (thr[:, 0] == 0).all() and np.allclose(thr, want, rtol=1e-12, atol=0)
    assert np.allclose(w.universal_thresholds(xt, 2, k=3.0, per_item=True)[:, 1:], 3.0 * np.outer(s, w.band_gains(2))[:, 1:], rtol=1e-12, atol=0)
    one = w.universal_thresholds(xt, 2)                          # the pooled form is what it was
    assert one.shape == (nb,) and np.allclose(one[1:], np.sqrt(2 * np.log(float(np.prod(sizes)))) * pooled * w.band_gains(2)[1:], rtol=1e-12, atol=0)
    out = w.denoise(xt, 2, thr)
    assert out.shape == xt.shape and bool(torch.isfinite(torch.view_as_real(out) if cplx else out).all())
    assert float((out - xt).abs().max()) > 0                      # the thresholds did something
    with pytest.raises(ValueError, match="one per band"):
        w.denoise(xt, 2, np.zeros((K + 1, nb)))


# ------------------------------------------------------------------------------------------------ shrink
# (plan shape, kinds, level)
SHRINK_SHAPES = [
    ("batch-5x96", ("f32", "c64", "f64", "c128"), 3),
    ("stack-3x16x16", ("f32", "f64"), 2),
    ("stack-2x8x8x8", ("c64",), 1),
    ("inner-3", ("f32", "c128"), 2),
]
SHRINK_CASES = [(f"{kind}-{shape}-{lay}", kind, shape, level, lay) for shape, kinds, level in SHRINK_SHAPES for kind in kinds
                for lay in ("packed", "plan-pitch", "odd-pitch")]


def table(items, nb, seed):
    """thresholds in quarters (exact in either precision), column 0 and a few other entries zero"""
    t = np.round(np.random.default_rng(seed).random((items, nb)) * 6 + 1) / 4
    t[:, 0] = 0.0
    t[0, nb - 1] = 0.0
    t[items - 1, 1] = 0.0 if nb > 2 else t[items - 1, 1]
    return t


def check_shrink_trace(recs, ishim, kind, comp, vec, n_item, nb, items):
    assert len(recs) == 1 and recs[0].family == "ShrinkItems", recs
    r = recs[0]
    assert r.params == {"T": tname(kind), "COMP": comp, "VEC": vec}, r
    chunks = int(ishim.sel_shrink_items_chunks(n_item, comp, int(vec), nb, items, cus()))
    assert r.grid == (nb * items * chunks, 1, 1) and r.block == (256, 1, 1), (r, chunks)


@pytest.mark.parametrize("cid,kind,shape,level,lay", SHRINK_CASES, ids=[c[0] for c in SHRINK_CASES])
def test_shrink_items_is_shrink_bands_on_every_item_with_its_own_row(ishim, cid, kind, shape, level, lay):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    plan, items, N, axes = make_plan(kind, shape)
    nb = ndwt.num_bands(axes, level)
    vol, n = items * N * comp, N * comp
    pitch = {"packed": 0, "plan-pitch": plan.band_pitch(), "odd-pitch": items * N + 1}[lay]
    bs = (pitch or items * N) * comp
    thr = table(items, nb, zlib.crc32(cid.encode()))
    for hard in (False, True):
        c = Coefs(rdt, vol, nb, bs, 21 + hard, scale=2).upload()
        with ndwt.kernel_trace() as recs:
            plan.shrink_bands_items(c.ptr, level, thr, hard, stream(), band_pitch=pitch)
        vec = c.ptr % (4 * c.host.itemsize) == 0 and bs % 4 == 0 and n % 4 == 0
        assert vec == (lay != "odd-pitch" and bs % 4 == 0), (lay, bs, vec)
        check_shrink_trace(recs, ishim, kind, comp, vec, n, nb, items)
        got = c.now()
        want = c.host.copy()
        for j in range(items):                                    # row j through the band-wide call: item j's blocks are the reference
            ref = Coefs(rdt, vol, nb, bs, 21 + hard, scale=2).upload()
            plan.shrink_bands(ref.ptr, level, thr[j], hard, stream(), band_pitch=pitch)
            r = ref.now()
            for b in range(nb):
                lo = GUARD + b * bs + j * n
                want[lo:lo + n] = r[lo:lo + n]
                if thr[j, b] == 0:
                    assert r[lo:lo + n].tobytes() == c.host[lo:lo + n].tobytes()
        assert got.tobytes() == want.tobytes(), cid               # every block, the padding of a pitch and the guard words
        assert (got != c.host).any()
    # an all-zero table launches nothing and leaves every byte
    c = Coefs(rdt, vol, nb, bs, 23, scale=2).upload()
    with ndwt.kernel_trace() as recs:
        plan.shrink_bands_items(c.ptr, level, np.zeros((items, nb)), False, stream(), band_pitch=pitch)
    assert recs == [] and c.unchanged()
    # one non-zero entry: exactly that (item, band) block changes
    one = np.zeros((items, nb))
    one[items - 1, nb - 1] = 0.75
    plan.shrink_bands_items(c.ptr, level, one, False, stream(), band_pitch=pitch)
    diff = c.now() != c.host
    lo = GUARD + (nb - 1) * bs + (items - 1) * n
    assert diff[lo:lo + n].any() and not diff[:lo].any() and not diff[lo + n:].any()


# ------------------------------------------------------------------------------------------------ denoise
DENOISE_CASES = [(f"{kind}-{shape}", kind, shape, level) for shape, kinds, level in SHRINK_SHAPES for kind in kinds]


def signal(kind, n_elements, seed):
    rdt, cplx = KINDS[kind]
    return np.random.default_rng(seed).standard_normal(n_elements * (2 if cplx else 1)).astype(rdt)


class Arr:
    """n scalars between GUARD scalars of zeros, on the device"""

    def __init__(self, host):
        self.n = host.size
        self.t = torch.zeros(self.n + 2 * GUARD, dtype=torch.from_numpy(host[:1]).dtype, device="cuda")
        self.t[GUARD:GUARD + self.n].copy_(torch.from_numpy(host).cuda())
        self.ptr = self.t.data_ptr() + GUARD * host.itemsize

    def get(self):
        return self.t[GUARD:GUARD + self.n].cpu().numpy()

    def clean_outside(self):
        return float(self.t[:GUARD].abs().sum()) == 0 and float(self.t[GUARD + self.n:].abs().sum()) == 0


@pytest.mark.parametrize("cid,kind,shape,level", DENOISE_CASES, ids=[c[0] for c in DENOISE_CASES])
def test_denoise_items_is_the_general_route_with_one_shrink_launch(ishim, cid, kind, shape, level):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    plan, items, N, axes = make_plan(kind, shape)
    plan.set_variant(fwd=9, inv=9)                                # the batched plan: one launch per level both ways, no Den1C -- for both calls
    nb = ndwt.num_bands(axes, level)
    thr = table(items, nb, zlib.crc32(cid.encode()))
    xh = signal(kind, items * N, 31)
    for hard in (False, True):
        x, out = Arr(xh), Arr(np.zeros_like(xh))
        with ndwt.kernel_trace() as recs:
            plan.denoise_bands_items(x.ptr, out.ptr, level, thr, hard, stream())
        got = out.get()
        assert out.clean_outside() and x.get().tobytes() == xh.tobytes()
        fams = [r.family for r in recs]
        assert fams.count("ShrinkItems") == 1 and "shrink_kernel" not in fams and "Den1C" not in fams, fams
        for j in range(items):
            o = Arr(np.zeros_like(xh))
            with ndwt.kernel_trace() as ref_recs:
                plan.denoise_bands(x.ptr, o.ptr, level, thr[j], hard, stream())
            rf = [r.family for r in ref_recs]
            i0, cnt = rf.index("shrink_kernel"), rf.count("shrink_kernel")
            assert cnt == int((thr[j] != 0).sum()) and rf[i0:i0 + cnt] == ["shrink_kernel"] * cnt
            assert fams == rf[:i0] + ["ShrinkItems"] + rf[i0 + cnt:], (fams, rf)   # between the dec and the rec, and nothing else changed
            lo = j * N * comp
            assert got[lo:lo + N * comp].tobytes() == o.get()[lo:lo + N * comp].tobytes(), (cid, hard, j)
    k = fams.index("ShrinkItems")
    r = recs[k]
    bs = plan.band_pitch() * comp
    vec = bs % 4 == 0 and (N * comp) % 4 == 0                     # (the plan's scratch is aligned)
    assert r.params == {"T": tname(kind), "COMP": comp, "VEC": vec}, r
    assert r.grid == (nb * items * int(ishim.sel_shrink_items_chunks(N * comp, comp, int(vec), nb, items, cus())), 1, 1), r


# ------------------------------------------------------------------------------------------------ denoise, one launch
def den1_tile_width(kind, L, nlev):
    """Den1C::WX: the lanes valid after nlev analysis and nlev synthesis levels, in whole 128-byte lines"""
    rdt, cplx = KINDS[kind]
    ew, lpl = (2 if cplx else 1), (8 if rdt == np.float32 else 4)
    GLa, GRa = ((L // 2 - 1) * ew + 3) // 4, ((L // 2) * ew + 3) // 4
    return 4 * ((64 - nlev * 2 * (GLa + GRa)) // lpl * lpl)


# the shapes of tests/test_emulated_den1r.py: (id, kind, wavelet, taps, levels, elements of a row)
ONE_LAUNCH = [
    ("f32-db4-4-n416", "f32", "db4", 8, 4, 416),
    ("f32-db1-1-n16", "f32", "db1", 2, 1, 16),
    ("c64-db2-3-n200", "c64", "db2", 4, 3, 200),
    ("f64-db3-2-n300", "f64", "db3", 6, 2, 300),
]


def rows3(nlev, seed):
    """K = 3: row 0 all-zero thresholds, row 1 all non-zero, row 2 zero for some bands; eighths, exact in either precision"""
    thr = np.round(np.random.default_rng(seed).random((3, 1 + nlev)) * 4 + 1) / 8
    thr[0] = 0.0
    thr[2, 0] = 0.0
    thr[2, nlev] = 0.0
    return thr


def run_denoise(plan, xh, level, thr, hard, off=0, inplace=False):
    """(output scalars, trace) of denoise_bands_items (a 2-D thr) or denoise_bands (a 1-D thr); off: `out` that many scalars past its
    aligned place; inplace: out = x"""
    x = Arr(xh)
    o = x if inplace else Arr(np.zeros(xh.size + off, dtype=xh.dtype))
    optr = o.ptr + off * xh.itemsize
    with ndwt.kernel_trace() as recs:
        if np.ndim(thr) == 2:
            plan.denoise_bands_items(x.ptr, optr, level, thr, hard, stream())
        else:
            plan.denoise_bands(x.ptr, optr, level, thr, hard, stream())
    assert o.clean_outside()
    return o.get()[off:off + xh.size].copy(), recs


@pytest.mark.parametrize("cid,kind,wn,L,level,n", ONE_LAUNCH, ids=[c[0] for c in ONE_LAUNCH])
def test_denoise_items_of_a_batch_runs_in_one_launch_with_a_row_of_thresholds_per_signal(cid, kind, wn, L, level, n):
    """variant 11 / 11: one Den1C record with ROWTHR = True on ceil(K nseg / 4) workgroups; row j bit-identical to denoise_bands(x, thr[j])
    of the same plan (the uniform Den1C), soft and hard; soft against the fp64 oracle at 20 TOL max|x| (the bound of
    tests/test_gpu_denoise_bands.py); a NaN signal in row 1 does not reach rows 0 and 2"""
    rdt, cplx = KINDS[kind]
    prec = "single" if rdt == np.float32 else "double"
    comp, K = (2 if cplx else 1), 3
    plan = ndwt.Plan([n], [wn], torch_real(kind), cplx, True, max_level=level, howmany=K).set_variant(fwd=11, inv=11)
    thr = rows3(level, zlib.crc32(cid.encode()))
    xh = signal(kind, K * n, 81)
    row = n * comp
    nseg = -(-row // den1_tile_width(kind, L, level))
    for hard in (False, True):
        got, recs = run_denoise(plan, xh, level, thr, hard)
        assert len(recs) == 1 and recs[0].family == "Den1C", recs
        r = recs[0]
        assert r.params == {"T": tname(kind), "L": L, "NLEV": level, "EW": comp, "WPE": 4, "ROWTHR": True}, r
        assert r.grid == (-(-K * nseg // 4), 1, 1) and r.block == (256, 1, 1), (r, nseg)
        for j in range(K):
            one, urecs = run_denoise(plan, xh, level, thr[j], hard)
            assert len(urecs) == 1 and urecs[0].family == "Den1C" and urecs[0].params["ROWTHR"] is False, urecs
            assert got[j * row:(j + 1) * row].tobytes() == one[j * row:(j + 1) * row].tobytes(), (cid, hard, j)
        if not hard:
            soft = got
    if cid == "f32-db4-4-n416":
        assert nseg == 3 and (K * nseg) % 4 == 1                   # three waves of the last workgroup are clamped onto the last item
    g = soft.astype(np.float64)
    g = (g[0::2] + 1j * g[1::2]) if cplx else g
    xd = xh.astype(np.float64)
    xd = (xd[0::2] + 1j * xd[1::2]) if cplx else xd
    for j in range(K):
        sig = xd[j * n:(j + 1) * n]
        c = orc_c.spatial_dec(sig, [wn], level, 1, "reference")
        m = np.abs(c)
        for b in range(level + 1):
            if thr[j, b]:
                c[..., b] = c[..., b] * np.where(m[..., b] > thr[j, b], (m[..., b] - thr[j, b]) / np.where(m[..., b] > 0, m[..., b], 1.0), 0.0)
        err = float(np.abs(g[j * n:(j + 1) * n] - orc_c.spatial_rec(c, [wn], 1, "reference")).max())
        print(f"{cid} row {j}: max error {err:.3g}, bound {20 * TOL[prec] * float(np.abs(sig).max()):.3g}")
        assert err <= 20 * TOL[prec] * float(np.abs(sig).max()), (cid, j, err)
    bad = xh.copy()
    bad[row:2 * row] = np.nan
    g2, recs = run_denoise(plan, bad, level, thr, False)
    assert [r.family for r in recs] == ["Den1C"]
    for j in (0, 2):
        assert g2[j * row:(j + 1) * row].tobytes() == soft[j * row:(j + 1) * row].tobytes()


def test_what_the_one_launch_does_not_serve_takes_the_general_route_silently():
    """x == out, `out` off by 4 bytes, level 5, a-trous and db5: no Den1C, one ShrinkItems between the dec and the rec, and row j is
    denoise_bands(x, thr[j]) under the same condition (which takes its own general route), bit for bit"""
    n, K = 416, 3
    xh = signal("f32", K * n, 91)
    cases = [("x == out", "db4", 4, "reference", 0, True), ("out off by 4 bytes", "db4", 4, "reference", 1, False),
             ("level 5", "db4", 5, "reference", 0, False), ("a-trous", "db4", 3, "atrous", 0, False), ("db5", "db5", 3, "reference", 0, False)]
    for what, wn, level, dil, off, inplace in cases:
        plan = ndwt.Plan([n], [wn], torch.float32, False, True, dil, max_level=level, howmany=K).set_variant(fwd=11, inv=11)
        thr = rows3(level, 92 + level)
        got, recs = run_denoise(plan, xh, level, thr, False, off, inplace)
        fams = [r.family for r in recs]
        assert "Den1C" not in fams and fams.count("ShrinkItems") == 1 and "shrink_kernel" not in fams, (what, fams)
        k = fams.index("ShrinkItems")
        assert 0 < k < len(fams) - 1, (what, fams)
        for j in range(K):
            one, urecs = run_denoise(plan, xh, level, thr[j], False, off, inplace)
            uf = [r.family for r in urecs]
            assert "Den1C" not in uf, (what, uf)
            if thr[j].any():
                i0, cnt = uf.index("shrink_kernel"), uf.count("shrink_kernel")
                assert fams == uf[:i0] + ["ShrinkItems"] + uf[i0 + cnt:], (what, fams, uf)
            assert got[j * n:(j + 1) * n].tobytes() == one[j * n:(j + 1) * n].tobytes(), (what, j)
    # the same plan and data served: one launch (the control of the cases above)
    plan = ndwt.Plan([n], ["db4"], torch.float32, False, True, max_level=4, howmany=K).set_variant(fwd=11, inv=11)
    assert [r.family for r in run_denoise(plan, xh, 4, rows3(4, 96), False)[1]] == ["Den1C"]
    # ... and by default too (float: denoise1_default), while variant 9 in either slot switches it off
    plan = ndwt.Plan([n], ["db4"], torch.float32, False, True, max_level=4, howmany=K)
    assert [r.family for r in run_denoise(plan, xh, 4, rows3(4, 96), False)[1]] == ["Den1C"]
    plan.set_variant(fwd=9)
    assert "Den1C" not in [r.family for r in run_denoise(plan, xh, 4, rows3(4, 96), False)[1]]


def test_two_calls_back_to_back_on_one_stream_each_use_their_own_table():
    plan, items, N, axes = make_plan("f32", "stack-3x16x16")
    level, nb = 2, ndwt.num_bands(2, 2)
    t1, t2 = table(items, nb, 1), table(items, nb, 2) * 3
    xh = signal("f32", items * N, 51)
    x = Arr(xh)
    ref = []
    for t in (t1, t2):                                            # each table alone, synchronised
        o = Arr(np.zeros_like(xh))
        plan.denoise_bands_items(x.ptr, o.ptr, level, t, False, stream())
        torch.cuda.synchronize()
        ref.append(o.get())
    assert ref[0].tobytes() != ref[1].tobytes()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        o1, o2, o3 = Arr(np.zeros_like(xh)), Arr(np.zeros_like(xh)), Arr(np.zeros_like(xh))
        s.synchronize()
        plan.denoise_bands_items(x.ptr, o1.ptr, level, t1, False, s.cuda_stream)
        plan.denoise_bands_items(x.ptr, o2.ptr, level, t2, False, s.cuda_stream)
        plan.denoise_bands_items(x.ptr, o3.ptr, level, t1, False, s.cuda_stream)
        s.synchronize()
    assert o1.get().tobytes() == ref[0].tobytes() and o2.get().tobytes() == ref[1].tobytes() and o3.get().tobytes() == ref[0].tobytes()


# ------------------------------------------------------------------------------------------------ classes
def test_the_classes_take_a_table_and_keep_their_other_forms():
    K, n, level = 5, 96, 3
    w = ndwt.nd_dwt_1D("db2", n, "batch", K, "precision", "single")
    nb = ndwt.num_bands(1, level)
    rng = np.random.default_rng(61)
    xt = torch.from_numpy(rng.standard_normal((K, n)).astype(np.float32)).cuda().permute(1, 0)      # MATLAB shape [n, K]
    thr = table(K, nb, 62)
    plan = w._plan(False, level, xt.device)
    xk = xt.permute(1, 0).contiguous()
    for mode in ("soft", "hard"):
        ok = torch.empty_like(xk)
        plan.denoise_bands_items(xk.data_ptr(), ok.data_ptr(), level, thr, mode == "hard", stream())
        assert torch.equal(w.denoise(xt, level, thr, mode).permute(1, 0).contiguous(), ok)
        assert torch.equal(w.denoise(xt, level, torch.from_numpy(thr), mode).permute(1, 0).contiguous(), ok)
        # the 1-D and the scalar form are the plan's band-wide calls, as before
        plan.denoise_bands(xk.data_ptr(), ok.data_ptr(), level, thr[1], mode == "hard", stream())
        assert torch.equal(w.denoise(xt, level, thr[1], mode).permute(1, 0).contiguous(), ok)
        plan.denoise(xk.data_ptr(), ok.data_ptr(), level, 0.5, mode == "hard", stream())
        assert torch.equal(w.denoise(xt, level, 0.5, mode).permute(1, 0).contiguous(), ok)
        # shrink: a table against the plan call on a copy of the coefficients
        y = w.dec(xt, level)
        yk = y.permute(2, 1, 0).contiguous().clone()            # (a copy: y itself goes to the class call)
        plan.shrink_bands_items(yk.data_ptr(), level, thr, mode == "hard", stream())
        assert torch.equal(w.shrink(y, thr, mode).permute(2, 1, 0).contiguous(), yk)
        yk = y.permute(2, 1, 0).contiguous().clone()            # (a copy: y itself goes to the class call)
        plan.shrink_bands(yk.data_ptr(), level, thr[2], mode == "hard", stream())
        assert torch.equal(w.shrink(y, thr[2], mode).permute(2, 1, 0).contiguous(), yk)
    for bad in (np.zeros((K + 1, nb)), np.zeros((K, nb + 1))):
        with pytest.raises(ValueError, match="one per band"):
            w.denoise(xt, level, bad)
        with pytest.raises(ValueError, match="one per band"):
            w.shrink(w.dec(xt, level), bad)
    with pytest.raises(ValueError, match="array of thresholds expected"):
        plan.denoise_bands_items(xk.data_ptr(), ok.data_ptr(), level, np.zeros((K + 1, nb)), False, stream())
    with pytest.raises(ValueError, match="array of thresholds expected"):
        plan.shrink_bands_items(xk.data_ptr(), level, np.zeros(K * nb), False, stream())


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_names_its_argument_and_launches_nothing():
    plan, items, N, axes = make_plan("f32", "batch-5x96")
    level, nb = 2, 3
    c = Coefs(np.float32, items * N, nb, items * N, 71).upload()
    x, out = Arr(signal("f32", items * N, 72)), Arr(np.zeros(items * N, dtype=np.float32))
    lib = ndwt.lib()
    err = lambda: lib.ndwt_last_error().decode()
    dp = ctypes.POINTER(ctypes.c_double)
    k = (ctypes.c_int64 * 5)(0, 1, 2, 3, 4)
    v = (ctypes.c_double * 20)(*[-1.0] * 20)
    s = (ctypes.c_double * 5)(*[-1.0] * 5)
    with ndwt.kernel_trace() as recs:
        for j, b, val in ((0, 0, -1.0), (3, 2, float("nan")), (4, 1, -0.0 - 1e-300), (2, 0, float("-inf"))):
            t = np.ones((items, nb))
            t[j, b] = val
            tp = t.ctypes.data_as(dp)
            for rc in (lib.ndwt_shrink_bands_items(plan._h, c.ptr, 0, level, tp, 0, None), lib.ndwt_denoise_bands_items(plan._h, x.ptr, out.ptr, level, tp, 0, None)):
                assert rc == 1 and f"item {j}, band {b}" in err(), (j, b, rc, err())
        t = np.ones((items, nb))
        tp = t.ctypes.data_as(dp)
        assert lib.ndwt_shrink_bands_items(plan._h, c.ptr, 0, level, None, 0, None) == 1 and "null thresholds" in err()
        assert lib.ndwt_denoise_bands_items(plan._h, x.ptr, out.ptr, level, None, 0, None) == 1 and "null thresholds" in err()
        assert lib.ndwt_shrink_bands_items(plan._h, None, 0, level, tp, 0, None) == 1 and "null data pointer" in err()
        assert lib.ndwt_denoise_bands_items(plan._h, None, out.ptr, level, tp, 0, None) == 1 and "null data pointer" in err()
        assert lib.ndwt_denoise_bands_items(plan._h, x.ptr, None, level, tp, 0, None) == 1 and "null data pointer" in err()
        assert lib.ndwt_shrink_bands_items(plan._h, c.ptr, 0, level, tp, 2, None) == 1 and "mode" in err()
        assert lib.ndwt_shrink_bands_items(plan._h, c.ptr, 0, 4, tp, 0, None) == 1 and "level 4" in err()
        assert lib.ndwt_shrink_bands_items(plan._h, c.ptr, items * N - 1, level, tp, 0, None) == 1 and "pitch" in err()
        # the select: the refusals of ndwt_band_select, the ranks inside ONE item
        sel = lambda *a: lib.ndwt_band_select_items(plan._h, *a, None)
        for args, word in (((None, 0, level, 1, 1, k, v), "y_dev"), ((c.ptr, 0, level, 1, 1, None, v), "(k)"), ((c.ptr, 0, level, 1, 1, k, None), "values"),
                           ((c.ptr, 0, level, -1, 1, k, v), "band -1"), ((c.ptr, 0, level, 3, 1, k, v), "band 3"), ((c.ptr, 0, level, 1, 0, k, v), "nk = 0"),
                           ((c.ptr, 0, level, 1, 5, k, v), "nk = 5"), ((c.ptr, 0, 4, 1, 1, k, v), "level 4"), ((c.ptr, items * N - 1, level, 1, 1, k, v), "pitch")):
            assert sel(*args) == 1 and word in err(), (word, err())
        for bad in (-1, N, items * N - 1, 1 << 40):               # a rank of the pooled band is outside one item
            kk = (ctypes.c_int64 * 2)(0, bad)
            assert sel(c.ptr, 0, level, 1, 2, kk, v) == 1 and "k[1]" in err() and str(bad) in err() and "one item" in err(), err()
        assert lib.ndwt_estimate_sigma_coef_items(plan._h, None, 0, level, s, None) == 1 and "y_dev" in err()
        assert lib.ndwt_estimate_sigma_coef_items(plan._h, c.ptr, 0, level, None, None) == 1 and "sigma" in err()
        assert lib.ndwt_estimate_sigma_coef_items(plan._h, c.ptr, 0, 0, s, None) == 1 and "level" in err()
        assert lib.ndwt_estimate_sigma_items(plan._h, None, s, None) == 1 and "x_dev" in err()
        assert lib.ndwt_estimate_sigma_items(plan._h, x.ptr, None, None) == 1 and "sigma" in err()
    assert recs == [] and list(s) == [-1.0] * 5 and list(v) == [-1.0] * 20
    assert c.unchanged() and out.clean_outside() and not out.get().any()
