"""Order statistics of a band's |c| and the noise estimate on the device: ndwt_band_select, ndwt_estimate_sigma_coef, ndwt_estimate_sigma
and the classes' estimate_sigma / band_median / universal_thresholds.

A selection needs no transform: the coefficient array is ARBITRARY DATA written by the test (tests/select_cases.py: the contents and
the two checks), the plan only supplies the sizes and the data kind.  Every band lies between guard words in a buffer of NaN-free
filler, and the whole buffer is compared with its copy after the calls: the input is never modified.

  bands     37 elements (below one workgroup, not a multiple of 4: the element-wise form); 4096 elements aligned (the 4-scalar form); the
            same band as band 3 behind a band pitch of 4097 elements (off the 16- / 32-byte groups: element-wise); a batched plan of
            5 x 96; interleaved samples with inner = 3; 40 000 elements with set_tuning(target_blocks=3): 3 workgroups, more than ten
            turns of the grid-stride loop each
  ranks     0, N - 1 and the two middle ranks in one call; one rank twice in one call
  real      values[i] == np.partition(np.abs(band), k)[k] bit for bit, for Gaussian data, all elements equal, two values split at the
            median, values that differ only in the lowest / only in the highest digit of the key, and zeros of both signs, denormals,
            one inf and one NaN (the NaN is the last order statistic, the others are unchanged by its presence)
  complex   count(m < v (1 - eps)) <= k < count(m <= v (1 + eps)), m = hypot(re, im) in double, eps = 4 machine epsilons of the scalar
            type (the device contracts re re + im im into an FMA: at most three roundings, under 2 ulp, and the margin is twice that);
            Gaussian, all-equal, the two-value split, zeros
  sigma     1-D batch, 2-D, 3-D x float, double, complex64 x db4 (pres_l2_norm) and db1: estimate_sigma(x) and
            estimate_sigma_coef(dec(x, 3)) against the formula of include/ndwt.h evaluated in numpy on the ORACLE's level-1 last band,
            |sigma - ref| <= 2 TOL max|c| / (0.6745 g) (a median moves by no more than the coefficients do), and against each other
            under the same bound; universal_thresholds, and denoise with what it returns
  route     under kernel_trace() a select launches BandHist exactly select_passes times and BandPick as often, and nothing else; the
            number comes from csrc/ndwt_select.h (tests/select/bandselect_shim.cpp), the form and the grid from select_vec / select_grid
  refusals  null pointers, band, nk and k[i] out of range, with the argument named and nothing launched; a band of 2^32 elements
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
import ndwt_oracle as orc
from select_cases import COMPLEX_CONTENTS, KINDS, REAL_CONTENTS, build_shim, check_complex, check_real, complex_band, rank_sets, real_band

pytestmark = pytest.mark.gpu

TOL = {"double": 1e-12, "single": 2e-6}                       # tests/test_gpu_parity.py
GUARD = 8                                                     # scalars before the first band and after the last (32 / 64 bytes: the alignment stays)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory)


def stream():
    return torch.cuda.current_stream().cuda_stream


def torch_real(kind):
    return torch.float32 if KINDS[kind][0] == np.float32 else torch.float64


def make_plan(kind, shape):
    """(plan, elements of a band, levels): the plan kinds of the band list"""
    rdt, cplx = torch_real(kind), KINDS[kind][1]
    if shape == "n37":
        return ndwt.Plan([37], ["db1"], rdt, cplx, max_level=3), 37
    if shape in ("n4096", "n4096-pitched"):
        return ndwt.Plan([64, 64], ["db2", "db2"], rdt, cplx, max_level=1), 4096
    if shape == "batch-5x96":
        return ndwt.Plan([96], ["db2"], rdt, cplx, max_level=3, howmany=5), 480
    if shape == "inner-3":
        return ndwt.Plan([100], ["db2"], rdt, cplx, max_level=3, inner=3, howmany=2), 600
    if shape == "n40000-3-workgroups":
        p = ndwt.Plan([200, 200], ["db1", "db1"], rdt, cplx, max_level=1)
        p.set_tuning(target_blocks=3)
        return p, 40000
    raise ValueError(shape)


# (id, level, band, band pitch in elements or 0 = packed, every content or Gaussian only)
SHAPES = [
    ("n37", 3, 2, 0, True),
    ("n4096", 1, 3, 0, True),
    ("n4096-pitched", 1, 3, 4097, False),
    ("batch-5x96", 3, 1, 0, False),
    ("inner-3", 2, 2, 0, False),
    ("n40000-3-workgroups", 1, 1, 0, False),
]
CASES = [(f"{kind}-{sid}-{content}", kind, sid, level, band, pitch, content)
         for kind, (rdt, cplx) in KINDS.items() for sid, level, band, pitch, every in SHAPES
         for content in ((COMPLEX_CONTENTS if cplx else REAL_CONTENTS) if every else ("gauss",))]


class Coefs:
    """a coefficient array of `nb` bands at `pitch` elements (0: packed) between GUARD scalars, band `band` holding `data`, the rest
    filler; on the device, with its host copy"""

    def __init__(self, kind, N, nb, band, pitch, data, seed):
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        bs = (pitch or N) * comp
        host = np.random.default_rng(seed).standard_normal(GUARD + nb * bs + GUARD).astype(rdt) * rdt(100)
        host[GUARD + band * bs:GUARD + band * bs + N * comp] = data
        self.host = host
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = self.dev.data_ptr() + GUARD * host.itemsize
        self.band_addr = self.ptr + band * bs * host.itemsize

    def unchanged(self):
        return self.dev.cpu().numpy().tobytes() == self.host.tobytes()


def expected_route(shim, kind, addr, N, target_blocks=0):
    rdt, cplx = KINDS[kind]
    comp, sb = (2 if cplx else 1), np.dtype(rdt).itemsize
    vec = bool(shim.sel_select_vec(addr, N * comp, sb))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return shim.sel_select_passes(int(sb == 8)), vec, int(shim.sel_select_grid(N * comp, comp, int(vec), cus, target_blocks))


def check_route(recs, shim, kind, addr, N, calls, target_blocks=0):
    """`calls` selections: per call select_passes x (BandHist on select_grid workgroups, BandPick on one), alternating; nothing else"""
    rdt, cplx = KINDS[kind]
    passes, vec, grid = expected_route(shim, kind, addr, N, target_blocks)
    T = "float" if rdt == np.float32 else "double"
    assert len(recs) == 2 * passes * calls, recs
    for i, r in enumerate(recs):
        if i % 2 == 0:
            assert r.family == "BandHist" and r.params == {"T": T, "COMP": 2 if cplx else 1, "VEC": vec, "AGG": 2}, r
            assert r.grid == (grid, 1, 1) and r.block == (256, 1, 1), (r, grid)
        else:
            assert r.family == "BandPick" and r.params == {"T": T} and r.grid == (1, 1, 1) and r.block == (256, 1, 1), r
    return vec, grid


@pytest.mark.parametrize("cid,kind,sid,level,band,pitch,content", CASES, ids=[c[0] for c in CASES])
def test_select_is_exact_on_every_band_and_content(shim, cid, kind, sid, level, band, pitch, content):
    rdt, cplx = KINDS[kind]
    plan, N = make_plan(kind, sid)
    seed = zlib.crc32(cid.encode())
    data = complex_band(rdt, N, content, seed) if cplx else real_band(rdt, N, content, seed)
    nb = ndwt.num_bands(plan.ndim, level)
    c = Coefs(kind, N, nb, band, pitch, data, seed + 1)
    sets = rank_sets(N)
    with ndwt.kernel_trace() as recs:
        got = [plan.band_select(c.ptr, level, band, ks, stream(), band_pitch=pitch) for ks in sets]
    for ks, g in zip(sets, got):
        (check_complex if cplx else check_real)(data, ks, g, cid)
    vec, grid = check_route(recs, shim, kind, c.band_addr, N, len(sets), 3 if sid.startswith("n40000") else 0)
    # the shapes take the forms they are there for
    assert vec == (sid in ("n4096", "batch-5x96", "inner-3", "n40000-3-workgroups")), (sid, vec)
    if sid.startswith("n40000"):
        assert grid == 3 and N * (2 if cplx else 1) // 4 > 10 * 3 * 256
    assert c.unchanged()                                          # the band, its neighbours and the guard words


def test_the_special_values_order_as_numpy_orders_them():
    """zeros of both signs are one key, the denormals follow, the inf is the last number and the NaN the last order statistic"""
    for kind in ("f32", "f64"):
        rdt = KINDS[kind][0]
        plan = ndwt.Plan([64], ["db1"], torch_real(kind), False, max_level=1)
        data = real_band(rdt, 64, "special", 7)
        c = Coefs(kind, 64, 2, 1, 0, data, 3)
        for ks in ([0, 1, 2, 3], [4, 5, 6, 7], [60, 61, 62, 63]):
            check_real(data, ks, plan.band_select(c.ptr, 1, 1, ks, stream()), kind)
        tail = plan.band_select(c.ptr, 1, 1, [62, 63], stream())
        assert np.isinf(tail[0]) and np.isnan(tail[1])
        head = plan.band_select(c.ptr, 1, 1, [0, 3, 4], stream())
        assert head[0] == 0 and head[1] == 0 and not np.signbit(head[:2]).any() and 0 < head[2] < np.finfo(rdt).tiny
        assert c.unchanged()


def test_the_combining_of_equal_digits_changes_no_value(shim):
    """variant 9 (select_agg: no wave-wide combining) launches BandHist<.., AGG = 0> and returns the same bits"""
    for kind in ("f32", "c128"):
        rdt, cplx = KINDS[kind]
        plan, N = make_plan(kind, "n4096")
        data = complex_band(rdt, N, "gauss", 11) if cplx else real_band(rdt, N, "gauss", 11)
        c = Coefs(kind, N, 4, 2, 0, data, 12)
        ks = rank_sets(N)[0]
        a = plan.band_select(c.ptr, 1, 2, ks, stream())
        plan.set_variant(fwd=9)
        with ndwt.kernel_trace() as recs:
            b = plan.band_select(c.ptr, 1, 2, ks, stream())
        assert shim.sel_select_agg(9) == 0 and all(r.params["AGG"] == 0 for r in recs if r.family == "BandHist")
        assert a.tobytes() == b.tobytes()


def _raw(plan, y, level, band, nk, k, values, pitch=0):
    lib = ndwt.lib()
    rc = lib.ndwt_band_select(plan._h, y, pitch, level, band, nk, k, values, None)
    return rc, lib.ndwt_last_error().decode()


def test_every_refusal_names_its_argument_and_launches_nothing():
    plan = ndwt.Plan([64, 64], ["db2", "db2"], torch.float32, False, max_level=2)
    c = Coefs("f32", 4096, 7, 1, 0, real_band(np.float32, 4096, "gauss", 1), 2)
    k = (ctypes.c_int64 * 5)(0, 1, 2, 3, 4)
    v = (ctypes.c_double * 5)(*[-1.0] * 5)
    s = ctypes.c_double(-1.0)
    lib = ndwt.lib()
    with ndwt.kernel_trace() as recs:
        assert _raw(plan, c.ptr, 2, 1, 4, k, v)[0] == 0
    assert len(recs) == 6
    with ndwt.kernel_trace() as recs:
        for args, word in (((None, 2, 1, 1, k, v), "y_dev"), ((c.ptr, 2, 1, 1, None, v), "(k)"), ((c.ptr, 2, 1, 1, k, None), "values"),
                           ((c.ptr, 2, -1, 1, k, v), "band -1"), ((c.ptr, 2, 7, 1, k, v), "band 7"), ((c.ptr, 1, 4, 1, k, v), "band 4"),
                           ((c.ptr, 2, 1, 0, k, v), "nk = 0"), ((c.ptr, 2, 1, 5, k, v), "nk = 5"), ((c.ptr, 3, 1, 1, k, v), "level 3")):
            rc, msg = _raw(plan, *args)
            assert rc == 1 and word in msg, (args[1:4], rc, msg)
        for bad in (-1, 4096, 1 << 40):
            kk = (ctypes.c_int64 * 2)(0, bad)
            rc, msg = _raw(plan, c.ptr, 2, 1, 2, kk, v)
            assert rc == 1 and "k[1]" in msg and str(bad) in msg, msg
        assert _raw(plan, c.ptr, 2, 1, 1, k, v, pitch=4095) [0] == 1 and "pitch" in lib.ndwt_last_error().decode()
        assert lib.ndwt_estimate_sigma_coef(plan._h, None, 0, 2, ctypes.byref(s), None) == 1 and "y_dev" in lib.ndwt_last_error().decode()
        assert lib.ndwt_estimate_sigma_coef(plan._h, c.ptr, 0, 2, None, None) == 1 and "sigma" in lib.ndwt_last_error().decode()
        assert lib.ndwt_estimate_sigma_coef(plan._h, c.ptr, 0, 0, ctypes.byref(s), None) == 1 and "level" in lib.ndwt_last_error().decode()
        assert lib.ndwt_estimate_sigma(plan._h, None, ctypes.byref(s), None) == 1 and "x_dev" in lib.ndwt_last_error().decode()
        assert lib.ndwt_estimate_sigma(plan._h, c.ptr, None, None) == 1 and "sigma" in lib.ndwt_last_error().decode()
    assert recs == [] and s.value == -1.0
    assert c.unchanged()


def test_a_band_of_two_to_the_32_elements_is_refused_before_any_launch():
    """the plan's creation allocates its two approximation buffers (16 GiB each); the call itself reads nothing of y"""
    try:
        plan = ndwt.Plan([1 << 16, 1 << 16], ["db1", "db1"], torch.float32, False, max_level=1)
    except ndwt.NdwtError as e:
        if e.code == 6:                                           # NDWT_ERR_ALLOC: the device is too full for the plan itself
            pytest.skip(f"no room for a plan over 2^32 elements: {e.message}")
        raise
    y = torch.zeros(64, dtype=torch.float32, device="cuda")
    with ndwt.kernel_trace() as recs:
        with pytest.raises(ndwt.NdwtError, match="32 bits") as ei:
            plan.band_select(y.data_ptr(), 1, 0, [0], stream())
    assert ei.value.code == 7 and recs == []                      # NDWT_ERR_UNSUPPORTED
    del plan
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ sigma
SIGMA_OBJECTS = {
    "1d-batch-8x256": (lambda wn, l2, prec: ndwt.nd_dwt_1D(wn, 256, "batch", 8, "pres_l2_norm", l2, "precision", prec), [256], 8),
    "2d-64x64": (lambda wn, l2, prec: ndwt.nd_dwt_2D(wn, [64, 64], "pres_l2_norm", l2, "precision", prec), [64, 64], None),
    "3d-16x16x16": (lambda wn, l2, prec: ndwt.nd_dwt_3D(wn, [16, 16, 16], "pres_l2_norm", l2, "precision", prec), [16, 16, 16], None),
}
SIGMA_CASES = [(f"{obj}-{kind}-{wn}", obj, kind, wn, l2) for obj in SIGMA_OBJECTS for kind in ("f32", "f64", "c64") for wn, l2 in (("db4", 1), ("db1", 0))]
_SIGMA = {}


def sigma_case(cid, obj, kind, wn, l2):
    """(x in MATLAB shape at the kind's precision, the oracle's level-1 last band over all items, its gain), made once"""
    if cid not in _SIGMA:
        rdt, cplx = KINDS[kind]
        _, sizes, K = SIGMA_OBJECTS[obj]
        rng = np.random.default_rng(zlib.crc32(cid.encode()))
        shape = sizes + ([K] if K else [])
        grid = np.meshgrid(*[np.linspace(0, 1, n, endpoint=False) for n in sizes], indexing="ij")
        smooth = sum(np.sin(2 * np.pi * (a + 1) * g) for a, g in enumerate(grid))
        smooth = smooth[..., None] * np.linspace(1, 2, K) if K else smooth
        x = smooth + 0.3 * rng.standard_normal(shape)
        if cplx:
            x = x + 1j * (0.5 * smooth + 0.3 * rng.standard_normal(shape))
        x = x.astype((np.complex64 if rdt == np.float32 else np.complex128) if cplx else rdt)
        xd = x.astype(np.complex128 if cplx else np.float64)

        def last_band(v):
            d = lambda u: orc.spatial_dec(u, [wn] * len(sizes), 1, l2)[..., -1]
            return d(v.real) + 1j * d(v.imag) if cplx else d(v)
        c = np.stack([last_band(xd[..., j]) for j in range(K)], axis=-1) if K else last_band(xd)
        g = float(ndwt.band_gains(sizes, wn, 1, pres_l2_norm=l2)[-1])
        _SIGMA[cid] = (x, c, g)
    return _SIGMA[cid]


@pytest.mark.parametrize("cid,obj,kind,wn,l2", SIGMA_CASES, ids=[c[0] for c in SIGMA_CASES])
def test_sigma_is_the_formula_on_the_oracles_last_band(cid, obj, kind, wn, l2):
    rdt, cplx = KINDS[kind]
    prec = "single" if rdt == np.float32 else "double"
    x, c, g = sigma_case(cid, obj, kind, wn, l2)
    w = SIGMA_OBJECTS[obj][0](wn, l2, prec)
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda().permute(*reversed(range(x.ndim)))
    m = float(np.median(np.abs(c)))
    ref = m / (1.1774100225154747 if cplx else 0.6744897501960817) / g
    bound = 2 * TOL[prec] * float(np.abs(c).max()) / (0.6745 * g)
    s_x = w.estimate_sigma(xt)
    s_c = w.estimate_sigma_coef(w.dec(xt, 3))
    print(f"{cid}: sigma from x {s_x:.9g}, from dec(x, 3) {s_c:.9g}, reference {ref:.9g}; bound {bound:.3g}, gain {g:.6g}")
    assert abs(s_x - ref) <= bound and abs(s_c - ref) <= bound
    assert abs(s_x - s_c) <= bound
    assert 0.2 < ref < 0.45                                       # the noise that was put in (0.3; the smooth part leaks a little)
    # band_median on the coefficient array: the same median, before the division
    y = w.dec(xt, 2)
    nb = y.shape[-1]
    assert abs(w.band_median(y, nb - 1) - m) <= 2 * TOL[prec] * float(np.abs(c).max())
    # universal thresholds: sqrt(2 ln N) sigma gains, entry 0 zero -- and the existing denoise takes them as they are
    sizes = SIGMA_OBJECTS[obj][1]
    thr = w.universal_thresholds(xt, 2)
    want = np.sqrt(2 * np.log(float(np.prod(sizes)))) * s_x * w.band_gains(2)
    want[0] = 0.0
    assert thr.shape == (nb,) and thr[0] == 0.0 and np.allclose(thr, want, rtol=1e-12, atol=0)
    assert np.allclose(w.universal_thresholds(xt, 2, k=3.0)[1:], 3.0 * s_x * w.band_gains(2)[1:], rtol=1e-12, atol=0)
    out = w.denoise(xt, 2, thr)
    assert out.shape == xt.shape and bool(torch.isfinite(torch.view_as_real(out) if cplx else out).all())
    assert float((out - xt).abs().max()) > 0                      # the thresholds did something
