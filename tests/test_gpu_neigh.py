"""Neighbourhood shrinkage on the device: ndwt_shrink_neigh, ndwt_denoise_neigh and the classes' shrink_neigh / denoise_neigh /
neigh_thresholds.

The shrink needs no transform: the coefficient array is ARBITRARY DATA written by the test (tests/neigh_cases.py: random items, an
integer-valued band, an item with a NaN, an all-zero item, -0), the plan only supplies the shapes and the data kind.  Both arrays lie
between guard scalars, the bands on a pitch have guard scalars between them, and the WHOLE output buffer is compared afterwards: float and
complex64 bit for bit with numpy, double and complex128 bit for bit with the exact-fma reference and, on the integer-valued band, with
plain numpy too (neigh_cases.check_neigh).

Shapes (neigh_cases.shape_list), TX, TY and the chunk taken from the instance under test (tests/select/neigh_shim.cpp):
  window        every filtered axis exactly 2r + 1 long, every neighbour wraps: all 36 instances
  tile+1  axes of TX + 1 (TY + 1), odd; the marched axis 3 (2r + 1) + 2 long with set_tuning forcing the smallest chunk: every seam
                and the wrap of the ring's priming
  2tile-1       axes of 2 TX - 1 (2 TY - 1)
  items         K = 3 on a batched 1-D plan, a 2-D stack and a 3-D stack, at a pitch larger than a band, one band with threshold 0 (copied
                with its NaN and -0)
the last three for every kind and number of axes, the radius rotating.  On their own: constant items (a window that leaks into the
neighbouring item fails there), a NaN (exactly the M positions whose window holds it become +0), the shifted form, denoise_neigh against
dec -> shrink_neigh (shifted) -> rec, the trace, the classes and the refusals.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
from neigh_cases import (BIG, GUARD_VALUE, INT_BAND, NAN_BAND, OUT_FILL, ZERO_BAND, band_view, check_neigh, geometry, levels_for, median_thresholds,
                         neigh_array, neigh_shim, reference_neigh, shape_list)
from select_cases import KINDS

pytestmark = pytest.mark.gpu

GUARD = 8                                                     # scalars before and after each array


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return neigh_shim(tmp_path_factory)


def stream():
    return torch.cuda.current_stream().cuda_stream


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def torch_real(kind):
    return torch.float32 if KINDS[kind][0] == np.float32 else torch.float64


def tname(kind):
    return "float" if KINDS[kind][0] == np.float32 else "double"


def elem_bytes(kind):
    return np.dtype(KINDS[kind][0]).itemsize * (2 if KINDS[kind][1] else 1)


def make_plan(kind, dims, items, level, wname="db1"):
    """an unbatched plan, a batched 1-D plan or a stack of `items` images / volumes"""
    rdt, cplx = torch_real(kind), KINDS[kind][1]
    nd = len(dims)
    if items == 1:
        return ndwt.Plan(dims, [wname] * nd, rdt, cplx, max_level=level)
    if nd == 1:
        return ndwt.Plan(dims, [wname], rdt, cplx, max_level=level, howmany=items)
    return ndwt.Plan(list(dims) + [items], [wname] * nd + [None], rdt, cplx, max_level=level, axes=tuple(range(nd)))


class Arrays:
    """the coefficient array of tests/neigh_cases.py and an output buffer of the same layout, each between GUARD scalars; band b of either
    lies at off + b * bs scalars"""

    def __init__(self, kind, items, dims, nb, pitch_elements, seed):
        rdt, cplx = KINDS[kind]
        self.kind, self.items, self.dims, self.nb = kind, items, list(dims), nb
        self.comp = 2 if cplx else 1
        n = items * int(np.prod(dims)) * self.comp
        self.bs = (pitch_elements * self.comp) if pitch_elements else n
        self.flat, lead, pitch = neigh_array(kind, items, dims, nb, self.bs - n, seed)
        assert pitch == self.bs
        self.flat = self.flat[lead:]                              # (the guards around the array are this class's)
        self.off = GUARD
        self.host = np.full(GUARD + nb * self.bs + GUARD, GUARD_VALUE, dtype=rdt)
        self.host[GUARD:GUARD + nb * self.bs] = self.flat
        self.host.setflags(write=False)
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.ptr = self.dev.data_ptr() + GUARD * self.host.itemsize
        self.fresh_out()

    def fresh_out(self):
        self.out = torch.full((self.host.size,), OUT_FILL, dtype=self.dev.dtype, device="cuda")
        self.optr = self.out.data_ptr() + GUARD * self.host.itemsize
        return self

    def result(self):
        """(the bands of the output as they are on the device, whether the guards around them are untouched)"""
        h = self.out.cpu().numpy()
        inner = slice(GUARD, GUARD + self.nb * self.bs)
        fill = KINDS[self.kind][0](OUT_FILL)
        return h[inner].copy(), bool((h[:GUARD] == fill).all() and (h[inner.stop:] == fill).all())

    def unchanged(self):
        return self.dev.cpu().numpy().tobytes() == self.host.tobytes()


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def all_cases():
    """[(id, kind, nd, r, shape id)] -- the list of tests/test_emulated_neigh.py: `window` for every instance, the other shapes for every
    kind and number of axes with the radius rotating"""
    out = []
    for ki, kind in enumerate(KINDS):
        for nd in (1, 2, 3):
            for r in (1, 2, 3):
                for sid in ("window", "tile+1", "2tile-1", "items"):
                    if sid == "window" or r == 1 + (ki + nd) % 3:
                        out.append((f"{kind}-{nd}d-r{r}-{sid}", kind, nd, r, sid))
    return out


CASES = all_cases()


def the_shape(shim, kind, nd, r, sid):
    sh = {s: (d, k) for s, d, k in shape_list(nd, r, shim.sel_neigh_tx(nd), shim.sel_neigh_ty(nd, elem_bytes(kind), r))}
    return sh[sid]


@pytest.mark.parametrize("cid,kind,nd,r,sid", CASES, ids=[c[0] for c in CASES])
def test_the_whole_output_buffer(shim, cid, kind, nd, r, sid):
    dims, items = the_shape(shim, kind, nd, r, sid)
    level = levels_for(nd)
    nb = ndwt.num_bands(nd, level)
    plan = make_plan(kind, dims, items, level)
    N = int(np.prod(dims))
    pitch = items * N + 5 if sid == "items" else 0                # a pitch larger than a band: guard scalars between the bands
    a = Arrays(kind, items, dims, nb, pitch, zlib.crc32(cid.encode()) % 100000)
    thr = median_thresholds(kind, a.flat, 0, a.bs, items, dims, nb, r, zero_bands=(ZERO_BAND,) if items > 1 else (), below=sid == "window")
    target = BIG if sid == "tile+1" else 0
    plan.set_tuning(target, 0)
    ntx, nty, chunk, nchunks = geometry(shim, nd, dims, elem_bytes(kind), r, nb * items, cus(), target)
    if sid == "tile+1":
        assert (ntx, nty) == (2, 2 if nd == 3 else 1)
        assert nd == 1 or (nchunks == 3 and 2 * r + 1 <= chunk <= 2 * r + 2)
    if sid == "2tile-1":
        assert (ntx, nty) == (2, 2 if nd == 3 else 1)
    for hard in (False, True):
        a.fresh_out()
        with ndwt.kernel_trace() as recs:
            plan.shrink_neigh(a.ptr, a.optr, level, thr, r, hard, stream(), band_pitch=pitch)
        assert len(recs) == 1 and recs[0].family == "NeighShrink", recs
        assert recs[0].params == {"T": tname(kind), "COMP": a.comp, "ND": nd, "R": r}, recs[0]
        assert recs[0].grid == (nb * items * nchunks * nty * ntx, 1, 1) and recs[0].block == (256, 1, 1), (recs[0], ntx, nty, chunk, nchunks)
        got, outside = a.result()
        assert outside and a.unchanged()                          # the guards around the output; y is read only, bit for bit
        check_neigh(kind, a.flat, got, 0, a.bs, items, dims, nb, thr, r, hard, what=f"{cid} hard={hard}")
        if items > 1:                                             # (in check_neigh's comparison too; said once more: threshold 0 is a copy)
            assert same(band_view(kind, got, 0, a.bs, items, dims, ZERO_BAND), band_view(kind, a.flat, 0, a.bs, items, dims, ZERO_BAND))
        assert hard or not same(got, a.flat)                      # (and something was shrunk)


CONSTANT = [("f32", 1, 3), ("c64", 2, 1), ("f64", 3, 2), ("c128", 1, 2), ("f32", 2, 2), ("c128", 3, 1)]


@pytest.mark.parametrize("kind,nd,r", CONSTANT, ids=[f"{k}-{nd}d-r{r}" for k, nd, r in CONSTANT])
def test_a_window_never_leaks_into_the_neighbouring_item(kind, nd, r):
    """3 constant items a_j = j + 1, hard, t^2 = 6 M between M a_1^2 and M a_2^2: items 0 and 1 become zero and item 2 is untouched, up to
    and including the items' first and last positions"""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    w = 2 * r + 1
    dims = [w + 2, w + 1, w][:nd]
    level = levels_for(nd)
    nb = ndwt.num_bands(nd, level)
    plan = make_plan(kind, dims, 3, level)
    n = int(np.prod(dims)) * comp
    src = np.zeros((nb, 3, n), dtype=rdt)
    for j in range(3):
        src[:, j, ::comp] = j + 1
    y = torch.from_numpy(src).cuda()
    out = torch.full_like(y, OUT_FILL)
    thr = np.full(nb, float(np.sqrt(6.0 * w ** nd)))
    plan.shrink_neigh(y.data_ptr(), out.data_ptr(), level, thr, r, True, stream())
    got = out.cpu().numpy()
    assert not got[:, :2].any() and not np.signbit(got[:, :2]).any() and same(got[:, 2], src[:, 2]) and same(y.cpu().numpy(), src)
    assert same(got.reshape(-1), reference_neigh(kind, src.reshape(-1), 0, 3 * n, 3, dims, nb, thr, r, True, fused=True))


NAN_CASES = [("f32", 1, 1), ("c64", 2, 2), ("f64", 3, 1), ("c128", 2, 3), ("f32", 3, 3)]


@pytest.mark.parametrize("kind,nd,r", NAN_CASES, ids=[f"{k}-{nd}d-r{r}" for k, nd, r in NAN_CASES])
def test_exactly_the_windows_that_hold_the_nan_become_zero(kind, nd, r):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    w = 2 * r + 1
    dims = [w + 3, w + 1, w + 2][:nd]
    level = levels_for(nd)
    nb = ndwt.num_bands(nd, level)
    plan = make_plan(kind, dims, 1, level)
    rng = np.random.default_rng(5)
    shape = tuple(reversed(dims)) + (comp,)
    src = (rng.standard_normal((nb,) + shape) + 3.0).astype(rdt)
    at = tuple(d // 3 for d in shape[:-1])
    src[(1,) + at + (comp - 1,)] = np.nan                         # band 1, one part of one element
    y = torch.from_numpy(src).cuda()
    out = torch.full_like(y, OUT_FILL)
    thr = np.full(nb, 1e-3)
    plan.shrink_neigh(y.data_ptr(), out.data_ptr(), level, thr, r, True, stream())
    got = out.cpu().numpy()
    hit = np.zeros(shape[:-1], dtype=bool)
    for off in np.ndindex(*([w] * nd)):
        hit[tuple((a + o - r) % d for a, o, d in zip(at, off, shape[:-1]))] = True
    assert int(hit.sum()) == w ** nd
    want = src.copy()
    want[1][hit] = 0
    assert same(got, want) and not np.signbit(got[1][hit]).any()


SHIFT_CASES = [("f32", 1, 2, 3), ("c64", 2, 1, 1), ("f64", 3, 1, 1), ("c128", 2, 3, 3), ("f32", 3, 2, 2)]


@pytest.mark.parametrize("kind,nd,r,items", SHIFT_CASES, ids=[f"{k}-{nd}d-r{r}-{i}items" for k, nd, r, i in SHIFT_CASES])
def test_the_output_one_band_slot_down_gives_the_bits_of_the_separate_output(kind, nd, r, items):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    w = 2 * r + 1
    dims = [w + 4, w + 2, 2 * w + 1][:nd]
    level = levels_for(nd)
    nb = ndwt.num_bands(nd, level)
    plan = make_plan(kind, dims, items, level)
    n = items * int(np.prod(dims)) * comp
    bs = n + 6 * comp                                             # 6 elements between the bands
    rng = np.random.default_rng(11)
    host = np.full((nb + 1) * bs, GUARD_VALUE, dtype=rdt)
    for b in range(nb):
        host[(b + 1) * bs:(b + 1) * bs + n] = rng.standard_normal(n).astype(rdt)
    thr = np.full(nb, 1.2 * np.sqrt(float(w ** nd) * comp))
    thr[[0, nb - 1]] = 0.0                                        # the first and the last band: copies
    isz = host.itemsize
    for hard in (False, True):
        buf = torch.from_numpy(host).cuda()
        sep = torch.full_like(buf, OUT_FILL)
        with ndwt.kernel_trace() as recs:
            plan.shrink_neigh(buf.data_ptr() + bs * isz, sep.data_ptr() + bs * isz, level, thr, r, hard, stream(), band_pitch=bs // comp)
        assert [x.family for x in recs] == ["NeighShrink"]
        with ndwt.kernel_trace() as recs:
            plan.shrink_neigh(buf.data_ptr() + bs * isz, buf.data_ptr(), level, thr, r, hard, stream(), band_pitch=bs // comp)
        assert [x.family for x in recs] == ["NeighShrink"] * (nb - 2), recs   # one per non-zero band, none for the copies
        assert all(x.grid == (recs[0].grid[0], 1, 1) for x in recs)
        got, want = buf.cpu().numpy(), sep.cpu().numpy()
        for b in range(nb):
            assert same(got[b * bs:b * bs + n], want[(b + 1) * bs:(b + 1) * bs + n]), b
            assert same(got[b * bs + n:(b + 1) * bs], host[b * bs + n:(b + 1) * bs]), b      # the scalars between the bands
        assert same(got[nb * bs:], host[nb * bs:])                # the last input band is still there
        assert same(got[:n], host[bs:bs + n]) and not same(got[bs:bs + n], host[2 * bs:2 * bs + n])
    # an all-zero table: copies only, in either form
    buf = torch.from_numpy(host).cuda()
    sep = torch.full_like(buf, OUT_FILL)
    with ndwt.kernel_trace() as recs:
        plan.shrink_neigh(buf.data_ptr() + bs * isz, sep.data_ptr() + bs * isz, level, np.zeros(nb), r, False, stream(), band_pitch=bs // comp)
        plan.shrink_neigh(buf.data_ptr() + bs * isz, buf.data_ptr(), level, np.zeros(nb), r, False, stream(), band_pitch=bs // comp)
    assert recs == []
    got, want = buf.cpu().numpy(), sep.cpu().numpy()
    for b in range(nb):
        assert same(got[b * bs:b * bs + n], host[(b + 1) * bs:(b + 1) * bs + n]) and same(want[(b + 1) * bs:(b + 1) * bs + n], host[(b + 1) * bs:(b + 1) * bs + n])
        assert (want[(b + 1) * bs + n:(b + 2) * bs] == rdt(OUT_FILL)).all()
    # any other overlap is refused
    lib = ndwt.lib()
    t = (ctypes.c_double * nb)(*([1.0] * nb))
    for delta in (0, isz * comp, -isz * comp, bs * isz, -2 * bs * isz + isz * comp):
        rc = lib.ndwt_shrink_neigh(plan._h, buf.data_ptr() + 2 * bs * isz, buf.data_ptr() + 2 * bs * isz + delta, bs // comp, level, r, t, 0, None)
        assert rc == 1 and "out_dev overlaps y_dev" in lib.ndwt_last_error().decode(), delta


DENOISE_CASES = [("f32", [40], 3, 2, 2), ("c64", [12, 10], 3, 1, 1), ("f64", [9, 8, 7], 1, 1, 1), ("c128", [16, 9], 1, 2, 3), ("f32", [8, 8, 8], 2, 1, 2)]


@pytest.mark.parametrize("kind,dims,items,level,r", DENOISE_CASES, ids=[f"{k}-{'x'.join(map(str, d))}-{i}items-r{r}" for k, d, i, _, r in DENOISE_CASES])
def test_denoise_neigh_is_dec_shrink_neigh_rec(kind, dims, items, level, r):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    nd = len(dims)
    plan = make_plan(kind, dims, items, level, "db2")
    nb = ndwt.num_bands(nd, level)
    rng = np.random.default_rng(zlib.crc32(f"den-{kind}-{dims}".encode()))
    xh = rng.standard_normal(items * int(np.prod(dims)) * comp).astype(rdt)
    x = torch.from_numpy(xh).cuda()
    pitch = plan.band_pitch()
    y = torch.zeros((nb + 1) * pitch * comp, dtype=x.dtype, device="cuda")
    slot1 = y.data_ptr() + pitch * comp * xh.itemsize
    thr = np.full(nb, 0.9 * np.sqrt(float((2 * r + 1) ** nd) * comp))
    thr[0] = 0.0
    for hard in (False, True):
        out, ref = torch.full_like(x, 7.0), torch.full_like(x, -7.0)
        with ndwt.kernel_trace() as recs:
            plan.denoise_neigh(x.data_ptr(), out.data_ptr(), level, thr, r, hard, stream())
        fams = [q.family for q in recs]
        assert fams.count("NeighShrink") == nb - 1, fams
        assert not {"shrink_kernel", "ShrinkItems", "JointShrink", "JointTile", "Den1C"} & set(fams), fams
        plan.dec(x.data_ptr(), slot1, level, stream(), band_pitch=pitch)
        plan.shrink_neigh(slot1, y.data_ptr(), level, thr, r, hard, stream(), band_pitch=pitch)
        plan.rec(y.data_ptr(), ref.data_ptr(), level, stream(), band_pitch=pitch)
        assert torch.equal(out, ref) and bool(torch.isfinite(out).all()) and not torch.equal(out, x)
        assert same(x.cpu().numpy(), xh)
    # the other calls on the plan's scratch still work after it grew by a slot
    out2, ref2 = torch.full_like(x, 7.0), torch.full_like(x, -7.0)
    plan.denoise_bands(x.data_ptr(), out2.data_ptr(), level, thr, False, stream())
    plan.dec(x.data_ptr(), y.data_ptr(), level, stream(), band_pitch=pitch)
    plan.shrink_bands(y.data_ptr(), level, thr, False, stream(), band_pitch=pitch)
    plan.rec(y.data_ptr(), ref2.data_ptr(), level, stream(), band_pitch=pitch)
    assert torch.equal(out2, ref2)


def test_the_default_chunk_rule_on_a_volume_and_the_same_bits_with_another_grid(shim):
    """a float volume of 70 x 20 x 40, r = 1: the default rule splits the march (few tiles on many compute units); the smallest chunks and
    one chunk give the same bits"""
    kind, dims, r, level = "f32", [70, 20, 40], 1, 1
    nb = ndwt.num_bands(3, level)
    plan = make_plan(kind, dims, 1, level)
    a = Arrays(kind, 1, dims, nb, 0, 77)
    thr = median_thresholds(kind, a.flat, 0, a.bs, 1, dims, nb, r)
    res = []
    for target in (0, BIG, 1):
        plan.set_tuning(target, 0)
        ntx, nty, chunk, nchunks = geometry(shim, 3, dims, 4, r, nb, cus(), target)
        a.fresh_out()
        with ndwt.kernel_trace() as recs:
            plan.shrink_neigh(a.ptr, a.optr, level, thr, r, False, stream())
        assert len(recs) == 1 and recs[0].grid == (nb * nchunks * nty * ntx, 1, 1), (recs, ntx, nty, chunk, nchunks)
        res.append(a.result()[0])
        assert nchunks == (1 if target == 1 else 10) and chunk == (40 if target == 1 else 4)
    check_neigh(kind, a.flat, res[0], 0, a.bs, 1, dims, nb, thr, r, False, what="default chunks")
    assert same(res[0], res[1]) and same(res[0], res[2])


def test_the_classes_run_against_the_same_reference():
    for prec, cplx, kind in (("single", False, "f32"), ("double", True, "c128")):
        rdt = KINDS[kind][0]
        comp = 2 if cplx else 1
        # a batch of signals: MATLAB shape [n, K]
        K, n, level, r = 3, 24, 2, 2
        w = ndwt.nd_dwt_1D("db2", n, "batch", K, "precision", prec)
        nb = ndwt.num_bands(1, level)
        rng = np.random.default_rng(71)
        x = rng.standard_normal((n, K)) + (1j * rng.standard_normal((n, K)) if cplx else 0)
        xt = torch.from_numpy(x.astype(np.complex128 if cplx else np.float32)).cuda()
        y = w.dec(xt, level)                                        # [n, K, bands]
        yk = y.permute(2, 1, 0).contiguous()                        # kernel order: [bands, K, n]
        flat = (torch.view_as_real(yk) if cplx else yk).cpu().numpy().reshape(-1)
        pitch = K * n * comp
        thr = np.array([0.0, 2.5, 3.5])
        plan = w._plan(cplx, level, xt.device)
        xk = xt.permute(1, 0).contiguous()
        for mode in ("soft", "hard"):
            for t, tv in ((thr, thr), (torch.from_numpy(thr), thr), (3.0, np.array([0.0, 3.0, 3.0]))):
                got = w.shrink_neigh(y, t, r, mode)
                assert got.shape == y.shape and got.dtype == y.dtype
                gk = got.permute(2, 1, 0).contiguous()
                gflat = (torch.view_as_real(gk) if cplx else gk).cpu().numpy().reshape(-1)
                want = reference_neigh(kind, flat, 0, pitch, K, [n], nb, tv, r, mode == "hard", fused=True)
                assert same(gflat, want) and not same(gflat, flat)
                ok = torch.empty_like(xk)
                plan.denoise_neigh(xk.data_ptr(), ok.data_ptr(), level, tv, r, mode == "hard", stream())
                assert torch.equal(w.denoise_neigh(xt, level, t, r, mode).permute(1, 0).contiguous(), ok)
        assert same(yk.cpu().numpy(), y.permute(2, 1, 0).contiguous().cpu().numpy())     # shrink_neigh returns a new array
        # the rules: host arithmetic over estimate_sigma and band_gains
        s, g = w.estimate_sigma(xt), w.band_gains(level)
        M, N = (2 * r + 1) ** 1, float(n)
        for rule, k in (("universal", np.sqrt(2 * np.log(N))), ("wiener", np.sqrt(M)), ("block", np.sqrt(4.50524 * M))):
            row = w.neigh_thresholds(xt, level, r, rule)
            assert row.shape == (nb,) and row[0] == 0 and np.allclose(row[1:], k * s * g[1:], rtol=1e-14)
            assert w.shrink_neigh(y, row, r).shape == y.shape
    # an image: MATLAB shape [n0, n1]
    w2 = ndwt.nd_dwt_2D("db1", [10, 7], "precision", "single")
    x2 = torch.from_numpy(np.random.default_rng(3).standard_normal((10, 7)).astype(np.float32)).cuda()
    y2 = w2.dec(x2, 1)                                              # [10, 7, 4]
    got = w2.shrink_neigh(y2, 1.5, 1)
    flat = y2.permute(2, 1, 0).contiguous().cpu().numpy().reshape(-1)
    want = reference_neigh("f32", flat, 0, 70, 1, [10, 7], 4, [0.0, 1.5, 1.5, 1.5], 1, False)
    assert same(got.permute(2, 1, 0).contiguous().cpu().numpy().reshape(-1), want)
    with pytest.raises(ValueError, match="mode must be"):
        w2.shrink_neigh(y2, 1.0, 1, "firm")
    with pytest.raises(ValueError, match="rule must be"):
        w2.neigh_thresholds(x2, 1, 1, "sure")


def test_every_refusal_names_its_argument_and_launches_nothing():
    plan = ndwt.Plan([24], ["db2"], torch.float32, False, max_level=3, howmany=5)
    items, N, level, nb = 5, 24, 2, 3
    a = Arrays("f32", items, [N], nb, 0, 5)
    lib = ndwt.lib()
    err = lambda: lib.ndwt_last_error().decode()
    dbl = lambda *v: (ctypes.c_double * len(v))(*v)
    good = dbl(0.0, 1.0, 1.0)
    x = torch.full((items * N,), 2.0, device="cuda")
    o = torch.full((items * N,), -2.0, device="cuda")
    INVALID, UNSUPPORTED = 1, 7
    with ndwt.kernel_trace() as recs:
        for args, word in (((None, a.optr, 0, level, 1, good, 0), "y_dev"), ((a.ptr, None, 0, level, 1, good, 0), "out_dev"),
                           ((a.ptr, a.optr, 0, level, 1, None, 0), "null thresholds"), ((a.ptr, a.optr, 0, level, 0, good, 0), "radius 0"),
                           ((a.ptr, a.optr, 0, level, 4, good, 0), "radius 4"), ((a.ptr, a.optr, 0, level, 1, dbl(0.0, -1.0, 1.0), 0), "threshold of band 1"),
                           ((a.ptr, a.optr, 0, level, 1, dbl(0.0, 1.0, float("nan")), 1), "threshold of band 2"), ((a.ptr, a.optr, 0, level, 1, good, 2), "mode"),
                           ((a.ptr, a.optr, 0, 0, 1, good, 0), "level 0"), ((a.ptr, a.optr, 0, 4, 1, good, 0), "level 4"),
                           ((a.ptr, a.optr, items * N - 1, level, 1, good, 0), "pitch"), ((a.ptr, a.ptr, 0, level, 1, good, 0), "out_dev overlaps y_dev")):
            assert lib.ndwt_shrink_neigh(plan._h, *args, None) == INVALID and word in err(), (word, err())
        for args, word in (((None, o.data_ptr(), level, 1, good, 0), "x_dev"), ((x.data_ptr(), None, level, 1, good, 0), "out_dev"),
                           ((x.data_ptr(), o.data_ptr(), level, 1, None, 0), "null thresholds"), ((x.data_ptr(), o.data_ptr(), level, 5, good, 0), "radius 5"),
                           ((x.data_ptr(), o.data_ptr(), level, 1, dbl(-0.5, 1.0, 1.0), 0), "threshold of band 0"),
                           ((x.data_ptr(), o.data_ptr(), level, 1, good, -1), "mode"), ((x.data_ptr(), o.data_ptr(), 4, 1, good, 0), "level 4")):
            assert lib.ndwt_denoise_neigh(plan._h, *args, None) == INVALID and word in err(), (word, err())
        # what the kernel does not serve
        inter = ndwt.Plan([16, 16], ["db1", "db1"], torch.float32, False, max_level=1, inner=3, howmany=2)
        four = ndwt.Plan([8, 8, 8, 8], ["db1"] * 4, torch.float32, False, max_level=1)
        short = ndwt.Plan([16, 4], ["db1", "db1"], torch.float32, False, max_level=1)
        g4, g16 = dbl(*[1.0] * 4), dbl(*[1.0] * 16)
        big = torch.zeros(16 * 4096, device="cuda")
        bo = torch.full_like(big, -2.0)
        for p, t, rad, word in ((inter, g4, 1, "interleaved"), (four, g16, 1, "filtered axes"), (short, g4, 2, "filtered axis 1 has 4 elements")):
            assert lib.ndwt_shrink_neigh(p._h, big.data_ptr(), bo.data_ptr(), 0, 1, rad, t, 0, None) == UNSUPPORTED and word in err(), (word, err())
            assert lib.ndwt_denoise_neigh(p._h, big.data_ptr(), bo.data_ptr(), 1, rad, t, 0, None) == UNSUPPORTED and word in err(), (word, err())
        assert lib.ndwt_shrink_neigh(short._h, big.data_ptr(), bo.data_ptr(), 0, 1, 1, g4, 0, None) == 0          # (radius 1 fits the axis of 4)
    assert [q.family for q in recs] == ["NeighShrink"]           # the one call that was served
    assert (o == -2.0).all().item() and a.unchanged() and (a.out == OUT_FILL).all().item() and (bo[64 * 4:] == -2.0).all().item()
    with pytest.raises(ndwt.NdwtError, match="radius 7"):
        plan.shrink_neigh(a.ptr, a.optr, level, [0.0, 1.0, 1.0], 7, False, stream())
    with pytest.raises(ValueError):
        plan.shrink_neigh(a.ptr, a.optr, level, [0.0, 1.0], 1, False, stream())          # two thresholds for three bands
