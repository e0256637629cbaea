"""Joint shrinkage across the items of a plan and the group norms on the device: ndwt_shrink_joint, ndwt_denoise_joint, ndwt_group_norms,
ndwt_group_norms_dev and the classes' shrink / denoise(joint=True), group_norms and l21_norm.

The shrink and the norms need no transform: the coefficient array is ARBITRARY DATA written by the test (tests/joint_cases.py: random
items, an all-equal item, an item with a NaN, an all-zero item with one -0, an integer-valued last band), the plan only supplies the
sizes, the items and the data kind.  Every array lies between guard words, the bands on a pitch have guard words between them, and the
whole buffer is compared afterwards.  The shapes are the smallest at which each form of the kernels can go wrong:

  batch 5 x 37, db2, float, level 2                     element-wise, the group in registers
  batch 5 x 96, db2, complex64, level 3                 the 4-scalar form, 4 bands
  batch (KREG + 1) x 96 and 40 x 96, db2, float         the first plan of two sweeps; many turns of the load queue
  batch 2 x 20000, db4, float and double, level 1       4 chunks, the last one ragged, so NormsFinish runs
  stack 8 x 12 x 3 items, db2, complex128, level 2      7 bands on a pitch, guard words between and behind the bands
  interleaved, inner = 3, 16 x 16 x 2 and 15 x 15 x 2   the items of ndwt_plan_create_interleaved; 675 scalars: no multiple of 4
  3-D 8 x 8 x 8, db2, double, level 2                   one item: the group is the element; one element off a 32-byte boundary
  1-D n = 37, complex64, level 2                        one complex item, element-wise

  values     soft and hard against tests/joint_cases.py (bit for bit; the double kinds also within the bound derived there against the
             plain numpy loop); a band with threshold 0 and every guard word untouched
  norms      nnz and max exactly, l1 and l2sq to the derived tolerance; group_norms_dev equals the host form bit for bit; two calls
             return the same bits; the array is read only
  together   a hard joint shrink at t = max[b] zeros band b; after a hard shrink at t, nnz[b] is numpy's count of m > t; on a real plan
             of one item hard mode equals shrink_bands bit for bit; denoise_joint equals dec -> shrink_joint -> rec bit for bit
  trace      exactly one JointShrink record for all bands with the grid joint_chunks gives, none for an all-zero array; one GroupNorms
             record, and NormsFinish only where a band has more than one chunk
  classes    shrink / denoise(joint=True), group_norms and l21_norm against the same reference; joint=False is the call without it
  refusals   name the argument and launch nothing
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
from items_cases import build_named_shim
from joint_cases import (band_view, check_group_norms, check_shrink, joint_array, magnitudes, median_thresholds, reference_norms, reference_shrink,
                         sum_squares)
from norms_cases import L1, MAX, NNZ
from select_cases import KINDS

pytestmark = pytest.mark.gpu

GUARD = 8                                                     # scalars before and after an array (32 / 64 bytes: the alignment stays)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_named_shim(tmp_path_factory, "joint_shim")
    lib.sel_joint_chunks.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_joint_chunks.restype = ctypes.c_longlong
    return lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def torch_real(kind):
    return torch.float32 if KINDS[kind][0] == np.float32 else torch.float64


def tname(kind):
    return "float" if KINDS[kind][0] == np.float32 else "double"


# -> (plan, items, elements of one item, filtered axes, level, pitched, skew in elements, the 4-scalar form)
def make_case(kind, shape):
    rdt, cplx = torch_real(kind), KINDS[kind][1]
    if shape == "1d-37":
        return ndwt.Plan([37], ["db2"], rdt, cplx, max_level=2), 1, 37, 1, 2, False, 0, False
    if shape == "batch-5x37":
        return ndwt.Plan([37], ["db2"], rdt, cplx, max_level=2, howmany=5), 5, 37, 1, 2, False, 0, False
    if shape == "batch-5x96":
        return ndwt.Plan([96], ["db2"], rdt, cplx, max_level=3, howmany=5), 5, 96, 1, 3, False, 0, True
    if shape in ("batch-9x96", "batch-40x96"):
        k = int(shape[6:].split("x")[0])
        return ndwt.Plan([96], ["db2"], rdt, cplx, max_level=2, howmany=k), k, 96, 1, 2, False, 0, True
    if shape == "batch-2x20000":
        return ndwt.Plan([20000], ["db4"], rdt, cplx, max_level=1, howmany=2), 2, 20000, 1, 1, False, 0, True
    if shape == "stack-3x8x12":
        return ndwt.Plan([8, 12, 3], ["db2", "db2", None], rdt, cplx, max_level=2, axes=(0, 1)), 3, 96, 2, 2, True, 0, True
    if shape == "3d-8x8x8-skew":
        return ndwt.Plan([8, 8, 8], ["db2"] * 3, rdt, cplx, max_level=2), 1, 512, 3, 2, False, 1, False
    if shape == "inner-3-16x16":
        return ndwt.Plan([16, 16], ["db1", "db1"], rdt, cplx, max_level=1, inner=3, howmany=2), 2, 768, 2, 1, False, 0, True
    if shape == "inner-3-15x15":
        return ndwt.Plan([15, 15], ["db1", "db1"], rdt, cplx, max_level=1, inner=3, howmany=2), 2, 675, 2, 1, False, 0, False
    raise ValueError(shape)


CASES = [("f32", "batch-5x37"), ("c64", "batch-5x96"), ("f32", "batch-9x96"), ("f32", "batch-40x96"), ("f32", "batch-2x20000"), ("f64", "batch-2x20000"),
         ("c128", "stack-3x8x12"), ("f32", "inner-3-16x16"), ("f32", "inner-3-15x15"), ("f64", "3d-8x8x8-skew"), ("c64", "1d-37")]


def test_kreg_is_the_librarys(shim):
    assert shim.sel_joint_reg() == 8 and "batch-9x96" in [s for _, s in CASES]   # (KREG + 1 items: the first plan of two sweeps)


class Coefs:
    """a coefficient array of tests/joint_cases.py between GUARD scalars of filler (and `skew` elements further), with its thresholds; the
    host copy stays as it is, every device() is a fresh copy of it"""

    def __init__(self, kind, items, N, nb, pitch_elements, seed, skew=0):
        rdt, cplx = KINDS[kind]
        self.kind, self.items, self.N, self.nb = kind, items, N, nb
        self.comp = 2 if cplx else 1
        n = items * N * self.comp
        self.bs = (pitch_elements or items * N) * self.comp
        self.ints = (nb - 1,) if nb >= 3 else ()
        self.zero = (1,) if nb >= 3 else ()
        self.flat, pitch = joint_array(kind, items, N, nb, self.bs - n, seed, integer_bands=self.ints)
        assert pitch == self.bs
        self.thr = median_thresholds(kind, self.flat, self.bs, items, N, nb, zero_bands=self.zero)
        self.off = GUARD + skew * self.comp
        self.host = np.full(self.off + nb * self.bs + GUARD, 1e30, dtype=rdt)
        self.host[self.off:self.off + nb * self.bs] = self.flat
        self.host.setflags(write=False)
        self.device()

    def device(self):
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.ptr = self.dev.data_ptr() + self.off * self.host.itemsize
        return self

    def get(self):
        """(the array as it is on the device, whether everything around it is untouched)"""
        h = self.dev.cpu().numpy()
        inner = slice(self.off, self.off + self.nb * self.bs)
        return h[inner].copy(), h[:self.off].tobytes() == self.host[:self.off].tobytes() and h[inner.stop:].tobytes() == self.host[inner.stop:].tobytes()

    def unchanged(self):
        return self.dev.cpu().numpy().tobytes() == self.host.tobytes()


_COEFS = {}


def coefs(kind, shape):
    """(the case, its array): the array and its reference inputs are made once and shared by the tests"""
    plan, items, N, axes, level, pitched, skew, vec = make_case(kind, shape)
    nb = ndwt.num_bands(axes, level)
    pitch = plan.band_pitch() + 4 if pitched else 0               # (4 elements on top: guard words between the bands whatever the plan's pitch)
    if (kind, shape) not in _COEFS:
        _COEFS[(kind, shape)] = Coefs(kind, items, N, nb, pitch, zlib.crc32(f"{kind}-{shape}".encode()) % 100000, skew)
    c = _COEFS[(kind, shape)].device()
    comp = c.comp
    assert plan.items == items and (not pitched or c.bs > items * N * comp)
    assert vec == (c.ptr % (4 * c.host.itemsize) == 0 and c.bs % 4 == 0 and (N * comp) % 4 == 0)
    return plan, items, N, nb, level, pitch, vec, c


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_the_whole_buffer_after_the_joint_shrink(shim, kind, shape):
    rdt, cplx = KINDS[kind]
    plan, items, N, nb, level, pitch, vec, c = coefs(kind, shape)
    comp, n = c.comp, N * c.comp
    chunks = int(shim.sel_joint_chunks(n, comp, int(vec), nb, items, cus(), 0))
    assert chunks == (4 if shape == "batch-2x20000" else 1)
    want = {"T": tname(kind), "COMP": comp, "VEC": vec, "REG": items <= shim.sel_joint_reg()}
    for hard in (False, True):
        c.device()
        with ndwt.kernel_trace() as recs:
            plan.shrink_joint(c.ptr, level, c.thr, hard, stream(), band_pitch=pitch)
        assert len(recs) == 1 and recs[0].family == "JointShrink" and recs[0].params == want, recs
        assert recs[0].grid == (nb * chunks, 1, 1) and recs[0].block == (256, 1, 1), (recs[0], chunks)
        got, outside = c.get()
        assert outside
        check_shrink(kind, c.flat, got, c.bs, items, N, nb, c.thr, hard, integer_bands=c.ints, what=f"{kind}-{shape} hard={hard}")
        for b in c.zero:                                          # (in check_shrink's comparison too; said once more: threshold 0)
            assert same(got[b * c.bs:(b + 1) * c.bs], c.flat[b * c.bs:(b + 1) * c.bs])
        if not hard:
            continue
        # after a hard shrink at t the groups that are not zero are those with m > t
        v = plan.group_norms(c.ptr, level, stream(), band_pitch=pitch)
        for b in range(nb):
            if c.thr[b] > 0:
                m = magnitudes(kind, sum_squares(kind, band_view(kind, c.flat, c.bs, items, N, b), True))
                assert v[b, NNZ] == np.count_nonzero(m > KINDS[kind][0](c.thr[b])), (b, v[b])
        if items == 1 and not cplx:
            # one real item: the group is the element, and hard mode is ndwt_shrink_bands bit for bit
            c.device()
            plan.shrink_bands(c.ptr, level, c.thr, True, stream(), band_pitch=pitch)
            assert same(c.get()[0], got)
    # an all-zero array of thresholds launches nothing
    c.device()
    with ndwt.kernel_trace() as recs:
        plan.shrink_joint(c.ptr, level, np.zeros(nb), False, stream(), band_pitch=pitch)
    assert recs == [] and c.unchanged()


@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_the_group_norms_of_every_band(shim, kind, shape):
    plan, items, N, nb, level, pitch, vec, c = coefs(kind, shape)
    comp, n = c.comp, N * c.comp
    chunks = int(shim.sel_joint_chunks(n, comp, int(vec), nb, items, cus(), 0))

    def traced(f):
        """f() with its trace checked: one GroupNorms on bands x chunks workgroups, and one NormsFinish where chunks > 1"""
        with ndwt.kernel_trace() as recs:
            out = f()
        assert len(recs) == (1 if chunks == 1 else 2), recs
        assert recs[0].family == "GroupNorms" and recs[0].params == {"T": tname(kind), "COMP": comp, "VEC": vec}, recs[0]
        assert recs[0].grid == (nb * chunks, 1, 1) and recs[0].block == (256, 1, 1), (recs[0], chunks)
        if chunks > 1:
            assert recs[1].family == "NormsFinish" and recs[1].grid == (nb, 1, 1) and recs[1].block == (64, 1, 1), recs[1]
        return out

    v = traced(lambda: plan.group_norms(c.ptr, level, stream(), band_pitch=pitch))
    assert v.shape == (nb, 4)
    check_group_norms(kind, c.flat, v, c.bs, items, N, nb, integer_bands=c.ints, what=f"{kind}-{shape}")
    assert same(plan.group_norms(c.ptr, level, stream(), band_pitch=pitch), v)       # the order of every sum is fixed
    raw = torch.full((1 + nb * 4 + 1,), -3.0, dtype=torch.float64, device="cuda")
    traced(lambda: plan.group_norms_dev(c.ptr, level, raw.data_ptr() + 8, stream(), band_pitch=pitch))
    got = raw.cpu().numpy()
    assert same(got[1:1 + v.size], v.reshape(-1)) and got[0] == -3.0 and got[-1] == -3.0
    assert c.unchanged()                                          # the array, the guard words between and around the bands
    if items == 1:
        # one item: the group is the element.  The count is that of the band norms; for real data so are max and l1 (sqrt(c^2) = |c|,
        # added in the same order).  (l2sq is not: the band norms fuse every square into the running sum, here s is rounded first.)
        bn = plan.band_norms(c.ptr, level, stream(), band_pitch=pitch)
        assert same(bn[:, NNZ], v[:, NNZ])
        if comp == 1:
            assert same(bn[:, MAX], v[:, MAX]) and same(bn[:, L1], v[:, L1])
    # a hard joint shrink at t = max[b] zeros band b and nothing else (the last band: it holds no NaN)
    b = nb - 1
    thr = np.zeros(nb)
    thr[b] = v[b, MAX]
    assert thr[b] > 0
    plan.shrink_joint(c.ptr, level, thr, True, stream(), band_pitch=pitch)
    got, outside = c.get()
    want = c.flat.copy()
    want[b * c.bs:b * c.bs + items * n] = 0
    assert outside and same(got, want)
    after = plan.group_norms(c.ptr, level, stream(), band_pitch=pitch)
    assert after[b].tolist() == [0.0, 0.0, 0.0, 0.0] and same(after[:b], v[:b])


DENOISE_CASES = [("c64", "batch-5x96"), ("f32", "batch-9x96"), ("c128", "stack-3x8x12"), ("f32", "inner-3-16x16"), ("f64", "3d-8x8x8-skew")]


@pytest.mark.parametrize("kind,shape", DENOISE_CASES, ids=[f"{k}-{s}" for k, s in DENOISE_CASES])
def test_denoise_joint_is_dec_shrink_joint_rec(kind, shape):
    rdt, cplx = KINDS[kind]
    plan, items, N, axes, level, _, _, _ = make_case(kind, shape)
    comp = 2 if cplx else 1
    nb = ndwt.num_bands(axes, level)
    rng = np.random.default_rng(zlib.crc32(f"den-{kind}-{shape}".encode()))
    xh = rng.standard_normal(items * N * comp).astype(rdt)
    x = torch.from_numpy(xh).cuda()
    pitch = plan.band_pitch()
    y = torch.zeros(nb * pitch * comp, dtype=x.dtype, device="cuda")
    thr = np.full(nb, 0.6)
    thr[0] = 0.0
    for hard in (False, True):
        out, ref = torch.full_like(x, 7.0), torch.full_like(x, -7.0)
        with ndwt.kernel_trace() as recs:
            plan.denoise_joint(x.data_ptr(), out.data_ptr(), level, thr, hard, stream())
        fams = [r.family for r in recs]
        assert fams.count("JointShrink") == 1 and "shrink_kernel" not in fams and "ShrinkItems" not in fams and "Den1C" not in fams, fams
        plan.dec(x.data_ptr(), y.data_ptr(), level, stream(), band_pitch=pitch)
        plan.shrink_joint(y.data_ptr(), level, thr, hard, stream(), band_pitch=pitch)
        plan.rec(y.data_ptr(), ref.data_ptr(), level, stream(), band_pitch=pitch)
        assert torch.equal(out, ref) and bool(torch.isfinite(out).all()) and not torch.equal(out, x)
        assert same(x.cpu().numpy(), xh)


def test_the_classes_take_joint_and_keep_their_other_forms():
    K, n, level = 5, 96, 3
    for prec, cplx, kind in (("single", False, "f32"), ("double", True, "c128")):
        w = ndwt.nd_dwt_1D("db2", n, "batch", K, "precision", prec)
        nb = ndwt.num_bands(1, level)
        rng = np.random.default_rng(71)
        x = rng.standard_normal((n, K)) + (1j * rng.standard_normal((n, K)) if cplx else 0)
        xt = torch.from_numpy(x.astype(np.complex128 if cplx else np.float32)).cuda()      # MATLAB shape [n, K]
        y = w.dec(xt, level)                                        # [n, K, bands]
        yk = y.permute(2, 1, 0).contiguous()                        # kernel order: [bands, K, n]
        flat = (torch.view_as_real(yk) if cplx else yk).cpu().numpy().reshape(-1)
        pitch = K * n * (2 if cplx else 1)
        thr = np.array([0.0, 0.9, 0.0, 1.4])
        plan = w._plan(cplx, level, xt.device)
        xk = xt.permute(1, 0).contiguous()
        for mode in ("soft", "hard"):
            for t, tv in ((thr, thr), (torch.from_numpy(thr), thr), (1.1, np.array([0.0, 1.1, 1.1, 1.1]))):
                got = w.shrink(y, t, mode, joint=True)
                assert got.shape == y.shape and got.dtype == y.dtype
                gk = got.permute(2, 1, 0).contiguous()
                gflat = (torch.view_as_real(gk) if cplx else gk).cpu().numpy().reshape(-1)
                assert same(gflat, reference_shrink(kind, flat, pitch, K, n, nb, tv, mode == "hard", fused=True))
                ok = torch.empty_like(xk)
                plan.denoise_joint(xk.data_ptr(), ok.data_ptr(), level, tv, mode == "hard", stream())
                assert torch.equal(w.denoise(xt, level, t, mode, joint=True).permute(1, 0).contiguous(), ok)
            # joint=False is the call without the argument: bands, rows per item and the scalar
            rows = np.tile(thr, (K, 1)) * np.arange(1, K + 1)[:, None]
            for t in (thr, rows, 0.7):
                assert torch.equal(w.shrink(y, t, mode, joint=False), w.shrink(y, t, mode))
                assert torch.equal(w.denoise(xt, level, t, mode, joint=False), w.denoise(xt, level, t, mode))
            assert not torch.equal(w.shrink(y, thr, mode, joint=True), w.shrink(y, thr, mode))
        assert same(yk.cpu().numpy(), y.permute(2, 1, 0).contiguous().cpu().numpy())     # shrink returns a new array
        # the norms of the groups
        ref = reference_norms(kind, flat, pitch, K, n, nb, fused=True)
        v = w.group_norms(y)
        assert set(v) == {"l1", "l2sq", "max", "nnz"} and all(v[k].shape == (nb,) for k in v)
        check_group_norms(kind, flat, np.stack([v["l1"], v["l2sq"], v["max"], v["nnz"]], axis=1), pitch, K, n, nb, what=f"class {kind}")
        tol = n * 2.0 ** -52
        wts = np.arange(1.0, nb + 1)
        assert isinstance(w.l21_norm(y), float)
        assert abs(w.l21_norm(y) - ref[1:, L1].sum()) <= 2 * tol * ref[1:, L1].sum()
        assert abs(w.l21_norm(y, wts) - ref[:, L1] @ wts) <= 2 * tol * (ref[:, L1] @ wts)
        # the prox shrinks the norm it belongs to
        assert w.l21_norm(w.shrink(y, 0.5, joint=True)) < w.l21_norm(y)
    with pytest.raises(ValueError, match="joint=True takes a scalar or 4 thresholds"):
        w.shrink(y, np.ones((K, nb)), joint=True)


def test_every_refusal_names_its_argument_and_launches_nothing():
    plan = ndwt.Plan([96], ["db2"], torch.float32, False, max_level=3, howmany=5)
    items, N, level, nb = 5, 96, 2, 3
    c = Coefs("f32", items, N, nb, 0, 5)
    lib = ndwt.lib()
    err = lambda: lib.ndwt_last_error().decode()
    dbl = lambda *a: (ctypes.c_double * len(a))(*a)
    good, v = dbl(0.0, 1.0, 1.0), dbl(*[-1.0] * 64)
    x = torch.full((items * N,), 2.0, device="cuda")
    out = torch.full((64,), -2.0, dtype=torch.float64, device="cuda")
    o = torch.full((items * N,), -2.0, device="cuda")
    with ndwt.kernel_trace() as recs:
        for args, word in (((None, 0, level, good, 0), "y_dev"), ((c.ptr, 0, level, None, 0), "null thresholds"),
                           ((c.ptr, 0, level, dbl(0.0, -1.0, 1.0), 0), "threshold of band 1"), ((c.ptr, 0, level, dbl(0.0, 1.0, float("nan")), 1), "threshold of band 2"),
                           ((c.ptr, 0, level, good, 2), "mode"), ((c.ptr, 0, 0, good, 0), "level 0"), ((c.ptr, 0, 4, good, 0), "level 4"),
                           ((c.ptr, items * N - 1, level, good, 0), "pitch")):
            assert lib.ndwt_shrink_joint(plan._h, *args, None) == 1 and word in err(), (word, err())
        for args, word in (((None, o.data_ptr(), level, good, 0), "x_dev"), ((x.data_ptr(), None, level, good, 0), "out_dev"),
                           ((x.data_ptr(), o.data_ptr(), level, None, 0), "null thresholds"), ((x.data_ptr(), o.data_ptr(), level, dbl(-0.5, 1.0, 1.0), 0), "threshold of band 0"),
                           ((x.data_ptr(), o.data_ptr(), level, good, -1), "mode"), ((x.data_ptr(), o.data_ptr(), 4, good, 0), "level 4")):
            assert lib.ndwt_denoise_joint(plan._h, *args, None) == 1 and word in err(), (word, err())
        for args, word in (((None, 0, level, v), "y_dev"), ((c.ptr, 0, level, None), "(norms)"), ((c.ptr, 0, 0, v), "level 0"), ((c.ptr, 0, 4, v), "level 4"),
                           ((c.ptr, items * N - 1, level, v), "pitch")):
            assert lib.ndwt_group_norms(plan._h, *args, None) == 1 and word in err(), (word, err())
        for args, word in (((None, 0, level, out.data_ptr()), "y_dev"), ((c.ptr, 0, level, None), "norms_dev"),
                           ((c.ptr, 0, level, out.data_ptr() + 4), "norms_dev must be 8-byte aligned"), ((c.ptr, 0, 4, out.data_ptr()), "level 4"),
                           ((c.ptr, items * N - 1, level, out.data_ptr()), "pitch")):
            assert lib.ndwt_group_norms_dev(plan._h, *args, None) == 1 and word in err(), (word, err())
    assert recs == [] and list(v) == [-1.0] * 64 and (out == -2.0).all().item() and (o == -2.0).all().item() and c.unchanged()
    with pytest.raises(ndwt.NdwtError, match="level 4"):
        plan.group_norms(c.ptr, 4, stream())
    with pytest.raises(ndwt.NdwtError, match="threshold of band 1"):
        plan.shrink_joint(c.ptr, level, [0.0, -2.0, 1.0], False, stream())
    with pytest.raises(ValueError):
        plan.shrink_joint(c.ptr, level, [0.0, 1.0], False, stream())        # two thresholds for three bands
