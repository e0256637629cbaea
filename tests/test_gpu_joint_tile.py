"""The tile form of the joint shrinkage and the group norms on the device (JointTile / GroupNormsTile, csrc/ndwt_device_joint_tile.h): the
route ndwt_plan_set_variant(plan, *, 11, ...) forces, against the reference of tests/joint_cases.py and against the chunk form of the same
plan (variant 9), bit for bit.

The coefficient array is ARBITRARY DATA written by the test (joint_cases.joint_array: random items, an all-equal item, an item with a NaN,
an all-zero item with one -0, an integer-valued last band), between guard words and, on a pitch, with guard words between the bands; the
whole buffer is compared.  J (the items of an LDS tile) and SW (the steps of a strip) are the kernels' own, read from
tests/select/joint_tile_shim.cpp; a pass loads 256 / SW items.  The shapes are the smallest at which each form can go wrong:

  batch (3 J + 5) x 96, db2, float, level 2            the 4-scalar form, 3 bands, 24 steps, more than three tiles, the last ragged
  batch J x 96 and (J + 1) x 96, float                  the tile boundary exactly, and one past it
  batch 5 x 96, float                                   fewer items than a pass: rows that load nothing
  batch (J + 3) x 96, complex64, level 3                two positions a step
  batch 70 x 37, complex64, level 2                     element-wise complex, a ragged last strip
  batch (2 J + 1) x 100, double, level 1                25 steps: a ragged last strip in the 4-scalar form
  stack 8 x 12 x (J + 3), complex128, level 2, pitched  7 bands, guard words between them
  interleaved, inner = 3, 15 x 15 and 16 x 16, J + 2    675 scalars (no multiple of 4) and 768
  3-D 8 x 8 x 8, double, one element off 32 bytes       one item: the group is the element

  values    soft and hard: the whole buffer bit-equal to the reference (the double kinds also within the derived bound of the plain numpy
            loop) AND to the same plan's result under variant 9; a zero-threshold band and every guard word untouched; an all-zero
            threshold array launches nothing
  norms     nnz and max exact, l1 and l2sq to joint_cases' tolerance; nnz and max are variant 9's bits; group_norms_dev equals the host form
            bit for bit; two calls return the same bits; the array is unchanged
  trace     under 11 exactly one JointTile record on bands x joint_tile_strips workgroups of 256 and no JointShrink; one GroupNormsTile
            record, and NormsFinish only where a band has more than one strip; under 9 the old families; under 0 what joint_route says
  together  denoise_joint under 11 equals dec -> shrink_joint -> rec on the same plan bit for bit; a hard shrink at t = max[b] zeros band
            b; the classes' shrink(y, t, joint=True) on a forced plan matches the reference
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
from items_cases import build_named_shim
from joint_cases import check_group_norms, check_shrink, reference_shrink
from norms_cases import MAX, NNZ
from select_cases import KINDS
from test_gpu_joint import Coefs, cus, same, stream, tname, torch_real

pytestmark = pytest.mark.gpu

TILE, CHUNKS, DEFAULT = 11, 9, 0


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_named_shim(tmp_path_factory, "joint_tile_shim")
    lib.sel_joint_route.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_joint_tile_strips.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_joint_tile_strips.restype = ctypes.c_longlong
    return lib


# -> (plan, items, elements of one item, filtered axes, level, pitched, skew in elements, the 4-scalar form)
def make_case(shim, kind, shape):
    rdt, cplx = torch_real(kind), KINDS[kind][1]
    J = shim.sel_joint_tile_j()
    batch = lambda k, n, level: ndwt.Plan([n], ["db2"], rdt, cplx, max_level=level, howmany=k)   # noqa: E731
    if shape == "batch-3J+5x96":
        return batch(3 * J + 5, 96, 2), 3 * J + 5, 96, 1, 2, False, 0, True
    if shape == "batch-Jx96":
        return batch(J, 96, 2), J, 96, 1, 2, False, 0, True
    if shape == "batch-J+1x96":
        return batch(J + 1, 96, 2), J + 1, 96, 1, 2, False, 0, True
    if shape == "batch-5x96":
        return batch(5, 96, 2), 5, 96, 1, 2, False, 0, True
    if shape == "batch-J+3x96-L3":
        return batch(J + 3, 96, 3), J + 3, 96, 1, 3, False, 0, True
    if shape == "batch-70x37":
        return batch(70, 37, 2), 70, 37, 1, 2, False, 0, False
    if shape == "batch-2J+1x100-L1":
        return batch(2 * J + 1, 100, 1), 2 * J + 1, 100, 1, 1, False, 0, True
    if shape == "stack-J+3x8x12":
        return ndwt.Plan([8, 12, J + 3], ["db2", "db2", None], rdt, cplx, max_level=2, axes=(0, 1)), J + 3, 96, 2, 2, True, 0, True
    if shape == "inner-3-16x16":
        return ndwt.Plan([16, 16], ["db1", "db1"], rdt, cplx, max_level=1, inner=3, howmany=J + 2), J + 2, 768, 2, 1, False, 0, True
    if shape == "inner-3-15x15":
        return ndwt.Plan([15, 15], ["db1", "db1"], rdt, cplx, max_level=1, inner=3, howmany=J + 2), J + 2, 675, 2, 1, False, 0, False
    if shape == "3d-8x8x8-skew":
        return ndwt.Plan([8, 8, 8], ["db2"] * 3, rdt, cplx, max_level=2), 1, 512, 3, 2, False, 1, False
    raise ValueError(shape)


CASES = [("f32", "batch-3J+5x96"), ("f32", "batch-Jx96"), ("f32", "batch-J+1x96"), ("f32", "batch-5x96"), ("c64", "batch-J+3x96-L3"), ("c64", "batch-70x37"),
         ("f64", "batch-2J+1x100-L1"), ("c128", "stack-J+3x8x12"), ("f32", "inner-3-15x15"), ("f32", "inner-3-16x16"), ("f64", "3d-8x8x8-skew")]
IDS = [f"{k}-{s}" for k, s in CASES]
_COEFS = {}


def coefs(shim, kind, shape):
    """(the case, its array): the array and its reference inputs are made once and shared by the tests"""
    plan, items, N, axes, level, pitched, skew, vec = make_case(shim, kind, shape)
    nb = ndwt.num_bands(axes, level)
    pitch = plan.band_pitch() + 4 if pitched else 0               # (4 elements on top: guard words between the bands whatever the plan's pitch)
    if (kind, shape) not in _COEFS:
        _COEFS[(kind, shape)] = Coefs(kind, items, N, nb, pitch, zlib.crc32(f"tile-{kind}-{shape}".encode()) % 100000, skew)
    c = _COEFS[(kind, shape)].device()
    assert plan.items == items and (not pitched or c.bs > items * N * c.comp)
    assert vec == (c.ptr % (4 * c.host.itemsize) == 0 and c.bs % 4 == 0 and (N * c.comp) % 4 == 0)
    strips = int(shim.sel_joint_tile_strips(N * c.comp, c.comp, int(vec)))
    return plan, items, N, nb, level, pitch, vec, c, strips


def test_the_shapes_cover_what_they_say(shim):
    J, SW = shim.sel_joint_tile_j(), shim.sel_joint_tile_sw()
    assert 256 % SW == 0 and J % (256 // SW) == 0 and 5 < 256 // SW     # (5 items: fewer than a pass)
    assert shim.sel_joint_tile_strips(100, 1, 1) * SW > 25 >= SW         # 25 steps: a ragged last strip, more than one strip
    assert shim.sel_joint_tile_strips(74, 2, 0) * SW > 37 > SW           # 37 elements: likewise, element-wise
    assert shim.sel_joint_tile_strips(512, 1, 0) > 1


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_the_whole_buffer_after_the_tile_form(shim, kind, shape):
    plan, items, N, nb, level, pitch, vec, c, strips = coefs(shim, kind, shape)
    want = {"T": tname(kind), "COMP": c.comp, "VEC": vec}
    for hard in (False, True):
        c.device()
        plan.set_variant(-1, TILE)
        with ndwt.kernel_trace() as recs:
            plan.shrink_joint(c.ptr, level, c.thr, hard, stream(), band_pitch=pitch)
        assert len(recs) == 1 and recs[0].family == "JointTile" and recs[0].params == want, recs
        assert recs[0].grid == (nb * strips, 1, 1) and recs[0].block == (256, 1, 1), (recs[0], strips)
        got, outside = c.get()
        assert outside
        check_shrink(kind, c.flat, got, c.bs, items, N, nb, c.thr, hard, integer_bands=c.ints, what=f"{kind}-{shape} hard={hard}")
        for b in c.zero:                                          # (in check_shrink's comparison too; said once more: threshold 0)
            assert same(got[b * c.bs:(b + 1) * c.bs], c.flat[b * c.bs:(b + 1) * c.bs])
        # the chunk form of the same plan: the same bits
        c.device()
        plan.set_variant(-1, CHUNKS)
        with ndwt.kernel_trace() as recs:
            plan.shrink_joint(c.ptr, level, c.thr, hard, stream(), band_pitch=pitch)
        assert [r.family for r in recs] == ["JointShrink"], recs
        old, outside = c.get()
        assert outside and same(old, got)
    # an all-zero array of thresholds launches nothing
    c.device()
    plan.set_variant(-1, TILE)
    with ndwt.kernel_trace() as recs:
        plan.shrink_joint(c.ptr, level, np.zeros(nb), False, stream(), band_pitch=pitch)
    assert recs == [] and c.unchanged()


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_the_group_norms_of_the_tile_form(shim, kind, shape):
    plan, items, N, nb, level, pitch, vec, c, strips = coefs(shim, kind, shape)
    plan.set_variant(-1, TILE)

    def traced(f):
        """f() with its trace checked: one GroupNormsTile on bands x strips workgroups, and one NormsFinish where strips > 1"""
        with ndwt.kernel_trace() as recs:
            out = f()
        assert len(recs) == (1 if strips == 1 else 2), recs
        assert recs[0].family == "GroupNormsTile" and recs[0].params == {"T": tname(kind), "COMP": c.comp, "VEC": vec}, recs[0]
        assert recs[0].grid == (nb * strips, 1, 1) and recs[0].block == (256, 1, 1), (recs[0], strips)
        if strips > 1:
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
    # every group's s and m are the chunk form's: its count and its max are the same bits
    plan.set_variant(-1, CHUNKS)
    with ndwt.kernel_trace() as recs:
        old = plan.group_norms(c.ptr, level, stream(), band_pitch=pitch)
    assert recs[0].family == "GroupNorms" and all(r.family in ("GroupNorms", "NormsFinish") for r in recs), recs
    assert same(old[:, NNZ], v[:, NNZ]) and same(old[:, MAX], v[:, MAX])
    # a hard joint shrink at t = max[b] zeros band b and nothing else (the integer-valued last band: it holds no NaN; the two bands of
    # the level-1 case both hold one, their max is a NaN and no threshold)
    plan.set_variant(-1, TILE)
    if not c.ints:
        assert nb == 2 and np.isnan(v[:, MAX]).all()
        return
    b = nb - 1
    thr = np.zeros(nb)
    thr[b] = v[b, MAX]
    assert thr[b] > 0
    plan.shrink_joint(c.ptr, level, thr, True, stream(), band_pitch=pitch)
    got, outside = c.get()
    want = c.flat.copy()
    want[b * c.bs:b * c.bs + items * N * c.comp] = 0
    assert outside and same(got, want)
    after = plan.group_norms(c.ptr, level, stream(), band_pitch=pitch)
    assert after[b].tolist() == [0.0, 0.0, 0.0, 0.0] and same(after[:b], v[:b])


@pytest.mark.parametrize("kind,shape", [("f32", "batch-3J+5x96"), ("f32", "batch-5x96"), ("f64", "batch-2J+1x100-L1")], ids=["many", "few", "double"])
def test_the_default_route_is_what_joint_route_says(shim, kind, shape):
    plan, items, N, nb, level, pitch, vec, c, strips = coefs(shim, kind, shape)
    plan.set_variant(-1, DEFAULT)
    tile = bool(shim.sel_joint_route(N * c.comp, c.comp, int(vec), nb, items, cus(), DEFAULT))
    assert not (tile and items < shim.sel_joint_tile_from())
    with ndwt.kernel_trace() as recs:
        plan.shrink_joint(c.ptr, level, c.thr, False, stream(), band_pitch=pitch)
        plan.group_norms(c.ptr, level, stream(), band_pitch=pitch)
    fams = [r.family for r in recs if r.family != "NormsFinish"]
    assert fams == (["JointTile", "GroupNormsTile"] if tile else ["JointShrink", "GroupNorms"]), (fams, tile)
    if tile:
        assert recs[0].grid == (nb * strips, 1, 1)


DENOISE_CASES = [("f32", "batch-J+1x96"), ("c64", "batch-J+3x96-L3"), ("c128", "stack-J+3x8x12"), ("f32", "inner-3-16x16")]


@pytest.mark.parametrize("kind,shape", DENOISE_CASES, ids=[f"{k}-{s}" for k, s in DENOISE_CASES])
def test_denoise_joint_under_the_tile_form_is_dec_shrink_joint_rec(shim, kind, shape):
    rdt, cplx = KINDS[kind]
    plan, items, N, axes, level, _, _, _ = make_case(shim, kind, shape)
    plan.set_variant(-1, TILE)
    comp = 2 if cplx else 1
    nb = ndwt.num_bands(axes, level)
    rng = np.random.default_rng(zlib.crc32(f"den-tile-{kind}-{shape}".encode()))
    xh = rng.standard_normal(items * N * comp).astype(rdt)
    x = torch.from_numpy(xh).cuda()
    pitch = plan.band_pitch()
    y = torch.zeros(nb * pitch * comp, dtype=x.dtype, device="cuda")
    thr = np.full(nb, 0.6 * np.sqrt(items))                       # (a group of `items` coefficients of about unit size)
    thr[0] = 0.0
    for hard in (False, True):
        out, ref = torch.full_like(x, 7.0), torch.full_like(x, -7.0)
        with ndwt.kernel_trace() as recs:
            plan.denoise_joint(x.data_ptr(), out.data_ptr(), level, thr, hard, stream())
        fams = [r.family for r in recs]
        assert fams.count("JointTile") == 1 and "JointShrink" not in fams and "shrink_kernel" not in fams and "ShrinkItems" not in fams, fams
        plan.dec(x.data_ptr(), y.data_ptr(), level, stream(), band_pitch=pitch)
        plan.shrink_joint(y.data_ptr(), level, thr, hard, stream(), band_pitch=pitch)
        plan.rec(y.data_ptr(), ref.data_ptr(), level, stream(), band_pitch=pitch)
        assert torch.equal(out, ref) and bool(torch.isfinite(out).all()) and not torch.equal(out, x)
        assert same(x.cpu().numpy(), xh)


def test_the_classes_shrink_on_a_forced_plan(shim):
    J = shim.sel_joint_tile_j()
    K, n, level = J + 1, 96, 2
    w = ndwt.nd_dwt_1D("db2", n, "batch", K, "precision", "single")
    nb = ndwt.num_bands(1, level)
    rng = np.random.default_rng(73)
    xt = torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)).cuda()      # MATLAB shape [n, K]
    y = w.dec(xt, level)                                          # [n, K, bands]
    flat = y.permute(2, 1, 0).contiguous().cpu().numpy().reshape(-1)   # kernel order: [bands, K, n]
    thr = np.array([0.0, 0.9, 1.4]) * np.sqrt(K)
    w._plan(False, level, xt.device).set_variant(-1, TILE)
    for mode in ("soft", "hard"):
        with ndwt.kernel_trace() as recs:
            got = w.shrink(y, thr, mode, joint=True)
        fams = [r.family for r in recs]
        assert "JointTile" in fams and "JointShrink" not in fams, fams
        gflat = got.permute(2, 1, 0).contiguous().cpu().numpy().reshape(-1)
        assert same(gflat, reference_shrink("f32", flat, K * n, K, n, nb, thr, mode == "hard", fused=True))
        assert not same(gflat, flat)
