"""The device memory a plan owns and grows on demand -- the staging of the host-pointer forms, the coefficient scratch and the level-1
approximation of ndwt_denoise, the temporaries of the per-axis passes and of the 4-D t split, the z-extended slab of the split-halo
analysis: ONE plan (max_level = 3) takes a small request, then a larger one, then the small one again, and after every call its
result equals, bit for bit, what a fresh plan gives for the same call (a buffer that grew, or one larger than the call needs, changes
nothing).  The dec calls are also compared with the CPU oracle at the tolerance of tests/test_gpu_parity.py.

Shapes are the smallest that take the paths: [16, 12, 10] with db2 (3-D, fused), [8, 8, 6, 6] (4-D) and the z-slab [16, 12, 8 of 24, 4]
of tests/test_gpu_zshard.py's dilated case.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ndwt_oracle as orc

pytestmark = pytest.mark.gpu

api = importlib.import_module("non-decimated_wavelets_amd.api")
L = importlib.import_module("non-decimated_wavelets_amd._lib")
TOL = {"double": 1e-12, "single": 2e-6}                       # tests/test_gpu_parity.py


def _relerr(got, want):
    return float(np.abs(np.asarray(got) - want).max() / max(np.abs(want).max(), 1e-300))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dec_host(plan, xk, level):
    y = np.empty((orc.num_bands(xk.ndim, level),) + xk.shape, dtype=xk.dtype)
    L.check(L.lib().ndwt_dec_host(plan._h, _ptr(xk), _ptr(y), level))
    return y


def _rec_host(plan, c, level):
    r = np.empty(c.shape[1:], dtype=c.dtype)
    L.check(L.lib().ndwt_rec_host(plan._h, _ptr(c), _ptr(r), level))
    return r


def test_host_pointer_staging_grows_and_is_released():
    dims, wn = [16, 12, 10], ["db2"] * 3
    rng = np.random.default_rng(11)
    x = rng.standard_normal(dims)
    xk = np.ascontiguousarray(x.T).astype(np.float32)
    coefs = {lev: rng.standard_normal((orc.num_bands(3, lev),) + xk.shape).astype(np.float32) for lev in (1, 3)}
    make = lambda: api.Plan(dims, wn, torch.float32, False, True, max_level=3)
    fresh = {lev: (_dec_host(make(), xk, lev), _rec_host(make(), coefs[lev], lev)) for lev in (1, 3)}
    for lev in (1, 3):
        assert _relerr(fresh[lev][0].T, orc.spatial_dec(x, wn, lev, 1)) <= TOL["single"]
    plan = make()
    for step, lev in enumerate((1, 3, 1)):
        y = _dec_host(plan, xk, lev)
        assert np.array_equal(y, fresh[lev][0]), (step, lev)
        assert _relerr(y.T, orc.spatial_dec(x, wn, lev, 1)) <= TOL["single"]
        if step == 1:
            plan.release_staging()                            # between the level-3 dec and rec: the rec allocates both buffers anew
        assert np.array_equal(_rec_host(plan, coefs[lev], lev), fresh[lev][1]), (step, lev)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_denoise_scratch_grows(precision):
    """double: the fused level-1 kernel does not apply, the coefficient scratch holds every band; single: level 1 in one launch, its
    approximation in a scratch of its own and the coefficient scratch for the levels above it"""
    dims, wn, thr = [16, 12, 10], ["db2"] * 3, 0.3
    tdt = torch.float64 if precision == "double" else torch.float32
    torch.manual_seed(12)
    xk = torch.randn(*reversed(dims), dtype=tdt, device="cuda:0")
    make = lambda: api.Plan(dims, wn, tdt, False, True, max_level=3)

    def denoise(plan, lev):
        out = torch.full_like(xk, float("nan"))
        plan.denoise(xk.data_ptr(), out.data_ptr(), lev, thr)
        torch.cuda.synchronize()
        return out

    fresh = {lev: denoise(make(), lev) for lev in (1, 3)}
    for lev in (1, 3):                                        # (it did something: not the input, not NaN)
        assert torch.isfinite(fresh[lev]).all() and not torch.equal(fresh[lev], xk)
    plan = make()
    for step, lev in enumerate((1, 3, 1)):
        assert torch.equal(denoise(plan, lev), fresh[lev]), (step, lev)


def test_temporaries_serve_the_per_axis_passes_and_the_t_split():
    dims, wn, level = [8, 8, 6, 6], ["db2"] * 4, 2
    rng = np.random.default_rng(13)
    x = rng.standard_normal(dims)
    xk = torch.from_numpy(np.ascontiguousarray(x.T).astype(np.float32)).to("cuda:0")
    want = orc.spatial_dec(x, wn, level, 1)
    make = lambda: api.Plan(dims, wn, torch.float32, False, True, max_level=3)

    def dec(plan, generic):
        plan.set_path(generic)
        y = torch.full((orc.num_bands(4, level),) + tuple(xk.shape), float("nan"), dtype=xk.dtype, device=xk.device)
        plan.dec(xk.data_ptr(), y.data_ptr(), level)
        torch.cuda.synchronize()
        return y

    fresh = {generic: dec(make(), generic) for generic in (True, False)}
    plan = make()
    for step, generic in enumerate((True, False, True)):
        y = dec(plan, generic)
        assert torch.equal(y, fresh[generic]), (step, generic)
        assert _relerr(y.cpu().numpy().T, want) <= TOL["single"]


def test_z_extended_slab_grows_with_the_halo():
    """a 4-D slab plan sharded on z, a-trous dilation: the split-halo analysis at tap stride 1, 2, 1 (the halo, and with it the slab the
    plan assembles, doubles and shrinks again).  Tap stride 1 is level 1 of the whole volume: also against the oracle"""
    dims, wn, nz, z0, n = [16, 12, 24, 4], ["db2"] * 4, 24, 0, 8
    local = dims[:2] + [n] + dims[3:]
    rng = np.random.default_rng(14)
    x = rng.standard_normal(dims)
    xk = torch.from_numpy(np.ascontiguousarray(x.T).astype(np.float32)).to("cuda:0")          # (nt, nz, ny, nx)
    want = orc.spatial_dec(x, wn, 1, 1, "atrous")[:, :, z0:z0 + n]                             # (nx, ny, n, nt, 16)
    make = lambda: api.Plan(local, wn, torch.float32, False, True, "atrous", max_level=3, global_outer=nz, shard_axis=2)

    def planes(lo, hi):
        return xk[:, [z % nz for z in range(lo, hi)]].contiguous()

    def split(plan, stride):
        ab, aa, _, _ = plan.slab_halo(stride)
        mid, before, after = planes(z0, z0 + n), planes(z0 - ab, z0), planes(z0 + n, z0 + n + aa)
        out = torch.full((16,) + tuple(mid.shape), float("nan"), dtype=xk.dtype, device=xk.device)
        plan.analysis_level_slab_split(mid.data_ptr(), before.data_ptr(), after.data_ptr(), [out[b].data_ptr() for b in range(16)], stride)
        torch.cuda.synchronize()
        return out

    fresh = {stride: split(make(), stride) for stride in (1, 2)}
    assert torch.isfinite(fresh[2]).all()
    plan = make()
    for step, stride in enumerate((1, 2, 1)):
        out = split(plan, stride)
        assert torch.equal(out, fresh[stride]), (step, stride)
        if stride == 1:
            assert _relerr(out.cpu().numpy().T, want) <= TOL["single"]
