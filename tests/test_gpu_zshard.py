"""z-sharded 4-D volumes on the GPU: the strided segment kernel, z-slab plans (ndwt_plan_create_slab_axis), the single-process
multi-device plan on z (ndwt_mplan_create_axis) and the per-process driver ShardedNdDwt(shard_axis=2), against the single-device
transform and the CPU oracle.

Tolerances: where the slab runs the kernels of the single-device transform (fused real plans, gather synthesis) the results are
equal bit for bit; elsewhere fp32 <= 4e-6 (dec) / 1e-5 (rec) and fp64 <= 1e-12 (dec) / 4e-12 (rec), relative to max |c|.
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import ndwt_oracle as orc

pytestmark = pytest.mark.gpu

api = importlib.import_module("non-decimated_wavelets_amd.api")
L = importlib.import_module("non-decimated_wavelets_amd._lib")
TOL = {"single": (4e-6, 1e-5), "double": (1e-12, 4e-12)}


def _relerr(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ------------------------------------------------------------------------------------------------------------ strided segments
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_segments_strided_against_torch(dtype):
    """copy and add of up to 8 runs x nrep repetitions in one launch: odd counts, pointers off 16-byte alignment, nrep 1 and many"""
    plan = api.Plan([8, 8, 8], ["db2"] * 3, dtype)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(5)
    for nrep in (1, 7, 40):
        for add in (False, True):
            for off in (0, 1, 3):                                 # element offsets: 16-byte aligned or not
                counts = [1, 5, 64, 257, 1000 + off, 3]
                dstr = [c + 11 + off for c in counts]          # (>= count: the repetitions of a run do not overlap)
                sstr = [c + (i % 3) * 4 for i, c in enumerate(counts)]
                dsts = [torch.randn(off + ds * nrep + 8, generator=g, dtype=dtype).to(dev) for ds in dstr]
                srcs = [torch.randn(off + max(ss, c) * nrep + 8, generator=g, dtype=dtype).to(dev) for ss, c in zip(sstr, counts)]
                want = [d.clone() for d in dsts]
                for w, s, c, ds, ss in zip(want, srcs, counts, dstr, sstr):
                    for r in range(nrep):
                        dv, sv = w[off + r * ds:off + r * ds + c], s[off + r * ss:off + r * ss + c]
                        dv.copy_(dv + sv if add else sv)
                plan.slab_segments_strided(add, [d.data_ptr() + off * d.element_size() for d in dsts],
                                           [s.data_ptr() + off * s.element_size() for s in srcs], counts, nrep, dstr, sstr)
                torch.cuda.synchronize()
                for d, w in zip(dsts, want):
                    assert torch.equal(d, w), (nrep, add, off)        # (elements between the runs untouched)
    with pytest.raises(L.NdwtError, match="destination stride"):
        plan.slab_segments_strided(False, [dsts[0].data_ptr()], [srcs[0].data_ptr()], [10], 2, [5], [10])


# ------------------------------------------------------------------------------------------------------------ z-slab plans
def test_slab_axis_arguments():
    wn = ["db4"] * 4
    for ndim, axis in ((4, 0), (4, 1), (4, 4), (3, 1), (3, 0), (2, 0)):
        with pytest.raises(L.NdwtError) as e:
            api.Plan([32, 32, 16, 8][:ndim], wn[:ndim], torch.float32, global_outer=64, shard_axis=axis)
        assert e.value.code == 7 and "shard_axis" in e.value.message
    # the reference's length check on the WHOLE sharded axis, with its message for the third dimension
    with pytest.raises(L.NdwtError, match="Third Dimension of Data is shorter than the wavelet filter being used"):
        api.Plan([32, 32, 4, 8], wn, torch.float32, global_outer=6, shard_axis=2)
    # a slab thinner than the z filter is accepted; the halo is the z filter's, not t's
    p = api.Plan([32, 32, 3, 8], ["db4", "db4", "db4", "db1"], torch.float32, global_outer=24, shard_axis=2)
    assert p.slab_halo(1) == (3, 4, 4, 3) and p.slab_halo(2) == (6, 8, 8, 6)
    p = api.Plan([32, 32, 8, 3], ["db4", "db4", "db4", "db1"], torch.float32, global_outer=24, shard_axis=3)   # = the t-slab plan
    assert p.slab_halo(1) == (0, 1, 1, 0)
    p = api.Plan([32, 32, 8], ["db2"] * 3, torch.float32, global_outer=24, shard_axis=2)                     # 3-D: its outer axis
    assert p.slab_halo(1) == (1, 2, 2, 1)


# ------------------------------------------------------------------------------------------------------------ multi-device plan
def _single_host(dims, wn, tdt, cplx, dilation, level, xk, c):
    p1 = api.Plan(dims, wn, tdt, cplx, True, dilation, max_level=level)
    y1 = np.empty((orc.num_bands(4, level),) + xk.shape, dtype=xk.dtype)
    L.check(L.lib().ndwt_dec_host(p1._h, xk.ctypes.data_as(ctypes.c_void_p), y1.ctypes.data_as(ctypes.c_void_p), level))
    r1 = np.empty(xk.shape, dtype=xk.dtype)
    L.check(L.lib().ndwt_rec_host(p1._h, c.ctypes.data_as(ctypes.c_void_p), r1.ctypes.data_as(ctypes.c_void_p), level))
    return y1, r1


@pytest.mark.parametrize("dims,wn,level,precision,cplx,dilation,nslab,exact", [
    ([24, 20, 24, 8], ["db4"] * 4, 2, "single", False, "reference", 3, True),                 # fused, z filter the longest
    ([20, 16, 12, 8], ["db4", "db4", "db4", "db2"], 2, "single", False, "reference", 4, True),   # 3 planes per slab under 8 taps
    ([16, 12, 18, 5], ["db2", "db3", "db4", "db2"], 2, "double", False, "reference", 2, True),   # fp64, mixed, z the longest
    ([16, 12, 14, 5], ["db4", "db2", "db3", "db2"], 2, "double", False, "reference", 3, False),  # fp64, z NOT the longest: per-axis
    ([16, 12, 16, 6], ["db3"] * 4, 2, "single", True, "reference", 2, False),                # interleaved complex
    ([16, 12, 24, 4], ["db2"] * 4, 3, "single", False, "atrous", 3, False),                  # dilated: 4 + 8 halo planes at level 3
])
def test_mplan_z_slabs(dims, wn, level, precision, cplx, dilation, nslab, exact):
    rng = np.random.default_rng(31)
    x = rng.standard_normal(dims) + (1j * rng.standard_normal(dims) if cplx else 0)
    rdt = np.float32 if precision == "single" else np.float64
    cdt = (np.complex64 if precision == "single" else np.complex128) if cplx else rdt
    tdt = torch.float32 if precision == "single" else torch.float64
    xk = np.ascontiguousarray(x.T).astype(cdt)
    mp = api.MultiPlan(dims, wn, tdt, [0] * nslab, cplx, True, dilation, max_level=level, shard_axis=2)
    sl = mp.slabs()
    assert len(sl) == nslab and sl[0][1] == 0 and sum(s[2] for s in sl) == dims[2]
    desc = mp.describe()
    assert "of axis 2 (z" in desc and "exchange, then compute" in desc
    yk = mp.dec(xk, level)
    c = (rng.standard_normal(yk.shape) + (1j * rng.standard_normal(yk.shape) if cplx else 0)).astype(cdt)
    y1, r1 = _single_host(dims, wn, tdt, cplx, dilation, level, xk, c)
    td, tr = TOL[precision]
    assert np.array_equal(yk, y1) if exact else _relerr(yk, y1) <= td
    assert _relerr(yk.T, orc.spatial_dec(x, wn, level, 1, dilation)) <= td
    want_r = orc.spatial_rec(np.transpose(c), wn, 1, dilation)
    for scheme in ("gather", "scatter"):
        mp.set_exchange(scheme)
        r = mp.rec(c)
        scatter = scheme == "scatter" and "scatter-add" in mp.describe()
        assert np.array_equal(r, r1) if exact and not scatter else _relerr(r, r1) <= tr, scheme
        assert _relerr(r.T, want_r) <= tr, scheme
        assert np.array_equal(r, mp.rec(c))                                 # a fixed order of summation
        assert _relerr(mp.rec(yk), xk) <= 20 * td
    lens = [len(orc.wave_filters(w)[0]) for w in wn]
    assert ("scatter-add" in mp.describe()) == (lens[2] == max(lens[:3]) and dilation == "reference")   # fused plans, z the longest
    # threads on / off: the same work on the same streams
    mp.set_threads(False)
    assert np.array_equal(mp.dec(xk, level), yk) and np.array_equal(mp.rec(c), r)
    mp.set_threads(True)
    # device-resident form: (nt, nz_i, ny, nx) per slab in, (bands, nt, nz_i, ny, nx) out, read and written in place
    dev = torch.device("cuda", 0)
    xs = [torch.from_numpy(np.ascontiguousarray(xk[:, z0:z0 + n])).to(dev) for _, z0, n in sl]
    ys = mp.dec_device(xs, level)
    assert all(np.array_equal(yd.cpu().numpy(), yk[:, :, z0:z0 + n]) for yd, (_, z0, n) in zip(ys, sl))
    cs = [torch.from_numpy(np.ascontiguousarray(c[:, :, z0:z0 + n])).to(dev) for _, z0, n in sl]
    rs = mp.rec_device(cs)
    assert all(np.array_equal(rd.cpu().numpy(), r[:, z0:z0 + n]) for rd, (_, z0, n) in zip(rs, sl))


def test_mplan_z_slabs_cfg5_proportions():
    """cfg5 (256^3 x 32, db4, 8 ranks) at half the edge: 128^3 x 32, 3 levels, 8 z-slabs of 16 planes -- device forms against the
    single-device transform (gather: bit for bit; scatter: to rounding)"""
    dims, wn, level = [128, 128, 128, 32], ["db4"] * 4, 3
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    xk = torch.randn(*reversed(dims), device=dev)
    p1 = api.Plan(dims, wn, torch.float32, False, True, max_level=level)
    nbt = orc.num_bands(4, level)
    y1 = torch.empty((nbt,) + tuple(xk.shape), device=dev)
    p1.dec(xk.data_ptr(), y1.data_ptr(), level)
    mp = api.MultiPlan(dims, wn, torch.float32, [0] * 8, False, True, max_level=level, shard_axis=2)
    sl = mp.slabs()
    assert [s[2] for s in sl] == [16] * 8
    ys = mp.dec_device([xk[:, z0:z0 + n].contiguous() for _, z0, n in sl], level)
    for yd, (_, z0, n) in zip(ys, sl):
        assert torch.equal(yd, y1[:, :, z0:z0 + n])
    del ys
    torch.manual_seed(4)
    c = torch.randn_like(y1)
    del y1
    r1 = torch.empty_like(xk)
    p1.rec(c.data_ptr(), r1.data_ptr(), level)
    torch.cuda.synchronize()
    cs = [c[:, :, z0:z0 + n].contiguous() for _, z0, n in sl]
    del c
    scale = float(r1.abs().max())
    for scheme in ("gather", "scatter"):
        mp.set_exchange(scheme)
        rs = mp.rec_device(cs)
        for rd, (_, z0, n) in zip(rs, sl):
            if scheme == "gather":
                assert torch.equal(rd, r1[:, z0:z0 + n])
            else:
                assert float((rd - r1[:, z0:z0 + n]).abs().max()) <= 1e-5 * scale


# ------------------------------------------------------------------------------------------------------------ per-process driver
def _single_dev(dims, wn, precision, level, xk, c):
    """single-device dec of xk and rec of c (kernel-order tensors on the GPU)"""
    p1 = api.Plan(dims, wn, xk.dtype, False, True, max_level=level, device=xk.device.index)
    y = torch.empty((orc.num_bands(4, level),) + tuple(xk.shape), dtype=xk.dtype, device=xk.device)
    p1.dec(xk.data_ptr(), y.data_ptr(), level)
    r = torch.empty_like(xk)
    p1.rec(c.data_ptr(), r.data_ptr(), level)
    torch.cuda.synchronize()
    return y, r


ZCASES = (([24, 20, 16, 8], "db4", 2, "single"), ([16, 12, 10, 4], ["db2", "db3", "db4", "db1"], 2, "double"))


def _check_driver(sh, dev, errs, **kw):
    for sizes, wn, level, precision in ZCASES:
        wl = [wn] * 4 if isinstance(wn, str) else wn
        torch.manual_seed(21)
        dt = torch.float32 if precision == "single" else torch.float64
        xk = torch.randn(*reversed(sizes), device=dev, dtype=dt)
        c = torch.randn((orc.num_bands(4, level),) + tuple(xk.shape), device=dev, dtype=dt)
        y1, r1 = _single_dev(sizes, wl, precision, level, xk, c)
        td, tr = TOL[precision]
        for scheme in ("gather", "scatter"):
            eng = sh.ShardedNdDwt(wl, sizes, pres_l2_norm=True, precision=precision, device=dev, synthesis_scheme=scheme,
                                  shard_axis=2, **kw)
            z0, z1 = eng.z0, eng.z1
            for _ in range(2):                                             # later calls reuse the driver's scratch
                y = eng.dec(xk[:, z0:z1].contiguous(), level)
                e_dec = float((y - y1[:, :, z0:z1]).abs().max() / y1.abs().max())
                r = eng.rec(c[:, :, z0:z1].contiguous())
                e_rec = float((r - r1[:, z0:z1]).abs().max() / r1.abs().max())
                errs.append((precision, scheme, e_dec, e_rec, td, tr))
        rec = eng.tune(xk[:, z0:z1].contiguous(), level, steps=1)
        errs.append(("tune", rec["schedule"], 0.0, float(any(k.startswith("ms_") and "overlap" in k for k in rec)), 1.0, 0.5))


def _assert_errs(errs):
    assert errs
    for e in errs:
        assert e[2] <= e[4] and e[3] <= e[5], e


def test_sharded_driver_z_world1():
    """world size 1 on cuda:0: the periodic self-halo of every frame through the strided segment kernel"""
    sh = importlib.import_module("non-decimated_wavelets_amd.sharded")
    dev = torch.device("cuda", 0)
    errs = []
    _check_driver(sh, dev, errs)
    _assert_errs(errs)
    eng = sh.ShardedNdDwt("db4", [24, 20, 16, 8], precision="single", device=dev, shard_axis=2)
    assert eng.scheme == "scatter" and eng.engine.supports_scatter and not eng.can_overlap


def _run_ranks(worker, world):
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sh = importlib.import_module("non-decimated_wavelets_amd.sharded")
        errs = []
        _check_driver(sh, torch.device("cuda", 0), errs)
        q.put((rank, errs, None))
    except Exception as exc:
        q.put((rank, [], f"{type(exc).__name__}: {exc}"[:400]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_driver_z_ranks_share_one_gpu_over_gloo(world):
    for rank, errs, info in _run_ranks(_gloo_worker, world):
        assert info is None, info
        _assert_errs(errs)


def _nccl_self_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    try:
        sh = importlib.import_module("non-decimated_wavelets_amd.sharded")
        errs = []
        for transport in ("torch", "rccl"):
            _check_driver(sh, dev, errs, transport=transport, _self_p2p=True)
        eng = sh.ShardedNdDwt("db4", [24, 20, 16, 8], precision="single", device=dev, shard_axis=2, _self_p2p=True)
        rec = eng.tune(torch.randn(8, 16, 20, 24, device=dev), 2, steps=2)
        info = None if set(k for k in rec if k.startswith("ms_")) == {"ms_one_piece", "ms_rccl_one_piece"} else f"tune: {rec}"
        torch.cuda.synchronize(dev)
        q.put((rank, errs, info))
    except Exception as exc:
        q.put((rank, [], f"{type(exc).__name__}: {exc}"[:400]))
    finally:
        dist.destroy_process_group()


def test_sharded_driver_z_rccl_self_p2p():
    """a 1-rank `nccl` group: the frames' halo runs and partial sums packed by the strided kernel into contiguous send buffers and
    sent to self through RCCL, both transports"""
    (rank, errs, info), = _run_ranks(_nccl_self_worker, 1)
    assert info is None, info
    _assert_errs(errs)
