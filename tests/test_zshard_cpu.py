"""z-sharded 4-D volumes on CPU (gloo): ShardedNdDwt(shard_axis=2) keeps t whole on every rank and exchanges the z halo of
every frame, with an oracle-backed z-slab engine standing in for the GPU one.

Gate: the sharded dec / rec equal the single-process oracle (fp64, 1e-12) -- uneven partitions of nz, slabs thinner than the z
filter (multi-hop halos), reference and a-trous dilation, mixed per-axis wavelets with the z filter the longest and not, both
synthesis schemes.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OracleZSlabEngine:
    """Slab compute of a z-slab (kernel order (nt, nz, ny, nx)) from the periodic oracle: the haloed slab is transformed as if
    periodic -- t is whole, so its wrap is the true one -- and cropped on z, where the filter support never reaches the wrap."""

    supports_scatter = True

    def __init__(self, wname, l2):
        import ndwt_oracle as orc
        self.orc = orc
        self.filt = [orc.wave_filters(w) for w in wname]
        self.l2 = l2
        self.L = len(self.filt[2][0])                       # the z filter sets the halo

    def halo(self, stride):
        L = self.L
        return ((L // 2 - 1) * stride, (L // 2) * stride, (L // 2) * stride, (L // 2 - 1) * stride)

    @staticmethod
    def _to_mat(t):
        return np.transpose(t.numpy())

    @staticmethod
    def _from_mat(a):
        return torch.from_numpy(np.ascontiguousarray(np.transpose(a)))

    def analysis_split(self, in_local, hb, ha, outs, stride):
        ab, _, _, _ = self.halo(stride)
        n = in_local.shape[1]
        y = self.orc.spatial_level_dec(self._to_mat(torch.cat([hb, in_local, ha], 1)), self.filt, self.l2, stride)
        for b, o in enumerate(outs):
            o.copy_(self._from_mat(y[..., b])[:, ab:ab + n])

    def synthesis(self, ins_with_halo, out, stride):
        _, _, sb, _ = self.halo(stride)
        c = np.stack([self._to_mat(t) for t in ins_with_halo], axis=-1)
        r = self._from_mat(self.orc.spatial_level_rec(c, self.filt, self.l2, stride))
        out.copy_(r[:, sb:sb + out.shape[1]])

    def synthesis_ext(self, ins_local, out_ext, stride):
        _, _, sb, sa = self.halo(stride)
        pad = (self.L - 1) * stride
        padded = [torch.nn.functional.pad(t, [0, 0, 0, 0, pad, pad]) for t in ins_local]
        c = np.stack([self._to_mat(t) for t in padded], axis=-1)
        r = self._from_mat(self.orc.spatial_level_rec(c, self.filt, self.l2, stride))
        n = ins_local[0].shape[1]
        out_ext.copy_(r[:, pad - sa:pad + n + sb])


def _worker(rank, world, port, sizes, wname, level, l2, dilation, schemes, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import importlib
    import ndwt_oracle as orc
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sh = importlib.import_module("non-decimated_wavelets_amd.sharded")
        rng = np.random.default_rng(11)
        x = rng.standard_normal(sizes)                                  # MATLAB shape [nx, ny, nz, nt], same on every rank
        xk = torch.from_numpy(np.ascontiguousarray(np.transpose(x)))    # (nt, nz, ny, nx)
        want = np.ascontiguousarray(np.transpose(orc.spatial_dec(x, wname, level, l2, dilation)))   # (bands, nt, nz, ny, nx)
        c = rng.standard_normal(list(sizes) + [orc.num_bands(4, level)])
        ck = torch.from_numpy(np.ascontiguousarray(np.transpose(c)))
        want2 = np.ascontiguousarray(np.transpose(orc.spatial_rec(c, wname, l2, dilation)))
        errs = []
        for scheme in schemes:
            eng = sh.ShardedNdDwt(wname, sizes, pres_l2_norm=l2, precision="double", dilation=dilation,
                                  engine=OracleZSlabEngine(wname, l2), synthesis_scheme=scheme, shard_axis=2)
            assert eng.ax == 1 and not eng.overlap and eng.scheme == scheme
            z0, z1 = eng.z0, eng.z1
            y_loc = eng.dec(xk[:, z0:z1].contiguous(), level)
            assert tuple(y_loc.shape) == (want.shape[0], sizes[3], z1 - z0, sizes[1], sizes[0])
            e_dec = float(np.abs(y_loc.numpy() - want[:, :, z0:z1]).max())
            r_loc = eng.rec(y_loc)
            e_rec = float(np.abs(r_loc.numpy() - xk[:, z0:z1].numpy()).max())
            r2 = eng.rec(ck[:, :, z0:z1].contiguous())                   # coefficients outside the range of dec
            e_rec2 = float(np.abs(r2.numpy() - want2[:, z0:z1]).max())
            errs.append((scheme, e_dec, e_rec, e_rec2))
        # tune(): no run-of-planes pieces on z-slabs -- only the one-piece schedule exists, and it is what every rank keeps
        rec = eng.tune(xk[:, eng.z0:eng.z1].contiguous(), level, steps=1)
        assert rec["schedule"] == "one_piece" and rec["ms_one_piece"] > 0 and "ms_overlap" not in rec, rec
        q.put((rank, errs))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


CASES = [
    # world, sizes [nx, ny, nz, nt],   wavelets [x, y, z, t],        level, l2, dilation
    (2, [6, 5, 11, 4], ["db1", "db2", "db3", "db2"], 2, 1, "reference"),     # z filter the longest, uneven partition
    (3, [5, 6, 8, 3], ["db2", "db1", "db3", "db1"], 2, 0, "reference"),      # 2-3 planes per rank < 3 halo planes after: multi-hop
    (3, [6, 7, 7, 5], ["db3", "db1", "db2", "db2"], 2, 1, "reference"),      # z filter NOT the longest
    (2, [6, 4, 9, 4], ["db1", "db1", "db2", "db1"], 2, 1, "atrous"),         # dilated z taps: 2 + 4 halo planes at level 2 over 4-5-plane slabs
    (3, [4, 4, 8, 6], ["db2", "db2", "db4", "db3"], 1, 0, "reference"),      # 2-3 planes per rank against 8 taps: multi-hop both ways
]


@pytest.mark.parametrize("world,sizes,wname,level,l2,dilation", CASES)
def test_zsharded_equals_single_process(world, sizes, wname, level, l2, dilation):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    schemes = ("gather", "scatter")
    procs = [ctx.Process(target=_worker, args=(r, world, port, sizes, wname, level, l2, dilation, schemes, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, errs in res:
        for scheme, e_dec, e_rec, e_rec2 in errs:
            assert e_dec < 1e-12 and e_rec < 1e-12 and e_rec2 < 1e-12, (rank, scheme, e_dec, e_rec, e_rec2)


def test_shard_axis_is_checked():
    """only the outermost axis, or z of a 4-D volume"""
    sys.path.insert(0, ROOT)
    import importlib
    sh = importlib.import_module("non-decimated_wavelets_amd.sharded")
    for sizes, axis in (([8, 8, 8], 1), ([8, 8, 8, 8], 1), ([8, 8, 8, 8], 0), ([8, 8, 8, 8], 4)):
        with pytest.raises(ValueError, match="shard_axis"):
            sh.ShardedNdDwt("db2", sizes, engine=OracleZSlabEngine(["db2"] * len(sizes), 0), shard_axis=axis)
    eng = sh.ShardedNdDwt("db2", [8, 6, 10, 3], engine=OracleZSlabEngine(["db2"] * 4, 0), shard_axis=2)
    assert (eng.z0, eng.z1, eng.n_outer, eng.ax) == (0, 10, 10, 1)
    eng = sh.ShardedNdDwt("db2", [8, 6, 10, 3], engine=OracleZSlabEngine(["db2"] * 4, 0), shard_axis=3)
    assert (eng.n_outer, eng.ax) == (3, 0)


def test_reps_layout():
    """the view geometry the strided segment kernel is fed with: nrep runs at a constant distance"""
    sys.path.insert(0, ROOT)
    import importlib
    sh = importlib.import_module("non-decimated_wavelets_amd.sharded")
    t = torch.zeros(4, 9, 5, 6)
    assert sh._reps(t) == (1, 4 * 9 * 5 * 6, 4 * 9 * 5 * 6)
    assert sh._reps(t[:, 2:5]) == (4, 3 * 30, 9 * 30)
    assert sh._reps(t[:, :1]) == (4, 30, 9 * 30)
    f = torch.zeros(16, 4, 9, 5, 6)
    assert sh._reps(f[:, :, 2:5]) == (64, 3 * 30, 9 * 30)
    assert sh._reps(f[:3, :, 2:5]) == (12, 3 * 30, 9 * 30)
    assert sh._reps(f[:, 1:3, 2:5]) is None                        # frames 1..2 of every band: not one constant distance
