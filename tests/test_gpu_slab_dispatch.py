"""Every kernel the slab entry points can run, pinned and checked with a halo on the device.

tests/test_gpu_dispatch.py pins the dispatcher through ndwt_dec / ndwt_rec: every launch there is periodic on the outer axis
(Fused3Args::z_wrap = 1, Fused2Args::y_wrap = 1, the per-axis kernels with wrap = 1).  The slab entry points of include/ndwt.h reach the
same kernel families through the other values of that run-time switch:
    0  the input carries its halo planes            ndwt_analysis_level_slab, ndwt_synthesis_level_slab, ndwt_analysis_level_slab_runs
    2  the halo planes lie in buffers of their own  ndwt_analysis_level_slab_split, ndwt_analysis_level_slab_part
    3  zero-extended synthesis (zlo / zhi / zbs)    ndwt_synthesis_level_slab_ext, ndwt_synthesis_level_slab_part / _runs
Each row cuts slabs out of ONE periodic volume, names the kernels the slab calls must launch (derived from csrc/ndwt_select.h:
level_route with the SlabMode, then fused3_select / fused2_select with the local n1, n2, nbatch) and compares every call with one level of
oracle/ndwt_spatial.c on the whole volume, in double, on the input rounded to the device precision.

Memory discipline of every call: the inputs lie between planes of NaN (a kernel that reads a plane too far returns NaN), every output
lies inside a buffer pre-filled with a non-zero pattern whose guard planes must come back untouched, and the inputs must be bit-identical
afterwards.  (A 4-D volume sharded on z keeps its frames back to back, as include/ndwt.h lays them out: there the NaN planes lie before
the first and after the last frame.)

Slab cuts of a row with the longest filter L on the sharded axis of N = 4 L planes (`std_cuts`):
    thick   planes [3, 2 L + 4): 2 L + 1 > 2 (L - 1) planes, marched in forced chunks of 4 (2 L + 1 is odd: the chunk never divides it)
    thin    3 planes (2 for L = 4) from N - 1 on, across the wrap of the volume: thinner than L - 1, a plan made with global_outer
The zero-extended synthesis is compared with the periodic oracle on the coefficients zeroed outside the slab: its support, n + L - 1
planes, must not meet itself round the wrap -- N >= n + 2 (L - 1), i.e. 4 L >= 4 L - 1 for the thick cut (asserted per call).
"""
import itertools
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
import ndwt_spatial as orc_c
from helpers import check_trace, matches, spec
from test_gpu_dispatch import TOL, _dtypes

pytestmark = pytest.mark.gpu

FILL = 1234.5                                                  # the pattern around every output: not zero (a stray zero store must show)


def std_cuts(L, N):
    assert N >= (2 * L + 1) + 2 * (L - 1)
    return [(3, 2 * L + 4, 4), (N - 1, N - 1 + (3 if L > 4 else 2), 2 if L > 4 else 0)]


def S(rid, dims, wn, ana, syn, prec="single", cplx=False, axis=None, cuts=None, fwd=-1, inv=-1, stride=1, fast=None, ext=None, whole=None):
    """dims: the whole volume; axis: the sharded axis (None: the outermost); cuts: (z0, z1, forced z-chunk) in planes of the whole volume;
    ana / syn: the kernels of the analysis / synthesis calls, "~" in front of those that run periodic (no halo on their axis);
    fast: what ndwt_plan_slab_fast must answer; ext: the zero-extended synthesis is offered; whole: describe() of the whole-array plan"""
    d = len(dims)
    axis = d - 1 if axis is None else axis
    wl = [wn] * d if isinstance(wn, str) else list(wn)
    L = 2 * int(wl[axis][2:])
    if fast is None:
        fast = d == 3 and stride == 1
    if ext is None:
        ext = fast
    return pytest.param(dict(id=rid, dims=dims, wl=wl, prec=prec, cplx=cplx, axis=axis, cuts=cuts or std_cuts(L, dims[axis]), fwd=fwd, inv=inv,
                             stride=stride, fast=fast, ext=ext, ana=list(ana), syn=list(syn), whole=whole), id=rid)


# ---- the rows.  n1, n2 are those of the matching row of tests/test_gpu_dispatch.py: the picks of fused3_select / fused2_select depend on
# n1, n2 and nbatch only (nbatch = 1 here; 2 in the _runs launches, which moves no row across the tall-tile threshold), so a slab of the
# same n1 x n2 takes the kernel of the whole array -- unless level_route sends the slab elsewhere, which the rows at the end pin.
ROWS = [
    # 3-D float real.  6 / 8 taps: tall 64x32 tile once ceil(n1/64) * ceil(n2/32) * nbatch >= 32
    S("db2-small-tile", [64, 40, 16], "db2", ["Fwd3 L=4 TY=16 NT=256 VEC4=true"], ["Inv3Y L=4 XSC=false VEC4=true DEPTH=1"]),   # 1 * 2 = 2
    S("db4-small-tile", [64, 40, 32], "db4", ["Fwd3 L=8 TY=16 NT=256 VEC4=true PIN=false"],
      ["Inv3Y L=8 XSC=false VEC4=true DEPTH=2 UNIYZ=false"]),                                                                   # 1 * 2 = 2
    # 4 * 8 = 32 tiles.  12 local planes in forced chunks of 5 and 3 planes across the wrap; N = 26 >= 12 + 14
    S("db4-tall-tile", [256, 256, 26], "db4", ["Fwd3 L=8 TY=32 NT=1024 VEC4=true PIN=false"], ["Inv3Y L=8 XSC=false VEC4=true DEPTH=2"],
      cuts=[(3, 15, 5), (25, 28, 2)]),
    S("db4-ragged-n1-70", [70, 40, 32], "db4", ["Fwd3 L=8 TY=16 VEC4=false"], ["Inv3Y L=8 XSC=false VEC4=false"]),              # 70 % 4 != 0
    # 10 .. 14 taps, vec4 rows, even padding: pinned taps; synthesis in scatter form from 10 taps
    S("db5-pinned", [64, 40, 40], "db5", ["Fwd3 L=10 PIN=true TY=32"], ["Inv3Y L=10 XSC=true UNIYZ=false DEPTH=2"]),
    S("db6-pinned", [64, 40, 48], "db6", ["Fwd3 L=12 PIN=true TY=32"], ["Inv3Y L=12 XSC=true UNIYZ=true DEPTH=2 ZLDS=6"]),
    S("db7-pinned", [64, 40, 56], "db7", ["Fwd3 L=14 PIN=true TY=32"], ["Inv3Y L=14 XSC=true UNIYZ=true DEPTH=1"]),
    # (10 - 8) / 2 = 1, odd padding of x: no pinned taps (64x32 tile, V = 2), no Inv3Y -> Inv3S on its tall tile (V = 1)
    S("odd-padding-10", [64, 40, 40], ["db4", "db5", "db5"], ["Fwd3 L=10 PIN=false TY=32 NT=1024 VEC4=true"], ["Inv3S L=10 TY=32 NT=1024 VEC4=true"]),
    # (16 - 14) / 2 = 1: Inv3S of 16 taps (512 threads x 2 items); analysis 16 taps: 2 window slots in LDS
    S("odd-padding-16", [64, 40, 64], ["db7", "db7", "db8"], ["Fwd3 L=16 WLDS=2 TY=32"], ["Inv3S L=16 TY=32 NT=512"]),
    S("db8-wlds2", [64, 40, 64], "db8", ["Fwd3 L=16 WLDS=2 TY=32 VEC4=true"], ["Inv3Y L=16 XSC=true UNIYZ=true"]),
    # 18 / 20 taps: fused in each direction (analysis up to 20 taps; synthesis above 16 through Inv3Y), but ndwt_plan_slab_fast asks
    # fused3_eligible for both at once (dir = -1: lmax = 16) -- the split-halo and zero-extended forms are not offered, modes 0 only
    S("db9-wlds0", [64, 48, 72], "db9", ["Fwd3 L=18 WLDS=0 TY=16 NT=512 VEC4=true"], ["Inv3Y L=18 XSC=true TY=24 UNIYZ=true"], fast=False),
    S("db10-wlds4-tx48", [64, 40, 80], "db10", ["Fwd3 L=20 WLDS=4 VEC4=true"], ["Inv3Y L=20 TX=48 TY=28 XSC=true UNIYZ=true"], fast=False),
    S("db10-ragged-gather", [70, 37, 80], "db10", ["Fwd3 L=20 WLDS=6 VEC4=false"], ["Inv3Y L=20 TX=48 XSC=false VEC4=false"], fast=False),
    # A/B variants of the synthesis
    S("db4-inv3-lds", [64, 40, 32], "db4", ["Fwd3 L=8 TY=16"], ["Inv3 L=8 TY=16"], inv=3),
    S("db4-inv3s-lane-shift", [64, 40, 32], "db4", ["Fwd3 L=8 TY=16"], ["Inv3S L=8 TY=32 NT=1024"], inv=4),
    S("db6-gather-12", [64, 40, 48], "db6", ["Fwd3 L=12 PIN=true"], ["Inv3Y L=12 XSC=false UNIYZ=true"], inv=11),
    # 3-D complex64 (EW = 2; n1 = 64 scalars): gather form at 8 taps, scatter form from 10
    S("c64-db4", [32, 24, 32], "db4", ["Fwd3 L=8 EW=2 TY=16"], ["Inv3Y L=8 EW=2 XSC=false"], cplx=True),
    S("c64-db5", [32, 24, 40], "db5", ["Fwd3 L=10 EW=2 NT=512"], ["Inv3Y L=10 EW=2 XSC=true"], cplx=True),
    S("c64-db6", [32, 24, 48], "db6", ["Fwd3 L=12 EW=2"], ["Inv3Y L=12 EW=2 XSC=true TX=48"], cplx=True),
    S("c128-db5", [32, 24, 40], "db5", ["Fwd3 T=double L=10 EW=2 TY=8 NT=512"], ["Inv3S T=double L=10 EW=2 TY=8 NT=512"], prec="double", cplx=True),
    # 3-D fp64 real: 6 / 8 taps one column per thread on 64x16 (V = 1), 10 taps 64x16 / synthesis 64x8, 12 .. 16 taps 64x8 with 512 threads
    S("f64-db3", [64, 40, 24], "db3", ["Fwd3 T=double L=6 TY=16 NT=512"], ["Inv3S T=double L=6 TY=16 NT=512"], prec="double"),
    S("f64-db4", [64, 40, 32], "db4", ["Fwd3 T=double L=8 TY=16 NT=512"], ["Inv3S T=double L=8 TY=16 NT=512"], prec="double"),
    S("f64-db5", [64, 40, 40], "db5", ["Fwd3 T=double L=10 TY=16 NT=512"], ["Inv3S T=double L=10 TY=8 NT=512"], prec="double"),
    S("f64-db6", [64, 40, 48], "db6", ["Fwd3 T=double L=12 TY=8 NT=512"], ["Inv3S T=double L=12 TY=8 NT=512"], prec="double"),
    S("f64-db7", [64, 40, 56], "db7", ["Fwd3 T=double L=14 TY=8 NT=512 WLDS=0"], ["Inv3S T=double L=14 TY=8"], prec="double"),
    S("f64-db8", [64, 40, 64], "db8", ["Fwd3 T=double L=16 WLDS=2"], ["Inv3S T=double L=16 TY=8"], prec="double"),
    # fp64 beyond 16 taps: per-axis passes, z first with its halo (AxisMarch, wrap = 0), y periodic (AxisMarch), x plain (18 taps > AxisX's 12)
    S("f64-db9-per-axis", [64, 40, 72], "db9", ["AxisMarch T=double L=18 SYN=false", "~axis_analysis_kernel T=double"],
      ["AxisMarch T=double L=18 SYN=true", "~axis_synthesis_kernel T=double"], prec="double", fast=False, whole="axis"),
    # the z filter is not the longest: a fused kernel marches Lp - 1 = 7 halo planes, the slab carries 3 -> level_route: per-axis passes
    # although the whole array is fused.  z: AxisMarch L=4 with the halo; y: AxisMarch L=8, x: AxisX (64 >= 8 * 8), both periodic
    S("z-filter-short-per-axis", [64, 40, 16], ["db4", "db4", "db2"], ["AxisMarch L=4 SYN=false", "~AxisMarch L=8 SYN=false", "~AxisX L=8 SYN=false VEC4=true"],
      ["AxisMarch L=4 SYN=true", "~AxisMarch L=8 SYN=true", "~AxisX L=8 SYN=true VEC4=true"], fast=False, whole="fused3d"),
    # a dilated level (tap stride 2) on a slab: no sub-lattice form for slabs -> per-axis.  Halo (L/2 - 1) * 2 = 2 / (L/2) * 2 = 4 planes.
    # z with its halo at stride 2: the plain kernel (the march needs a periodic axis to split into sub-lattices); y periodic: AxisMarch on
    # the 2 interleaved sub-lattices; x: inner = 2 scalars, no march, stride 2, no AxisX -> the plain kernel again
    # thick: 15 > 2 * 6 planes from the odd plane 3; thin: 3 < 6 planes; N = 32 (no zero-extended form at stride 2)
    S("atrous-stride-2", [32, 24, 32], "db2", ["axis_analysis_kernel T=float", "~AxisMarch L=4 SYN=false"],
      ["axis_synthesis_kernel T=float", "~AxisMarch L=4 SYN=true"], stride=2, cuts=[(3, 18, 4), (31, 34, 2)], fast=False),
    # 4-D sharded on t: the t pass takes the halo (AxisMarch, wrap = 0), the fused 3-D level runs periodic per frame.  The zero-extended
    # form (slab_ext4_impl) is the same pair over zero-padded t-bands
    S("4d-t-db2", [24, 20, 12, 16], "db2", ["AxisMarch L=4 SYN=false", "~Fwd3 L=4 EW=1"], ["~Inv3Y L=4 EW=1", "AxisMarch L=4 SYN=true"], fast=False, ext=True),
    # 4-D sharded on z: the t pass periodic over the z-extended frames, the fused level with the halo on z batched over the 8 frames
    # (1 * 1 * 8 = 8 tiles < 32: small tile); the split form assembles the slab first (segments_strided_kernel)
    S("4d-z-db4", [32, 24, 32, 8], "db4", ["~AxisMarch L=8 SYN=false", "Fwd3 L=8 TY=16 NT=256 EW=1"], ["Inv3Y L=8 XSC=false DEPTH=2", "~AxisMarch L=8 SYN=true"],
      axis=2, fast=True),
    S("4d-z-f64-mixed", [32, 24, 32, 8], ["db2", "db3", "db4", "db2"], ["~AxisMarch T=double L=4 SYN=false", "Fwd3 T=double L=8 TY=16 NT=512"],
      ["Inv3S T=double L=8 TY=16 NT=512", "~AxisMarch T=double L=4 SYN=true"], prec="double", axis=2, fast=True),
    # 2-D sharded on y (y_wrap = 0).  Inv2P: vec4 rows, <= 12 taps, local n2 >= 64 and tiles * ceil(n2 / 70) <= 1280; else Inv2S
    # 64 local rows in forced chunks of 9, and 70 rows across the wrap (N = 96 >= 70 + 14): 2 tiles * 1 chunk
    S("2d-db4-inv2p", [256, 96], "db4", ["Fwd2S L=8 VEC4=true"], ["Inv2P L=8 PD=4 PK=true"], cuts=[(5, 69, 9), (40, 110, 0)]),
    S("2d-db4-inv2s", [256, 32], "db4", ["Fwd2S L=8 VEC4=true"], ["Inv2S L=8 VEC4=true"]),                                      # 17 and 3 local rows < 64
    S("2d-db7", [260, 56], "db7", ["Fwd2S L=14 VEC4=true"], ["Inv2S L=14 VEC4=true"]),
    S("2d-db4-ragged", [250, 32], "db4", ["Fwd2S L=8 VEC4=false"], ["Inv2S L=8 VEC4=false"]),                                   # 250 % 4 != 0
    S("2d-c64-db5", [128, 40], "db5", ["Fwd2S L=10 EW=2"], ["Inv2S L=10 EW=2"], cplx=True),
    S("2d-f64-db4-inv2p", [260, 96], "db4", ["Fwd2S T=double L=8"], ["Inv2P T=double L=8"], prec="double", cuts=[(5, 69, 9), (40, 110, 0)]),
    S("2d-f64-db8", [260, 64], "db8", ["Fwd2S T=double L=16"], ["Inv2S T=double L=16"], prec="double"),
    # the y filter is the shorter one: per-axis, y first with its halo (AxisMarch L=4), x periodic (AxisX: 256 >= 8 * 8)
    S("2d-y-filter-short-per-axis", [256, 16], ["db4", "db2"], ["AxisMarch L=4 SYN=false", "~AxisX L=8 SYN=false VEC4=true"],
      ["AxisMarch L=4 SYN=true", "~AxisX L=8 SYN=true VEC4=true"], whole="fused2d"),
]

# (kernel instance, mode) pairs that some row must have launched, with the oracle agreeing.  Mode: z_wrap / y_wrap of the fused families,
# 0 for a per-axis kernel that ran with wrap = 0.  A kernel family of trace.FAMILY_PARAMS is either here or in NO_SLAB_BRANCH.
_FWD3 = ["Fwd3 T=float EW=1 L=4", "Fwd3 T=float EW=1 L=8 TY=16", "Fwd3 TY=32 NT=1024 L=8", "Fwd3 T=float VEC4=false L=8", "Fwd3 L=10 PIN=true",
         "Fwd3 L=12 PIN=true", "Fwd3 L=14 PIN=true", "Fwd3 L=10 PIN=false T=float EW=1", "Fwd3 L=16 WLDS=2 T=float", "Fwd3 L=18 T=float",
         "Fwd3 L=20 WLDS=4", "Fwd3 L=20 WLDS=6 VEC4=false", "Fwd3 T=float EW=2 L=8", "Fwd3 T=float EW=2 L=10", "Fwd3 T=float EW=2 L=12",
         "Fwd3 T=double EW=2"] + [f"Fwd3 T=double EW=1 L={L}" for L in (6, 8, 10, 12, 14, 16)]
_INV3 = ["Inv3 L=8", "Inv3S T=float L=8", "Inv3S T=float L=10", "Inv3S T=float L=16", "Inv3S T=double EW=2"] + \
        [f"Inv3S T=double EW=1 L={L}" for L in (6, 8, 10, 12, 14, 16)] + \
        ["Inv3Y L=4 XSC=false", "Inv3Y L=8 XSC=false VEC4=true EW=1", "Inv3Y L=8 XSC=false VEC4=false", "Inv3Y L=10 XSC=true EW=1",
         "Inv3Y L=12 XSC=true EW=1", "Inv3Y L=12 XSC=false EW=1", "Inv3Y L=14 XSC=true", "Inv3Y L=16 XSC=true EW=1", "Inv3Y L=18 XSC=true",
         "Inv3Y L=20 TX=48 XSC=true", "Inv3Y L=20 TX=48 XSC=false VEC4=false", "Inv3Y EW=2 XSC=false", "Inv3Y EW=2 XSC=true L=10",
         "Inv3Y EW=2 XSC=true TX=48"]
_MODE0_ONLY = ("L=18", "L=20")                                # no split-halo / zero-extended form is offered above 16 taps (see the rows)
SLAB_COVERAGE = ([(s, m) for s in _FWD3 for m in (0, 2) if m == 0 or not any(t in s.split() for t in _MODE0_ONLY)] +
                 [(s, m) for s in _INV3 for m in (0, 3) if m == 0 or not any(t in s.split() for t in _MODE0_ONLY)] +
                 [(s, 0) for s in ["Fwd2S T=float VEC4=true EW=1", "Fwd2S VEC4=false", "Fwd2S EW=2", "Fwd2S T=double", "Fwd2S L=14",
                                   "Inv2S T=float VEC4=true EW=1", "Inv2S VEC4=false", "Inv2S EW=2", "Inv2S T=double", "Inv2S L=14",
                                   "Inv2P PK=true", "Inv2P T=double",
                                   "AxisMarch T=float SYN=false", "AxisMarch T=float SYN=true", "AxisMarch T=double SYN=false",
                                   "AxisMarch T=double SYN=true", "axis_analysis_kernel T=float", "axis_synthesis_kernel T=float"]])
NO_SLAB_BRANCH = {"Den3", "Fwd2C", "Inv2C", "AxisX"}          # whole arrays only: no halo switch in these kernels

RAN = {}                                                       # row id -> [(mode, launch record)] of the rows that passed


class _Guarded:
    """nblk blocks of cnt scalars on the device, each between `guard` scalars of a fill value (NaN around inputs, FILL around outputs)"""
    def __init__(self, nblk, cnt, guard, rdt, fill, data=None):
        self.cnt, self.g, self.fill = int(cnt), int(guard), fill
        self.t = torch.full((nblk, self.g + self.cnt + self.g), fill, dtype=rdt, device="cuda")
        self.pay = self.t[:, self.g:self.g + self.cnt]
        if data is not None:
            flat = np.ascontiguousarray(data)
            flat = flat.view(flat.real.dtype).reshape(nblk, self.cnt)
            self.pay.copy_(torch.from_numpy(flat).to(rdt))
        self.snap = self.t.clone()
        self.idt = torch.int32 if rdt == torch.float32 else torch.int64

    def ptr(self, b=0, off=0):
        return self.t.data_ptr() + (b * self.t.shape[1] + self.g + int(off)) * self.t.element_size()

    def ptrs(self, off=0):
        return [self.ptr(b, off) for b in range(self.t.shape[0])]

    def unchanged(self):                                       # inputs: every bit, the NaN planes included
        return torch.equal(self.t.view(self.idt), self.snap.view(self.idt))

    def guards_intact(self):                                   # outputs: the guard scalars against the pristine clone
        c = self.t.clone()
        c[:, self.g:self.g + self.cnt] = self.fill
        return torch.equal(c.view(self.idt), self.snap.view(self.idt))

    def numpy(self, shape, cdt):
        a = self.pay.contiguous().cpu().numpy()
        return a.view(cdt).reshape((self.t.shape[0],) + tuple(shape))


def _sublattices(fn, a, d, stride):
    """a level of tap stride s on axes that divide by s IS the stride-1 level on each of the s^d sub-lattices (sample n = s m + r reads
    samples s (m + j) + r only): the level-1 oracle applied to each of them"""
    if stride == 1:
        return fn(a)
    out = None
    for offs in itertools.product(range(stride), repeat=d):
        sl = tuple(slice(o, None, stride) for o in offs)
        r = fn(np.ascontiguousarray(a[sl]))
        if out is None:
            out = np.empty(tuple(a.shape[:d]) + r.shape[d:], dtype=r.dtype)
        out[sl] = r
    return out


def run_row(row):
    dims, wl, prec, cplx, ax, stride = row["dims"], row["wl"], row["prec"], row["cplx"], row["axis"], row["stride"]
    d, N = len(dims), dims[row["axis"]]
    nb = 2 ** d
    ndt, tdt = _dtypes(prec, cplx)
    rdt = torch.float32 if prec == "single" else torch.float64
    hdt = np.complex128 if cplx else np.float64
    tol, comp = TOL[prec], 2 if cplx else 1
    L = 2 * int(wl[ax][2:])
    assert all(n % stride == 0 for n in dims)
    rng = np.random.default_rng(zlib.crc32(repr((dims, wl, prec, cplx, ax, stride)).encode()))

    def draw(shape):
        a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
        return a.astype(ndt).astype(hdt)                       # the oracle sees what the device sees

    # ---- all data and the whole-volume oracle, once per row
    x = draw(dims)
    c = draw(dims + [nb])
    want = _sublattices(lambda a: orc_c.spatial_dec(a, wl, 1, 1), x, d, stride)
    want_r = _sublattices(lambda a: orc_c.spatial_rec(a, wl, 1), c, d, stride)
    kax = d - 1 - ax                                           # the sharded axis in kernel order (x fastest)
    xk, rk = np.ascontiguousarray(x.T), np.ascontiguousarray(want_r.T)
    yk, ck = np.ascontiguousarray(want.T), np.ascontiguousarray(c.T)      # (bands, nd, .., n1)
    ymax, rmax, cmax = np.abs(want).max(), np.abs(want_r).max(), np.abs(c).max()
    plane = comp * int(np.prod(dims[:ax]))                     # scalars of one plane of the sharded axis
    outer = int(np.prod(dims[ax + 1:]))                        # 4-D sharded on z: the frames
    what = f"{row['id']} {dims} {wl} {prec}{' complex' if cplx else ''} axis {ax} stride {stride}"
    stream = torch.cuda.current_stream().cuda_stream
    if row["whole"]:
        full = ndwt.Plan(dims, wl, rdt, cplx, True, "atrous" if stride > 1 else "reference", max_level=1)
        assert full.describe() == row["whole"], what
    launched = []

    def take(a, lo, hi, bands=False):                          # planes [lo, hi) of the periodic volume
        return np.ascontiguousarray(np.take(a, np.arange(lo, hi) % N, axis=kax + (1 if bands else 0)))

    def inbuf(a, nblk):
        return _Guarded(nblk, a.size * comp // nblk, 2 * plane, rdt, float("nan"), a.astype(ndt))

    def outbuf(nblk, planes):
        return _Guarded(nblk, outer * planes * plane, plane, rdt, FILL)

    def shape_of(planes):
        s = list(dims[::-1])
        s[kax] = planes
        if cplx:
            s[-1] = dims[0]
        return s

    for z0, z1, zc in row["cuts"]:
        nl = z1 - z0
        local = list(dims)
        local[ax] = nl
        plan = ndwt.Plan(local, wl, rdt, cplx, True, "atrous" if stride > 1 else "reference", max_level=2 if stride > 1 else 1,
                         global_outer=N, shard_axis=ax if ax != d - 1 else None)
        plan.set_tuning(0, zc)
        if row["fwd"] >= 0 or row["inv"] >= 0:
            plan.set_variant(fwd=row["fwd"], inv=row["inv"])
        ab, aa, sb, sa = plan.slab_halo(stride)
        assert (ab, aa, sb, sa) == ((L // 2 - 1) * stride, (L // 2) * stride, (L // 2) * stride, (L // 2 - 1) * stride), what
        assert bool(ndwt.lib().ndwt_plan_slab_fast(plan._h)) == row["fast"] or stride > 1, what
        fast3 = d == 3 and row["fast"]                         # the run-of-planes forms
        zslab = ax != d - 1
        cut = f"{what} planes [{z0}, {z1}) chunk {zc}"

        def call(name, mode, specs, fn, ins, out):
            with ndwt.kernel_trace() as recs:
                fn()
            torch.cuda.synchronize()
            check_trace(recs, [s.lstrip("~") for s in specs], f"{name} {cut}")
            assert bool(torch.isfinite(out.pay).all()), (cut, name, "a NaN plane was read, or an output element was not written")
            assert out.guards_intact(), (cut, name, "stored outside the output")
            assert all(i.unchanged() for i in ins), (cut, name, "an input was modified")
            halo = [spec(s) for s in specs if not s.startswith("~")]
            launched.extend((mode, r) for r in recs if any(matches(r, sp) for sp in halo))

        def ana_err(got, lo, hi):
            return np.abs(got - take(yk, lo, hi, True)).max() / ymax

        # ---- haloed analysis (mode 0)
        xin = inbuf(take(xk, z0 - ab, z1 + aa), 1)
        o0 = outbuf(nb, nl)
        call("analysis_level_slab", 0, row["ana"], lambda: plan.analysis_level_slab(xin.ptr(), o0.ptrs(), stride, stream), [xin], o0)
        err = ana_err(o0.numpy(shape_of(nl), ndt), z0, z1)
        assert err <= tol, (cut, "analysis_level_slab", err)

        # ---- split-halo analysis (mode 2; a z-slab is assembled with its halo first and then runs mode 0)
        if fast3 or zslab:
            loc, hb, ha = inbuf(take(xk, z0, z1), 1), inbuf(take(xk, z0 - ab, z0), 1), inbuf(take(xk, z1, z1 + aa), 1)
            o2 = outbuf(nb, nl)
            call("analysis_level_slab_split", 0 if zslab else 2, row["ana"] + (["~segments_strided_kernel"] if zslab else []),
                 lambda: plan.analysis_level_slab_split(loc.ptr(), hb.ptr(), ha.ptr(), o2.ptrs(), stride, stream), [loc, hb, ha], o2)
            err = ana_err(o2.numpy(shape_of(nl), ndt), z0, z1)
            assert err <= tol, (cut, "analysis_level_slab_split", err)
            assert torch.equal(o2.pay, o0.pay), (cut, "split-halo analysis differs from the haloed one: same kernel, same operands")
        elif d == 3:
            with pytest.raises(ndwt.NdwtError):
                plan.analysis_level_slab_split(xin.ptr(), xin.ptr(), xin.ptr(), o0.ptrs(), stride, stream)
        if fast3 and nl >= L:                                  # three runs: the interior, whose halo is the slab itself, and the two ends
            o3 = outbuf(nb, nl)
            runs = ((ab, nl - aa, loc.ptr(0, 0), loc.ptr(0, (nl - aa) * plane)), (0, ab, hb.ptr(), loc.ptr(0, ab * plane)),
                    (nl - aa, nl, loc.ptr(0, (nl - aa - ab) * plane), ha.ptr()))

            def parts():
                for a0, a1, before, after in runs:
                    plan.analysis_level_slab_part(loc.ptr(0, a0 * plane), before, after, o3.ptrs(a0 * plane), a1 - a0, stride, stream)
            call("analysis_level_slab_part", 2, row["ana"], parts, [loc, hb, ha], o3)
            err = ana_err(o3.numpy(shape_of(nl), ndt), z0, z1)
            assert err <= tol, (cut, "analysis_level_slab_part", err)
            assert torch.equal(o3.pay, o0.pay), (cut, "runs of the split-halo analysis differ from the haloed one")
            # both ends in one launch: two runs of m planes on the contiguous haloed input, the planes between them untouched
            m = max(ab, aa)
            o4 = outbuf(nb, nl)
            call("analysis_level_slab_runs", 0, row["ana"],
                 lambda: plan.analysis_level_slab_runs(xin.ptr(), o4.ptrs(), m, 2, nl - m, stride, stream), [xin], o4)
            g4, g0 = o4.numpy(shape_of(nl), ndt), o0.numpy(shape_of(nl), ndt)
            assert max(ana_err(g4[:, :m], z0, z0 + m), ana_err(g4[:, nl - m:], z1 - m, z1)) <= tol, (cut, "analysis_level_slab_runs")
            assert np.array_equal(g4[:, :m], g0[:, :m]) and np.array_equal(g4[:, nl - m:], g0[:, nl - m:]), (cut, "analysis_level_slab_runs")
            assert bool((o4.pay.reshape(nb, nl, plane)[:, m:nl - m] == FILL).all()), (cut, "analysis_level_slab_runs wrote between its runs")

        # ---- haloed synthesis (mode 0)
        cin = inbuf(take(ck, z0 - sb, z1 + sa, True), nb)
        r0 = outbuf(1, nl)
        call("synthesis_level_slab", 0, row["syn"], lambda: plan.synthesis_level_slab(cin.ptrs(), r0.ptr(), stride, stream), [cin], r0)
        err = np.abs(r0.numpy(shape_of(nl), ndt)[0] - take(rk, z0, z1)).max() / max(rmax, cmax)
        assert err <= 4 * tol, (cut, "synthesis_level_slab", err)

        # ---- zero-extended synthesis (mode 3): the oracle on the coefficients zeroed outside the slab
        if not row["ext"]:
            if d == 3:
                with pytest.raises(ndwt.NdwtError):
                    plan.synthesis_level_slab_ext(cin.ptrs(), r0.ptr(), stride, stream)
            continue
        assert N >= nl + 2 * (L - 1), "the support of the zero-extended slab must not meet itself round the wrap"
        cz = np.zeros_like(ck)
        idx = [slice(None)] * ck.ndim
        idx[kax + 1] = np.arange(z0, z1) % N
        cz[tuple(idx)] = ck[tuple(idx)]
        rz = np.ascontiguousarray(orc_c.spatial_rec(np.ascontiguousarray(cz.T), wl, 1).T)
        want_e = take(rz, z0 - sa, z1 + sb)                    # sa planes owed to the slab before, the slab, sb planes owed to the one after
        den = max(np.abs(rz).max(), cmax)
        ne = sa + nl + sb
        cl = inbuf(take(ck, z0, z1, True), nb)
        e0 = outbuf(1, ne)
        # (4-D sharded on t: the fused launches run periodic per frame, the t pass reads the zero-padded t-bands with wrap = 0)
        call("synthesis_level_slab_ext", 0 if d == 4 and not zslab else 3, row["syn"],
             lambda: plan.synthesis_level_slab_ext(cl.ptrs(), e0.ptr(), stride, stream), [cl], e0)
        err = np.abs(e0.numpy(shape_of(ne), ndt)[0] - want_e).max() / den
        assert err <= 4 * tol, (cut, "synthesis_level_slab_ext", err)
        if not fast3:
            continue
        e1 = outbuf(1, ne)

        def sparts():
            for a0, a1 in ((0, sa), (sa + nl, ne), (sa, sa + nl)):
                plan.synthesis_level_slab_part(cl.ptrs(), nl, a0, a1 - a0, e1.ptr(0, a0 * plane), stride, stream)
        call("synthesis_level_slab_part", 3, row["syn"], sparts, [cl], e1)
        err = np.abs(e1.numpy(shape_of(ne), ndt)[0] - want_e).max() / den
        assert err <= 4 * tol, (cut, "synthesis_level_slab_part", err)
        # the two ends in one launch: run r = planes [r (n + sa), + sb) of the zero-extended result (zlo, zhi and zbs at work)
        e2 = outbuf(1, 2 * sb)
        call("synthesis_level_slab_runs", 3, row["syn"],
             lambda: plan.synthesis_level_slab_runs(cl.ptrs(), nl, 0, nl + sa, 2, sb, e2.ptr(), stride, stream), [cl], e2)
        g2 = e2.numpy(shape_of(2 * sb), ndt)[0]
        err = max(np.abs(g2[:sb] - want_e[:sb]).max(), np.abs(g2[sb:] - want_e[nl + sa:]).max()) / den
        assert err <= 4 * tol, (cut, "synthesis_level_slab_runs", err)
    RAN[row["id"]] = launched


@pytest.mark.parametrize("row", ROWS)
def test_slab_dispatch_row(row):
    run_row(row)


def test_slab_dispatch_coverage():
    """every (kernel instance, mode) pair of SLAB_COVERAGE was launched by a row that agreed with the oracle; every kernel family of the
    library is in that list or named as having no halo branch"""
    for p in ROWS:                                             # run on its own, this test runs the rows it needs
        if p.values[0]["id"] not in RAN:
            run_row(p.values[0])
    seen = [mr for recs in RAN.values() for mr in recs]
    missing = [f"[{s}] mode {m}" for s, m in SLAB_COVERAGE if not any(mode == m and matches(r, spec(s)) for mode, r in seen)]
    assert not missing, f"not reached by any slab row: {missing}"
    listed = {spec(s)[0] for s, _ in SLAB_COVERAGE}
    families = set(ndwt.trace.FAMILY_PARAMS)
    assert families - listed == NO_SLAB_BRANCH, f"kernel families without a slab row or an exemption: {sorted(families - listed - NO_SLAB_BRANCH)}"
