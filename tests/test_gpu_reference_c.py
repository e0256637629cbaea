"""The HIP transforms against the reference's own C code, directly -- not through the oracle.

Part a, always: tests/golden/refc/*.npz, written by mex/nddwt.c of the reference (tests/golden/make_golden_refc.py), through the four
classes and through the C ABI (Plan.dec / Plan.rec on raw pointers, the output between guard words), in double and single precision,
real and complex data, both pres_l2_norm settings, with set_path(False) and set_path(True).

Part b, where oracle/_ref/libnddwt_ref.so is present (it is built where a reference checkout is, and is never committed): the compiled
reference run on the spot at the smallest shape of tests/test_gpu_dispatch.py that reaches each kernel family; the launch trace must
show that family.  The input is rounded to the device precision first, as run_row does there.  Part b skips only when the library is
absent, and says so.

Tolerances of the project (tests/test_gpu_dispatch.py): dec <= TOL max|c|, rec <= 4 TOL max|c|, TOL = 1e-12 (fp64), 2e-6 (fp32);
c = the coefficients of the call (dec: the reference's output, rec: the input).
"""
import glob
import os
import time
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
import ndwt_ref as ref
from helpers import check_trace

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REFC = sorted(glob.glob(os.path.join(HERE, "golden", "refc", "*.npz")))
TOL = {"single": 2e-6, "double": 1e-12}
WORST = {"a": {"single": 0.0, "double": 0.0}, "b": {"single": 0.0, "double": 0.0}}     # relative to max|c|; a rec error counts at a quarter
PART_B = {"ran": 0}
GUARD, NGUARD = 7.25, 8
PER_AXIS_ONLY = {"axis_analysis_kernel", "axis_synthesis_kernel"}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for part in ("a", "b"):
        print(f"\n[gpu-reference-c] part {part}: worst HIP error against the reference's C code, relative to max|c| (rec / 4): "
              + ", ".join(f"{p} {WORST[part][p]:.3g} (bound {TOL[p]:.0e})" for p in ("double", "single")))
    if PART_B["ran"]:
        print(f"[gpu-reference-c] part b RAN: {PART_B['ran']} direct cases against {ref.LIB_PATH}")
    else:
        print("[gpu-reference-c] part b SKIPPED: oracle/_ref/libnddwt_ref.so is not here")


def _cls(d):
    return {1: ndwt.nd_dwt_1D, 2: ndwt.nd_dwt_2D, 3: ndwt.nd_dwt_3D, 4: ndwt.nd_dwt_4D}[d]


def _dtypes(prec, cplx):
    real = np.float32 if prec == "single" else np.float64
    if not cplx:
        return real, (torch.float32 if prec == "single" else torch.float64)
    return (np.complex64 if prec == "single" else np.complex128), (torch.complex64 if prec == "single" else torch.complex128)


def _colmajor_gpu(a, tdt):
    """numpy MATLAB-shaped array -> GPU tensor of the same shape, column-major memory"""
    t = torch.from_numpy(np.ascontiguousarray(np.transpose(a))).cuda().to(tdt)
    return t.permute(*reversed(range(t.dim())))


class _Guarded:
    """n elements on the device between NGUARD guard words on either side"""
    def __init__(self, n, tdt):
        self.t = torch.full((n + 2 * NGUARD,), GUARD, dtype=tdt, device="cuda")
        self.view = self.t[NGUARD:NGUARD + n]

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.t[:NGUARD] == GUARD).all()) and bool((self.t[-NGUARD:] == GUARD).all())


def _hold(part, prec, got, want, scale, factor, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max() / scale)
    WORST[part][prec] = max(WORST[part][prec], err / factor)
    print(f"[gpu-reference-c] {what}: {err:.3g} (bound {factor * TOL[prec]:.3g})")
    assert err <= factor * TOL[prec], (what, err)


def _abi_dec_rec(plan, x, c, level, ndt, tdt, traces=None):
    """Plan.dec(x) and Plan.rec(c) on raw device pointers -> (y, r) in MATLAB shape; the outputs lie between guard words"""
    dims = list(x.shape)
    vol, nb = int(np.prod(dims)), c.shape[-1]
    stream = torch.cuda.current_stream().cuda_stream
    xb, yb = _Guarded(vol, tdt), _Guarded(nb * vol, tdt)
    xb.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(x)).astype(ndt).reshape(-1)).cuda())
    with ndwt.kernel_trace() as recs_d:
        plan.dec(xb.ptr(), yb.ptr(), level, stream)
    torch.cuda.synchronize()
    assert yb.intact() and xb.intact(), "dec stored outside its output"
    y = np.transpose(yb.view.cpu().numpy().reshape([nb] + dims[::-1]))
    cb, rb = _Guarded(nb * vol, tdt), _Guarded(vol, tdt)
    cb.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(c)).astype(ndt).reshape(-1)).cuda())
    with ndwt.kernel_trace() as recs_r:
        plan.rec(cb.ptr(), rb.ptr(), level, stream)
    torch.cuda.synchronize()
    assert rb.intact() and cb.intact(), "rec stored outside its output"
    r = np.transpose(rb.view.cpu().numpy().reshape(dims[::-1]))
    if traces is not None:
        traces += [recs_d, recs_r]
    return y, r


# ---------------------------------------------------------------------------------------------------------------------------------
# part a: the fixtures the reference wrote
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_reference_fixtures_travelled():
    assert len(REFC) == 10, REFC


@pytest.mark.parametrize("path", REFC, ids=[os.path.basename(p)[:-4] for p in REFC])
@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("generic", [False, True], ids=["auto", "generic"])
def test_hip_reproduces_the_reference_fixtures(path, precision, generic):
    g = np.load(path)
    base = os.path.basename(path)[:-4]
    cplx = base[-1] == "c"
    tag = base[-1]
    sizes, level, wl = [int(s) for s in g["sizes"]], int(g["level"]), [str(w) for w in g["wname"]]
    d = len(sizes)
    ndt, tdt = _dtypes(precision, cplx)
    x, c = g[f"x_{tag}"], g[f"c_{tag}"]
    assert np.iscomplexobj(x) == cplx
    for l2 in (0, 1):
        want_y, want_r = g[f"y_{tag}_l2{l2}"], g[f"rec_{tag}_l2{l2}"]
        what = f"{base} {precision} {'generic' if generic else 'auto'} l2={l2}"
        # the classes
        w = _cls(d)(wl[0] if d == 1 else wl, sizes, "pres_l2_norm", l2, "precision", precision)
        w._plan(cplx, level, torch.device("cuda", torch.cuda.current_device())).set_path(generic)
        y = w.dec(_colmajor_gpu(x, tdt), level)
        assert y.dtype == tdt and len(w._plans) == 1
        _hold("a", precision, y.cpu().numpy(), want_y, np.abs(want_y).max(), 1, f"class dec {what}")
        r = w.rec(_colmajor_gpu(c, tdt))
        assert r.dtype == tdt and len(w._plans) == 1
        _hold("a", precision, r.cpu().numpy(), want_r, np.abs(c).max(), 4, f"class rec {what}")
        # the C ABI
        plan = ndwt.Plan(sizes, wl, torch.float32 if precision == "single" else torch.float64, cplx, bool(l2), "reference", max_level=level)
        plan.set_path(generic)
        traces = []
        y, r = _abi_dec_rec(plan, x, c, level, ndt, tdt, traces)
        for recs in traces:
            assert recs, what
            if generic:
                assert {k.family for k in recs} <= PER_AXIS_ONLY, (what, recs)
        _hold("a", precision, y, want_y, np.abs(want_y).max(), 1, f"abi dec {what}")
        _hold("a", precision, r, want_r, np.abs(c).max(), 4, f"abi rec {what}")


# ---------------------------------------------------------------------------------------------------------------------------------
# part b: the compiled reference, run here, at the smallest shape of tests/test_gpu_dispatch.py that reaches each family
# ---------------------------------------------------------------------------------------------------------------------------------
def B(bid, dims, wn, prec="single", cplx=False, level=2, fwd=-1, inv=-1, dec=(), rec=()):
    return pytest.param(dict(dims=dims, wn=wn, prec=prec, cplx=cplx, level=level, fwd=fwd, inv=inv, dec=list(dec), rec=list(rec)), id=bid)


DIRECT = [
    B("fwd3-inv3y", [64, 40, 36], "db4", dec=["Fwd3 T=float L=8"], rec=["Inv3Y T=float L=8 XSC=false"]),
    B("fwd3-inv3s-f64", [64, 40, 36], "db4", prec="double", dec=["Fwd3 T=double L=8"], rec=["Inv3S T=double L=8"]),
    B("inv3y-scatter", [64, 40, 36], "db8", dec=["Fwd3 T=float L=16"], rec=["Inv3Y T=float L=16 XSC=true"]),
    B("c64", [32, 24, 20], "db4", cplx=True, dec=["Fwd3 T=float L=8 EW=2"], rec=["Inv3Y T=float L=8 EW=2"]),
    B("fwd2s-inv2p", [256, 64], "db4", dec=["Fwd2S T=float L=8"], rec=["Inv2P T=float L=8"]),
    B("inv2s", [256, 63], "db4", dec=["Fwd2S T=float L=8"], rec=["Inv2S T=float L=8"]),
    B("fwd2c-inv2c", [256, 96], "db4", level=3, fwd=11, inv=11, dec=["Fwd2C T=float L=8 NLEV=3"], rec=["Inv2C T=float L=8 NLEV=3"]),
    B("axisx", [4096], "db2", dec=["AxisX T=float L=4 SYN=false"], rec=["AxisX T=float L=4 SYN=true"]),
    B("plain-axis-f64", [4096], "db7", prec="double", dec=["axis_analysis_kernel T=double"], rec=["axis_synthesis_kernel T=double"]),
    B("fwd3-axismarch-4d", [24, 20, 12, 16], "db2", level=1, dec=["Fwd3 T=float L=4", "AxisMarch T=float L=4 SYN=false"],
      rec=["Inv3Y T=float L=4", "AxisMarch T=float L=4 SYN=true"]),
]


@pytest.mark.parametrize("case", DIRECT)
def test_hip_against_the_compiled_reference(case):
    if not ref.available():
        print("[gpu-reference-c] part b skipped: oracle/_ref/libnddwt_ref.so is not here")
        pytest.skip("oracle/_ref/libnddwt_ref.so is not here (it is built where a reference checkout is)")
    dims, wn, prec, cplx, level = case["dims"], case["wn"], case["prec"], case["cplx"], case["level"]
    d = len(dims)
    wl = [wn] * d
    ndt, tdt = _dtypes(prec, cplx)
    rng = np.random.default_rng(zlib.crc32(repr((dims, wn, prec, cplx, level)).encode()))
    wide = np.complex128 if cplx else np.float64
    x = rng.standard_normal(dims) + (1j * rng.standard_normal(dims) if cplx else 0)
    x = x.astype(ndt).astype(wide)                               # the reference sees the input the device sees
    nb = ndwt.num_bands(d, level)
    c = rng.standard_normal(dims + [nb]) + (1j * rng.standard_normal(dims + [nb]) if cplx else 0)
    c = c.astype(ndt).astype(wide)
    t0 = time.time()
    want_y = ref.dec(x, wl, level, 1)
    want_r = ref.rec(c, wl, 1)
    what = f"{dims} {wn} {prec}{' complex' if cplx else ''} L{level}"
    print(f"[gpu-reference-c] {what}: the compiled reference took {time.time() - t0:.2f} s")
    plan = ndwt.Plan(dims, wl, torch.float32 if prec == "single" else torch.float64, cplx, True, "reference", max_level=level)
    if case["fwd"] >= 0 or case["inv"] >= 0:
        plan.set_variant(fwd=case["fwd"], inv=case["inv"])
    traces = []
    y, r = _abi_dec_rec(plan, x, c, level, ndt, tdt, traces)
    check_trace(traces[0], case["dec"], f"dec {what}")
    check_trace(traces[1], case["rec"], f"rec {what}")
    print(f"[gpu-reference-c] {what}: ran dec {sorted({k.family for k in traces[0]})}, rec {sorted({k.family for k in traces[1]})}")
    _hold("b", prec, y, want_y, np.abs(want_y).max(), 1, f"direct dec {what}")
    _hold("b", prec, r, want_r, np.abs(c).max(), 4, f"direct rec {what}")
    PART_B["ran"] += 1
