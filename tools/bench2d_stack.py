#!/usr/bin/env python3
"""Stack plans (ndwt_plan_create_axes) against what a caller did before them, db4, 3 levels, device-resident data, hipEvent timing:

  (a) K calls on an unbatched plan of the PARENT build, one per item (--parent-lib: its libndwt_hip.so, loaded into this process beside
      this build's; without it the unbatched plan of this build);
  (b) a stack plan, one launch per level (variants 9 / 9);
  (c) a stack plan with the 2-D cascade forced (variants 11 / 11); 3-D shapes have no (c).

Interleaved batches: after 5 warm-ups of every line, 4 rounds of 5 timed calls per line, the lines taking turns; the median of a line's 20.
The unbatched control (--control, default 4096 x 4096 float): one image on this build against the parent, the same way.

    python tools/bench2d_stack.py [--parent-lib PATH] [--shapes f32:64x512x512,...] [--level 3] [--control f32:4096x4096]

A shape is kind:K x n2 x n1 (images) or kind:K x n3 x n2 x n1 (volumes).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--shapes", default="f32:64x512x512,f32:256x256x256,f32:1024x128x128,f32:16x2048x2048,c64:64x512x512,f64:64x512x512,"
                                    "f64:16x1024x1024,c128:32x512x512,f32:8x128x128x128,f32:64x64x64x64")
ap.add_argument("--level", type=int, default=3)
ap.add_argument("--wname", default="db4")
ap.add_argument("--control", default="f32:4096x4096")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import ndwt_amd as ndwt  # noqa: E402

KINDS = {"f32": (torch.float32, False), "c64": (torch.float32, True), "f64": (torch.float64, False), "c128": (torch.float64, True)}
level = args.level
s = torch.cuda.current_stream().cuda_stream


class RawPlan:
    """an unbatched plan through the C ABI of any build of the library (the parent's knows nothing newer)"""

    def __init__(self, lib, dims, rdt, cplx):
        self.lib, self.h = lib, ctypes.c_void_p(None)
        d = len(dims)
        lib.ndwt_plan_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_char_p)] + [ctypes.c_int] * 6
        for f in (lib.ndwt_dec, lib.ndwt_rec):
            f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        lib.ndwt_plan_destroy.argtypes = [ctypes.c_void_p]
        rc = lib.ndwt_plan_create(ctypes.byref(self.h), d, (ctypes.c_int64 * d)(*dims), (ctypes.c_char_p * d)(*[args.wname.encode()] * d),
                                  0 if rdt == torch.float32 else 1, int(cplx), 1, 0, level, torch.cuda.current_device())
        assert rc == 0, rc

    def dec(self, x, y):
        assert self.lib.ndwt_dec(self.h, x, y, level, s) == 0

    def rec(self, y, x):
        assert self.lib.ndwt_rec(self.h, y, x, level, s) == 0

    def close(self):
        self.lib.ndwt_plan_destroy(self.h)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def interleaved(fns, rounds=4, per_round=5, warm=5):
    """{name: fn} -> {name: (median us, min, max)}"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k] += [once(fn) for _ in range(per_round)]
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


this_lib = ndwt.lib()
parent_lib = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None
print(f"device: {torch.cuda.get_device_name()}; parent build: {'loaded from ' + os.path.basename(args.parent_lib) if parent_lib else 'none (line (a) runs this build)'}")

for shape in [v for v in args.shapes.split(",") if v]:
    kind, dd = shape.split(":")
    K, *rev = (int(v) for v in dd.split("x"))
    dims = list(reversed(rev))                                # fastest axis first
    k = len(dims)
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    esize = (4 if rdt == torch.float32 else 8) * comp
    item = 1
    for d in dims:
        item *= d
    nb = int(ndwt.num_bands(k, level))
    x = torch.randn(K * item * comp, dtype=rdt, device="cuda")
    y = torch.randn(nb * K * item * comp, dtype=rdt, device="cuda")
    out_y, out_x = torch.empty_like(y), torch.empty_like(x)
    # (a): item j alone -- its coefficients packed per item
    pa = RawPlan(parent_lib or this_lib, dims, rdt, cplx)
    xs, ys = item * esize, nb * item * esize

    def dec_each():
        for j in range(K):
            pa.dec(x.data_ptr() + j * xs, out_y.data_ptr() + j * ys)

    def rec_each():
        for j in range(K):
            pa.rec(y.data_ptr() + j * ys, out_x.data_ptr() + j * xs)
    dec, rec = {"(a) K calls, unbatched plan" + (" of the parent" if parent_lib else ""): dec_each}, {}
    rec[next(iter(dec))] = rec_each
    plans = []
    for name, v in (("(b) stack plan, 9 / 9", 9), ("(c) stack plan, cascade forced (11 / 11)", 11)):
        if v == 11 and k != 2:
            continue
        p = ndwt.Plan(dims + [K], [args.wname] * k + [None], rdt, cplx, True, "reference", max_level=level, axes=tuple(range(k)))
        p.set_variant(fwd=v, inv=v)
        plans.append(p)
        dec[name] = (lambda p=p: p.dec(x.data_ptr(), out_y.data_ptr(), level, s))
        rec[name] = (lambda p=p: p.rec(y.data_ptr(), out_x.data_ptr(), level, s))
        print(f"    {name}: {p.describe()}")
    td, tr = interleaved(dec), interleaved(rec)
    print(f"{kind} {args.wname} level {level}, {K} items of {' x '.join(map(str, dims))} ({K * item * esize / 1e6:.1f} MB per band, item height {dims[1]})")
    for name in dec:
        print(f"    {name:48s} dec {td[name][0]:10.1f} us [{td[name][1]:.1f} .. {td[name][2]:.1f}]   rec {tr[name][0]:10.1f} us [{tr[name][1]:.1f} .. {tr[name][2]:.1f}]")
    print(json.dumps({"shape": shape, "level": level, "wname": args.wname, "bytes_per_band": K * item * esize,
                      "lines": {n: {"dec_us": round(td[n][0], 1), "rec_us": round(tr[n][0], 1)} for n in dec}}))
    pa.close()
    del x, y, out_x, out_y, plans, dec, rec
    torch.cuda.empty_cache()

if args.control and not parent_lib:
    print("unbatched control SKIPPED: it compares this build with the parent's and needs --parent-lib; line (a) above ran THIS build")
if args.control and parent_lib:
    kind, dd = args.control.split(":")
    dims = list(reversed([int(v) for v in dd.split("x")]))
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    n = comp
    for d in dims:
        n *= d
    nb = int(ndwt.num_bands(len(dims), level))
    x = torch.randn(n, dtype=rdt, device="cuda")
    y = torch.randn(nb * n, dtype=rdt, device="cuda")
    out_y, out_x = torch.empty_like(y), torch.empty_like(x)
    pl = {"parent": RawPlan(parent_lib, dims, rdt, cplx), "this build": RawPlan(this_lib, dims, rdt, cplx)}
    # (the two builds are held to half a percent: 10 rounds of 10 calls each, the median of 100)
    td = interleaved({k: (lambda p=p: p.dec(x.data_ptr(), out_y.data_ptr())) for k, p in pl.items()}, rounds=10, per_round=10)
    tr = interleaved({k: (lambda p=p: p.rec(y.data_ptr(), out_x.data_ptr())) for k, p in pl.items()}, rounds=10, per_round=10)
    print(f"unbatched control, {kind} {' x '.join(map(str, dims))} {args.wname} level {level}:")
    for k in pl:
        print(f"    {k:12s} dec {td[k][0]:9.1f} us [{td[k][1]:.1f} .. {td[k][2]:.1f}]   rec {tr[k][0]:9.1f} us [{tr[k][1]:.1f} .. {tr[k][2]:.1f}]")
    print(f"    this build / parent: dec {td['this build'][0] / td['parent'][0]:.4f}, rec {tr['this build'][0] / tr['parent'][0]:.4f}")
    print(json.dumps({"control": args.control, "dec_us": {k: round(td[k][0], 1) for k in pl}, "rec_us": {k: round(tr[k][0], 1) for k in pl}}))
