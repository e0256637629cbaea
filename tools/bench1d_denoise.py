#!/usr/bin/env python3
"""Denoising of a batched 1-D plan (ndwt_plan_create_many), device-resident data, hipEvent timing:

  (a) ndwt_denoise with ONE threshold, through the library named by --parent (a build of the parent commit, loaded into this process):
      what existed before per-band thresholds -- Fwd1C, the shrink passes, Inv1C;
  (b) this build's ndwt_denoise_bands on the general route (variant 9 / 9: dec, one shrink pass per band, rec);
  (c) this build's ndwt_denoise_bands in one launch (variant 11 / 11: Den1C).

Median of 20 timed calls in 4 interleaved rounds of 5 (a, b, c, a, b, c, ..) after 5 warm-ups of each line.  Beside the times: the
signal volumes each route moves -- 4 level + 4 for (a) and (b) (dec level + 2, a read and a write of every shrunk band, rec level + 2),
2 and the halo for (c).  --control adds the unbatched control: ndwt_denoise with a scalar on a batched plan and on a 64^3 volume, this
build against --parent.

    python tools/bench1d_denoise.py [--parent LIB] [--shapes f32:4096x4096,...] [--cases db4:4,db2:3] [--control]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default="", help="libndwt_hip.so of the parent commit; without it line (a) runs this build's ndwt_denoise")
ap.add_argument("--shapes", default="f32:4096x4096,f32:65536x256,f32:16x1048576,c64:4096x2048,f64:4096x4096")
ap.add_argument("--cases", default="db4:4,db2:3")
ap.add_argument("--control", action="store_true")
ap.add_argument("--swap", action="store_true", help="control: the parent first in every round")
ap.add_argument("--no-shapes", action="store_true", help="the control only")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ndwt_amd as ndwt  # noqa: E402

KINDS = {"f32": (torch.float32, False), "c64": (torch.float32, True), "f64": (torch.float64, False), "c128": (torch.float64, True)}
s = torch.cuda.current_stream().cuda_stream


class ParentPlan:
    """a batched (howmany) or plain plan of the parent commit's library, through its C ABI"""

    def __init__(self, lib, dims, wnames, f64, cplx, level, howmany=None):
        self.lib, self.h = lib, ctypes.c_void_p(None)
        d = len(dims)
        cd, cn = (ctypes.c_int64 * d)(*dims), (ctypes.c_char_p * d)(*[w.encode() for w in wnames])
        if howmany is None:
            lib.ndwt_plan_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_char_p)] + [ctypes.c_int] * 6
            rc = lib.ndwt_plan_create(ctypes.byref(self.h), d, cd, cn, int(f64), int(cplx), 1, 0, level, 0)
        else:
            lib.ndwt_plan_create_many.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64,
                                                  ctypes.POINTER(ctypes.c_char_p)] + [ctypes.c_int] * 6
            rc = lib.ndwt_plan_create_many(ctypes.byref(self.h), d, cd, howmany, cn, int(f64), int(cplx), 1, 0, level, 0)
        assert rc == 0, rc
        lib.ndwt_denoise.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
        lib.ndwt_plan_destroy.argtypes = [ctypes.c_void_p]

    def denoise(self, x, out, level, thr):
        assert self.lib.ndwt_denoise(self.h, x, out, level, thr, 0, ctypes.c_void_p(s)) == 0

    def close(self):
        self.lib.ndwt_plan_destroy(self.h)


def timed_interleaved(fns, rounds=4, per=5, warm=5):
    for f in fns.values():
        for _ in range(warm):
            f()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            for _ in range(per):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: statistics.median(v) for k, v in ts.items()}


parent = ctypes.CDLL(os.path.abspath(args.parent)) if args.parent else None
print(f"line (a): {'the parent library ' + args.parent if parent else 'THIS build (no --parent given)'}")
for case in ([] if args.no_shapes else args.cases.split(",")):
    wn, level = case.split(":")[0], int(case.split(":")[1])
    for shape in args.shapes.split(","):
        kind, kn = shape.split(":")
        K, n = (int(v) for v in kn.split("x"))
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        x = torch.randn(K * n * comp, dtype=rdt, device="cuda")
        outs = {k: torch.empty_like(x) for k in "abc"}
        thr = 1.5 * ndwt.band_gains([n], wn, level, pres_l2_norm=1)
        thr[0] = 0.0
        pa = ParentPlan(parent, [n], [wn], rdt == torch.float64, cplx, level, K) if parent else ndwt.Plan([n], [wn], rdt, cplx, True, "reference", max_level=level, howmany=K)
        pb = ndwt.Plan([n], [wn], rdt, cplx, True, "reference", max_level=level, howmany=K)
        pb.set_variant(fwd=9, inv=9)
        pc = ndwt.Plan([n], [wn], rdt, cplx, True, "reference", max_level=level, howmany=K)
        pc.set_variant(fwd=11, inv=11)
        fa = (lambda: pa.denoise(x.data_ptr(), outs["a"].data_ptr(), level, float(thr[-1]))) if parent else \
             (lambda: pa.denoise(x.data_ptr(), outs["a"].data_ptr(), level, float(thr[-1]), False, s))
        with ndwt.kernel_trace() as recs:
            pc.denoise_bands(x.data_ptr(), outs["c"].data_ptr(), level, thr, False, s)
        one_launch = [r.family for r in recs] == ["Den1C"]
        t = timed_interleaved({
            "a": fa,
            "b": lambda: pb.denoise_bands(x.data_ptr(), outs["b"].data_ptr(), level, thr, False, s),
            "c": lambda: pc.denoise_bands(x.data_ptr(), outs["c"].data_ptr(), level, thr, False, s)})
        torch.cuda.synchronize()
        diff = float((outs["c"] - outs["b"]).abs().max())
        vol_mb = K * n * comp * (4 if rdt == torch.float32 else 8) / 1e6
        print(f"{kind} {wn} level {level}, K x n = {K} x {n} ({vol_mb:.1f} MB per volume); (c) is {'Den1C' if one_launch else 'NOT one launch: ' + str([r.family for r in recs])}; "
              f"max |c - b| {diff:.3g}")
        for k, name, vols in (("a", "(a) ndwt_denoise, one threshold" + (", parent" if parent else ""), 4 * level + 4),
                              ("b", "(b) ndwt_denoise_bands, general route", 4 * level + 4), ("c", "(c) ndwt_denoise_bands, one launch", 2)):
            print(f"    {name:44s} {t[k]:10.1f} us   ({vols * vol_mb / 1e3 / t[k] * 1e6:7.0f} GB/s of {vols} volumes)   c / this = {t['c'] / t[k]:.3f}")
        print(json.dumps({"shape": shape, "wname": wn, "level": level, "one_launch": one_launch, "us": {k: round(v, 1) for k, v in t.items()}}))
        if parent:
            pa.close()
        del pa, pb, pc, x, outs
        torch.cuda.empty_cache()

if args.control:
    print("control: ndwt_denoise with a scalar, this build against the parent (interleaved)")
    for name, dims, wn, level, K in (("batched f32 4096 x 4096 db4 level 4", [4096], ["db4"], 4, 4096), ("64^3 f32 db2 level 3", [64, 64, 64], ["db2"] * 3, 3, None)):
        nel = int(np.prod(dims)) * (K or 1)
        x, o = torch.randn(nel, dtype=torch.float32, device="cuda"), torch.empty(nel, dtype=torch.float32, device="cuda")
        pn = ndwt.Plan(dims, wn, torch.float32, False, True, "reference", max_level=level, howmany=K)
        fns = {"this": lambda: pn.denoise(x.data_ptr(), o.data_ptr(), level, 0.3, False, s)}
        if parent:
            pp = ParentPlan(parent, dims, wn, False, False, level, K)
            fns["parent"] = lambda: pp.denoise(x.data_ptr(), o.data_ptr(), level, 0.3)
        if args.swap:
            fns = dict(reversed(list(fns.items())))
        t = timed_interleaved(fns)
        print(f"    {name}: " + ", ".join(f"{k} {v:.1f} us" for k, v in t.items()) + (f", this / parent = {t['this'] / t['parent']:.4f}" if parent else ""))
        print(json.dumps({"control": name, "us": {k: round(v, 1) for k, v in t.items()}}))
