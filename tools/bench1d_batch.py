#!/usr/bin/env python3
"""Batched 1-D plans (ndwt_plan_create_many) against what a caller did before them, db4, device-resident data, hipEvent timing:

  (a) K calls on an unbatched plan, one per signal (what a user does without a batched plan; runs on a build without them too);
  (b) a batched plan with the cascade off (variant 9): one AxisX launch per level over all K signals;
  (c) a batched plan as it dispatches by default: two to four levels per launch (Fwd1C / Inv1C).

Median of 20 timed calls after 5 warm-ups; line (a) of a shape with more than 20 000 launches per call: median of 3 after 1 (said in
its line).  Beside the times: the algorithmic bytes, (level + 2) signal volumes per direction for (c), 3 level for (a) and (b).

    python tools/bench1d_batch.py [--root DIR] [--only a|bc] [--shapes f32:4096x4096,f32:16x1048576,...] [--level 4]

--root: the directory that holds the package to measure (default: this checkout) -- a build of the parent commit for its line (a).
"""
import argparse
import importlib
import inspect
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--only", default="abc")
ap.add_argument("--shapes", default="f32:4096x4096,f32:65536x256,f32:16x1048576,f32:1x16777216,c64:4096x2048,f64:4096x4096")
ap.add_argument("--level", type=int, default=4)
ap.add_argument("--wname", default="db4")
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch  # noqa: E402

api = importlib.import_module("non-decimated_wavelets_amd.api")
BATCHED = "howmany" in inspect.signature(api.Plan.__init__).parameters
KINDS = {"f32": (torch.float32, False), "c64": (torch.float32, True), "f64": (torch.float64, False), "c128": (torch.float64, True)}
level, nb = args.level, 1 + args.level
s = torch.cuda.current_stream().cuda_stream


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


for shape in args.shapes.split(","):
    kind, kn = shape.split(":")
    K, n = (int(v) for v in kn.split("x"))
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    esize = (4 if rdt == torch.float32 else 8) * comp
    x = torch.randn(K * n * comp, dtype=rdt, device="cuda")
    y = torch.randn(nb * K * n * comp, dtype=rdt, device="cuda")
    out_y, out_x = torch.empty_like(y), torch.empty_like(x)
    vol_mb = K * n * esize / 1e6
    lines = {}
    if "a" in args.only:
        p = api.Plan([n], [args.wname], rdt, cplx, True, "reference", max_level=level)
        xs, ys = n * esize, nb * n * esize

        def dec_each():
            for k in range(K):
                p.dec(x.data_ptr() + k * xs, out_y.data_ptr() + k * ys, level, s)

        def rec_each():
            for k in range(K):
                p.rec(y.data_ptr() + k * ys, out_x.data_ptr() + k * xs, level, s)
        reps, warm = (20, 5) if K * level <= 20000 else (3, 1)
        lines[f"(a) {K} calls, unbatched plan" + ("" if reps == 20 else f" [median of {reps}]")] = (timed(dec_each, reps, warm), timed(rec_each, reps, warm), 3 * level)
    if BATCHED and ("b" in args.only or "c" in args.only):
        ref = None
        for name, v, vols in (("(b) batched plan, variant 9", 9, 3 * level), ("(c) batched plan, default", 0, level + 2)):
            p = api.Plan([n], [args.wname], rdt, cplx, True, "reference", max_level=level, howmany=K)
            p.set_variant(fwd=v, inv=v)
            lines[name] = (timed(lambda: p.dec(x.data_ptr(), out_y.data_ptr(), level, s), 20, 5),
                           timed(lambda: p.rec(y.data_ptr(), out_x.data_ptr(), level, s), 20, 5), vols)
            torch.cuda.synchronize()
            if ref is None:
                ref = (out_y.clone(), out_x.clone())
            else:
                print(f"    default against variant 9: dec bit-identical {torch.equal(out_y, ref[0])}, rec bit-identical {torch.equal(out_x, ref[1])}, "
                      f"rec max |diff| {float((out_x - ref[1]).abs().max()):.3g}")
            del p
    print(f"{kind} {args.wname} level {level}, K x n = {K} x {n} ({vol_mb:.1f} MB per band)")
    for name, (td, tr, vols) in lines.items():
        gb = vols * vol_mb / 1e3
        print(f"    {name:42s} dec {td:10.1f} us ({gb / td * 1e6:7.0f} GB/s of {vols} volumes)   rec {tr:10.1f} us ({gb / tr * 1e6:7.0f} GB/s)")
    print(json.dumps({"shape": shape, "level": level, "wname": args.wname,
                      "lines": {k: {"dec_us": round(v[0], 1), "rec_us": round(v[1], 1), "volumes": v[2]} for k, v in lines.items()}}))
    del x, y, out_x, out_y
    torch.cuda.empty_cache()
