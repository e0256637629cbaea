#!/usr/bin/env python3
"""The one-launch denoise of a batched 1-D plan with a threshold row per signal (ndwt_denoise_bands_items: Den1C<.., ROWTHR = true>)
against the same build's uniform one-launch denoise (ndwt_denoise_bands: Den1C, the parent's kernel, unchanged), device-resident data,
hipEvent timing.  Beside them the general route of the per-item call (variant 9 / 9: dec, one ShrinkItems launch, rec).

  (u)  ndwt_denoise_bands, one threshold row for all signals, variant 11 / 11
  (r)  ndwt_denoise_bands_items, a row per signal, variant 11 / 11 -- the upload of the table (signals x 5 scalars through the plan's
       pinned buffer) is inside the timed call
  (g)  ndwt_denoise_bands_items on the general route, variant 9 / 9

Expectation: (r) within the 5 % spread between boxes of (u): five uniform loads per wave more.  The ratio is recorded, not gated.
Median of 20 timed calls in 4 interleaved rounds of 5 (u, r, g, u, ..) after 5 warm-ups of each line, as tools/bench1d_denoise.py.

    python tools/bench1d_denoise_items.py [--shapes f32:4096x4096,f32:65536x256,f64:4096x4096] [--wname db4] [--level 4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="f32:4096x4096,f32:65536x256,f64:4096x4096")
ap.add_argument("--wname", default="db4")
ap.add_argument("--level", type=int, default=4)
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ndwt_amd as ndwt  # noqa: E402

s = torch.cuda.current_stream().cuda_stream
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


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


for spec in args.shapes.split(","):
    kind, dims = spec.split(":")
    K, n = (int(v) for v in dims.split("x"))
    rdt = torch.float32 if kind == "f32" else torch.float64
    level, nb = args.level, args.level + 1
    mk = lambda v: ndwt.Plan([n], [args.wname], rdt, False, True, "reference", max_level=level, howmany=K).set_variant(fwd=v, inv=v)   # noqa: E731
    pu, pr, pg = mk(11), mk(11), mk(9)
    x = torch.randn((K, n), device="cuda", dtype=rdt)
    out = torch.empty_like(x)
    row = np.array([0.0] + [0.5 + 0.25 * b for b in range(1, nb)])
    table = np.ascontiguousarray(np.outer(1.0 + np.arange(K) / K, row))
    # the same rows everywhere: the row-threshold launch returns the uniform launch's bits
    pu.denoise_bands(x.data_ptr(), out.data_ptr(), level, row, False, s)
    ref = out.clone()
    pr.denoise_bands_items(x.data_ptr(), out.data_ptr(), level, np.tile(row, (K, 1)), False, s)
    assert torch.equal(ref, out)
    with ndwt.kernel_trace() as recs:
        pr.denoise_bands_items(x.data_ptr(), out.data_ptr(), level, table, False, s)
    assert [r.family for r in recs] == ["Den1C"] and recs[0].params["ROWTHR"] is True, recs
    t = timed_interleaved({"u": lambda: pu.denoise_bands(x.data_ptr(), out.data_ptr(), level, row, False, s),
                           "r": lambda: pr.denoise_bands_items(x.data_ptr(), out.data_ptr(), level, table, False, s),
                           "g": lambda: pg.denoise_bands_items(x.data_ptr(), out.data_ptr(), level, table, False, s)})
    say(f"{kind} {K} x {n} {args.wname} L{level}:  uniform Den1C {t['u']:9.1f} us   row thresholds {t['r']:9.1f} us   r / u = {t['r'] / t['u']:.3f}"
        f"   general route {t['g']:9.1f} us   g / r = {t['g'] / t['r']:.2f}")
    say(json.dumps({"shape": spec, "wname": args.wname, "level": level, "us": {k: round(v, 1) for k, v in t.items()}}))
    del x, out, ref
    torch.cuda.empty_cache()

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
