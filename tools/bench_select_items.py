#!/usr/bin/env python3
"""The median of |c| of every ITEM of a band on the device (ndwt_band_select_items), hipEvent timing: the two routes of
select_items_route (csrc/ndwt_select.h) against each other, and against what a user could do before.

  (9)   the loop: the BandHist / BandPick passes of ndwt_band_select once per item on that item's part, one copy back at the end
  (11)  one launch: ItemSelect, one workgroup runs all passes of one item
  (t)   torch.median(band.abs(), dim=1) on the same device band (the large shapes only: a copy of the band and a sort per item)

Route table: float and double at items in {8, 64} x item sizes 2^14, 2^18, 2^22 scalars -- fewer items than compute units, where the
crossover in item size is what csrc/ndwt_select.h needs (kItemsOneLaunchMaxScalars: the rule of DESIGN.md 4.3b).  Large shapes: 4096 x
4096 and 1024 x 128^2, where the one launch is taken unasked.  The data are Gaussian, item j scaled by j + 1; the two routes must return
the same bits.  Median of 20 timed calls in 4 interleaved rounds of 5 (9, 11, 9, 11, ..) after 3 warm-ups of each line; the copy of the
results and the synchronisation are inside the timed call.

    python tools/bench_select_items.py [--table f32,f64] [--large f32:4096x4096,f32:1024x16384] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--table", default="f32,f64")
ap.add_argument("--large", default="f32:4096x4096,f32:1024x16384,f64:4096x4096")
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ndwt_amd as ndwt  # noqa: E402

s = torch.cuda.current_stream().cuda_stream
CUS = torch.cuda.get_device_properties(0).multi_processor_count
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed_interleaved(fns, rounds=4, per=5, warm=3):
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


def one_shape(kind, items, n, with_torch):
    rdt = torch.float32 if kind == "f32" else torch.float64
    passes = 3 if kind == "f32" else 6
    band = torch.randn((items, n), device="cuda", dtype=rdt) * torch.arange(1, items + 1, device="cuda", dtype=rdt)[:, None]
    plans = {}
    for route in (9, 11):
        plans[route] = ndwt.Plan([n], ["db1"], rdt, False, max_level=1, howmany=items).set_variant(inv=route)
    ks = [(n - 1) // 2] if n % 2 else [n // 2 - 1, n // 2]
    call = lambda p: p.band_select_items(band.data_ptr(), 1, 0, ks, s)   # noqa: E731  (band 0 of a level-1 array: the band itself)
    got = {r: call(p) for r, p in plans.items()}
    assert got[9].tobytes() == got[11].tobytes()
    assert np.array_equal(got[9][:, 0], torch.sort(band.abs(), dim=1).values[:, ks[0]].double().cpu().numpy())
    fns = {r: (lambda p=p: call(p)) for r, p in plans.items()}
    if with_torch:
        fns["t"] = lambda: torch.median(band.abs(), dim=1).values.cpu()
    t = timed_interleaved(fns)
    mb = items * n * band.element_size() / 1e6
    line = f"{kind} {items:5d} x {n:8d} ({mb:8.1f} MB, {passes} passes)   loop {t[9]:10.1f} us   one launch {t[11]:10.1f} us   one / loop = {t[11] / t[9]:5.2f}"
    if with_torch:
        line += f"   torch.median(dim=1) {t['t']:10.1f} us ({t['t'] / t[11]:.1f} x the one launch)"
    say(line)
    say(json.dumps({"kind": kind, "items": items, "item_scalars": n, "us": {str(k): round(v, 1) for k, v in t.items()}}))
    del band


say(f"ndwt_band_select_items, the median of every item; {CUS} compute units")
for kind in [k for k in args.table.split(",") if k]:
    for items in (8, 64):
        for lg in (14, 18, 22):
            one_shape(kind, items, 1 << lg, False)
for spec in [v for v in args.large.split(",") if v]:
    kind, dims = spec.split(":")
    items, n = (int(v) for v in dims.split("x"))
    one_shape(kind, items, n, True)

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
