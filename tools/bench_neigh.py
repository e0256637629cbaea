#!/usr/bin/env python3
"""Neighbourhood shrinkage (ndwt_shrink_neigh), hipEvent timing.  Per workload:

  (a) torch composing the same soft rule band by band: the squares in double, the window sum as 2r + 1 torch.roll per filtered axis,
      g = ((S - t^2) / S).clamp(min=0), out = band * g -- tens of passes and three band-sized temporaries in double;
  (b) ndwt_shrink_neigh (Plan.shrink_neigh) from the array into a second one: one launch over all bands, the upload of the squared
      thresholds included;
  (c) the bytes of one read plus one write of the array at the copy rate (--copy-gbs: the "copy 1->1 linear" line of
      tools/micro/stream_pattern, which counts the bytes read and the bytes written -- the rate tools/bench_joint.py is judged by), the
      read part multiplied by the halo factor of the instance's tile, (TX + 2r)(TY + 2r) / (TX TY): what the kernel asks
      of the memory system if no halo element were found in a cache.  This is the figure the kernel is judged against.

Workloads at level 1, random coefficients (the call needs no transform), thresholds at about the median window sum: the 8 bands of a
512^3 float volume at r = 1 and r = 2, the same in double at r = 1, 64 float images of 512^2 at r = 1 (4 bands), 4096 float signals of
4096 samples at r = 2 (2 bands).  Median of 20 timed calls in 4 interleaved rounds of 5 after 5 warm-ups of each line, as
tools/bench_joint.py.  The library's values are checked against torch's before timing.

    python tools/bench_neigh.py [--shapes vol3:f32:512:1,vol3:f32:512:2,vol3:f64:512:1,stack2:f32:512x64:1,batch:f32:4096x4096:2] [--copy-gbs N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="vol3:f32:512:1,vol3:f32:512:2,vol3:f64:512:1,stack2:f32:512x64:1,batch:f32:4096x4096:2")
ap.add_argument("--copy-gbs", type=float, default=4681.0)
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


def halo_factor(nd, elem_bytes, r):
    """(TX + 2r)(TY + 2r) / (TX TY) of the instance's tile (csrc/ndwt_select.h: neigh_tx, neigh_ty)"""
    if nd < 3:
        return (256 + 2 * r) / 256
    ty = 16 if elem_bytes <= 4 or (elem_bytes <= 8 and r < 3) else 8
    return (64 + 2 * r) * (ty + 2 * r) / (64 * ty)


def torch_neigh(src, dst, shape, nd, r, thr):
    """band by band: src, dst lists of flat bands; shape = (items, n_{nd-1}, .., n_0)"""
    for v, o, t in zip(src, dst, thr):
        S = v.view(shape).double().pow(2)
        for axis in range(len(shape) - 1, len(shape) - 1 - nd, -1):
            T = torch.roll(S, r, axis)
            for d in range(-r + 1, r + 1):
                T = T + torch.roll(S, -d, axis)
            S = T
        g = ((S - t * t) / S).clamp(min=0).to(v.dtype)
        torch.mul(v.view(shape), g, out=o.view(shape))


def lines(name, plan, shape, nd, r, nb, rdt):
    N = int(np.prod(shape))
    gen = torch.Generator(device="cuda").manual_seed(7)
    y = torch.randn(nb * N, dtype=rdt, device="cuda", generator=gen)
    out, ref = torch.empty_like(y), torch.empty_like(y)
    M = (2 * r + 1) ** nd
    thr = np.full(nb, float(np.sqrt(M - 0.7)))                  # about the median of a chi-square of M degrees
    src = [y[b * N:(b + 1) * N] for b in range(nb)]
    shrink = lambda: plan.shrink_neigh(y.data_ptr(), out.data_ptr(), 1, thr, r, False, s)   # noqa: E731
    tshrink = lambda: torch_neigh(src, [ref[b * N:(b + 1) * N] for b in range(nb)], shape, nd, r, thr)   # noqa: E731
    shrink()
    tshrink()
    tol = 1e-5 if rdt == torch.float32 else 1e-12               # (torch squares in double without the fma and sums in another order)
    survive = float((out != 0).double().mean())
    assert torch.allclose(out, ref, rtol=tol, atol=tol) and 0.2 < survive < 0.8, (name, survive, float((out - ref).abs().max()))
    with ndwt.kernel_trace() as recs:
        shrink()
    t = timed_interleaved({"a": tshrink, "b": shrink})
    gb = nb * N * y.element_size() / 1e9
    halo = halo_factor(nd, y.element_size(), r)
    floor = (gb * halo + gb) / args.copy_gbs * 1e6
    say(f"{name}: {nb} bands of {'x'.join(str(v) for v in shape)} scalars, radius {r}, {gb * 1e3:.1f} MB read and as much written, {survive:.0%} of the "
        "coefficients survive; launches: " + ", ".join(f"{q.family}<{', '.join(str(v) for v in q.params.values())}> x {q.grid[0]}" for q in recs))
    say(f"    (a)  torch, squares in double / rolls / clamp / mul per band {t['a']:10.1f} us")
    say(f"    (b)  ndwt_shrink_neigh                                       {t['b']:10.1f} us   {2 * gb / t['b'] * 1e6:7.0f} GB/s of one read + one write   a / b = {t['a'] / t['b']:.2f}")
    say(f"    (c)  {halo:.3f} reads + one write at {args.copy_gbs:.0f} GB/s (copy)            {floor:10.1f} us   b / c = {t['b'] / floor:.2f}")
    say(json.dumps({"shape": name, "bands": nb, "dims": list(shape), "radius": r, "us": {k: round(v, 1) for k, v in t.items()}, "halo": round(halo, 4),
                    "floor_us": round(floor, 1)}))


for spec in args.shapes.split(","):
    what, kind, dims, r = spec.split(":")
    rdt = torch.float32 if kind == "f32" else torch.float64
    r = int(r)
    if what == "vol3":
        a = int(dims)
        plan, shape, nd, nb = ndwt.Plan([a, a, a], ["db4"] * 3, rdt, False, True, "reference", max_level=1), (1, a, a, a), 3, 8
    elif what == "stack2":
        a, K = (int(v) for v in dims.split("x"))
        plan, shape, nd, nb = ndwt.Plan([a, a, K], ["db4", "db4", None], rdt, False, True, "reference", max_level=1, axes=(0, 1)), (K, a, a), 2, 4
    else:
        K, a = (int(v) for v in dims.split("x"))               # batch:KxN
        plan, shape, nd, nb = ndwt.Plan([a], ["db4"], rdt, False, True, "reference", max_level=1, howmany=K), (K, a), 1, 2
    lines(spec, plan, shape, nd, r, nb, rdt)
    del plan
    torch.cuda.empty_cache()

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
