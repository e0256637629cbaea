#!/usr/bin/env python3
"""Joint shrinkage across the items of a plan (ndwt_shrink_joint) and the group norms (ndwt_group_norms_dev), hipEvent timing.  Per shape:

  (a) torch doing the same soft group thresholding band by band on the band viewed as [items, n]: m = band.pow(2).sum(0).sqrt(),
      g = (1 - t / m).clamp(min=0), band.mul_(g) -- five passes and temporaries of a band and of an item;
  (b) ndwt_shrink_joint (Plan.shrink_joint): one launch over all bands, the upload of the thresholds included;
  (c) the bytes of one read plus one write of the array at the copy rate (--copy-gbs: the "copy 1->1 linear" line of
      tools/micro/stream_pattern of the same session, which counts the bytes read and the bytes written); where the plan has more items
      than JointShrink keeps in registers the kernel reads twice, and the line (c2) adds one more read at --read-gbs ("read linear");
  (d) torch computing the four group norms band by band; (e) ndwt_group_norms_dev, the results left on the device; (f) one read of the
      array at --read-gbs.

Shapes at level 1, float and double, random coefficients (the calls need no transform), thresholds at about the median group
magnitude: a stack of 8 volumes of 256^3 (8 bands; the group in registers), a stack of 32 images of 512^2 (4 bands; two sweeps, a
workgroup's step spans 128 KiB), a batch of 4096 signals of 4096 (2 bands; two sweeps over 4096 items, and only 1024 steps a band:
joint_chunks gives 4 workgroups a band).  The array is restored from a copy before every timed call of (a) and (b), outside the events.
Median of 20 timed calls in 4 interleaved rounds of 5 after 5 warm-ups of each line, as tools/bench_norms.py.  The library's values are
checked against torch's before timing.

    python tools/bench_joint.py [--shapes stack3:f32:256x8,stack2:f32:512x32,batch:f32:4096x4096,...] [--copy-gbs N] [--read-gbs N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="stack3:f32:256x8,stack2:f32:512x32,batch:f32:4096x4096,stack3:f64:256x8,stack2:f64:512x32,batch:f64:4096x4096")
ap.add_argument("--copy-gbs", type=float, default=0.0)
ap.add_argument("--read-gbs", type=float, default=0.0)
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ndwt_amd as ndwt  # noqa: E402

s = torch.cuda.current_stream().cuda_stream
KREG = 8                                                       # kJointReg (csrc/ndwt_select.h)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed_interleaved(fns, before=None, rounds=4, per=5, warm=5):
    for f in fns.values():
        for _ in range(warm):
            f()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            for _ in range(per):
                if before and k in before:
                    before[k]()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: statistics.median(v) for k, v in ts.items()}


def torch_shrink(bands, K, thr):
    for v, t in zip(bands, thr):
        v = v.view(K, -1)
        m = v.pow(2).sum(0).sqrt()
        g = (1 - t / m).clamp(min=0)
        v.mul_(g)


def torch_norms(bands, K):
    rows = []
    for v in bands:
        sq = v.view(K, -1).pow(2).sum(0, dtype=torch.float64)
        m = sq.sqrt()
        rows.append(torch.stack([m.sum(), sq.sum(), m.max(), torch.count_nonzero(sq).double()]))
    return torch.stack(rows)


def lines(name, plan, K, n, nb, rdt):
    N = K * n
    gen = torch.Generator(device="cuda").manual_seed(7)
    y0 = torch.randn(nb * N, dtype=rdt, device="cuda", generator=gen)
    y = y0.clone()
    bands = [y[b * N:(b + 1) * N] for b in range(nb)]
    thr = np.full(nb, float(np.sqrt(K - 0.5)))                  # about the median of a chi variable of K degrees
    restore = lambda: y.copy_(y0)                               # noqa: E731
    shrink = lambda: plan.shrink_joint(y.data_ptr(), 1, thr, False, s)   # noqa: E731
    tshrink = lambda: torch_shrink(bands, K, thr)               # noqa: E731
    out = torch.empty(nb * 4, dtype=torch.float64, device="cuda")
    norms = lambda: plan.group_norms_dev(y.data_ptr(), 1, out.data_ptr(), s)   # noqa: E731
    # the values first: the library against torch (torch sums the squares in the scalar type and in another order)
    shrink()
    got = y.clone()
    restore()
    tshrink()
    tol = 1e-4 if rdt == torch.float32 else 1e-11
    survive = float((got != 0).double().mean())
    assert torch.allclose(got, y, rtol=tol, atol=tol) and 0.2 < survive < 0.8, (name, survive)
    restore()
    norms()
    want = torch_norms(bands, K)
    assert torch.allclose(out.view(nb, 4), want, rtol=1e-5 if rdt == torch.float32 else 1e-12), name
    del got, want
    with ndwt.kernel_trace() as recs:
        shrink()
        norms()
    restore()
    t = timed_interleaved({"a": tshrink, "b": shrink, "d": lambda: torch_norms(bands, K), "e": norms}, before={"a": restore, "b": restore})
    gb = nb * N * y.element_size() / 1e9
    say(f"{name}: {nb} bands of {K} items of {n} scalars, {gb * 1e3:.1f} MB in all, {survive:.0%} of the coefficients survive; launches: " +
        ", ".join(f"{r.family}<{', '.join(str(v) for v in r.params.values())}> x {r.grid[0]}" for r in recs))
    say(f"    (a)  torch, pow / sum / sqrt / clamp / mul per band  {t['a']:10.1f} us")
    say(f"    (b)  ndwt_shrink_joint                               {t['b']:10.1f} us   {2 * gb / t['b'] * 1e6:7.0f} GB/s of one read + one write   a / b = {t['a'] / t['b']:.2f}")
    floor = floor2 = rfloor = 0.0
    if args.copy_gbs > 0:
        floor = 2 * gb / args.copy_gbs * 1e6
        say(f"    (c)  one read + one write at {args.copy_gbs:.0f} GB/s (copy)         {floor:10.1f} us   b / c = {t['b'] / floor:.2f}")
        if K > KREG and args.read_gbs > 0:
            floor2 = floor + gb / args.read_gbs * 1e6
            say(f"    (c2) two reads + one write (the second sweep)        {floor2:10.1f} us   b / c2 = {t['b'] / floor2:.2f}")
    say(f"    (d)  torch, the four group norms per band            {t['d']:10.1f} us")
    say(f"    (e)  ndwt_group_norms_dev (enqueue only)             {t['e']:10.1f} us   {gb / t['e'] * 1e6:7.0f} GB/s of one read   d / e = {t['d'] / t['e']:.2f}")
    if args.read_gbs > 0:
        rfloor = gb / args.read_gbs * 1e6
        say(f"    (f)  one read at {args.read_gbs:.0f} GB/s (read)                     {rfloor:10.1f} us   e / f = {t['e'] / rfloor:.2f}")
    say(json.dumps({"shape": name, "items": K, "bands": nb, "item_scalars": n, "us": {k: round(v, 1) for k, v in t.items()},
                    "floor_1r1w_us": round(floor, 1), "floor_2r1w_us": round(floor2, 1), "floor_1r_us": round(rfloor, 1)}))


for shape in args.shapes.split(","):
    what, kind, dims = shape.split(":")
    rdt = torch.float32 if kind == "f32" else torch.float64
    a, K = (int(v) for v in dims.split("x"))
    if what == "stack3":
        plan, n, nb = ndwt.Plan([a, a, a, K], ["db4"] * 3 + [None], rdt, False, True, "reference", max_level=1, axes=(0, 1, 2)), a ** 3, 8
    elif what == "stack2":
        plan, n, nb = ndwt.Plan([a, a, K], ["db4", "db4", None], rdt, False, True, "reference", max_level=1, axes=(0, 1)), a * a, 4
    else:
        a, K = K, a                                             # batch:KxN
        plan, n, nb = ndwt.Plan([a], ["db4"], rdt, False, True, "reference", max_level=1, howmany=K), a, 2
    assert plan.items == K
    lines(shape, plan, K, n, nb, rdt)
    del plan
    torch.cuda.empty_cache()

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
