#!/usr/bin/env python3
"""The four sums of every band of a coefficient array on the device (l1, energy, max, non-zeros), hipEvent timing.  Per shape:

  (a) torch computing the same four statistics on the same array, band by band: band.abs().sum(float64), (band * band).sum(float64),
      band.abs().max(), count_nonzero(band) -- per item: the same with dim=1 on the band viewed as [items, n]; the results stay on the
      device;
  (b) ndwt_band_norms (Plan.band_norms): one launch over all bands (and NormsFinish), the copy of the results and the synchronisation
      included; (b') ndwt_band_norms_dev: the same launches alone, the results left on the device; per item: ndwt_band_norms_items and
      the per_item device form;
  (c) the bytes of ONE read of the array divided by a read-only rate: --read-gbs, the "read linear" line of tools/micro/stream_pattern
      measured in the same session (without it the line is left out).

Shapes, float and double: the 8 level-1 bands of a 512^3 volume on the plan's band pitch (smooth signal + noise), and the 5 bands of a
4-level db4 dec of a 4096 x 4096 batch of signals, band-wide and per item.  Median of 20 timed calls in 4 interleaved rounds of 5 (a, b,
b', a, ...) after 5 warm-ups of each line, as tools/bench_select.py.  The library's values are checked against torch's before timing.

    python tools/bench_norms.py [--shapes vol:f32:512,batch:f32:4096x4096,...] [--read-gbs N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="vol:f32:512,batch:f32:4096x4096,vol:f64:512,batch:f64:4096x4096")
ap.add_argument("--read-gbs", type=float, default=0.0)
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


def torch_norms(bands, items):
    """[nb, 4] (items = 0) or [items, nb, 4] doubles on the device, band by band"""
    rows = []
    for b in bands:
        v = b.view(items, -1) if items else b
        a = v.abs()
        kw = {"dim": 1} if items else {}
        mx = a.amax(dim=1) if items else a.max()
        rows.append(torch.stack([a.sum(dtype=torch.float64, **kw), (v * v).sum(dtype=torch.float64, **kw), mx.double(),
                                 torch.count_nonzero(v, **kw).double()], dim=-1))
    return torch.stack(rows, dim=-2 if items else 0)


def norms_lines(name, plan, y, pitch, nb, N, level, items):
    """y: nb bands of N scalars at `pitch` scalars on the device"""
    bands = [y[b * pitch:b * pitch + N] for b in range(nb)]
    out = torch.empty(max(items, 1) * nb * 4, dtype=torch.float64, device="cuda")
    host = (lambda: plan.band_norms_items(y.data_ptr(), level, s, band_pitch=pitch)) if items else (lambda: plan.band_norms(y.data_ptr(), level, s, band_pitch=pitch))
    dev = lambda: plan.band_norms_dev(y.data_ptr(), level, out.data_ptr(), bool(items), s, band_pitch=pitch)   # noqa: E731
    got, want = host(), torch_norms(bands, items).cpu().numpy()
    dev()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == got.tobytes()
    assert np.array_equal(got[..., 2:], want[..., 2:]) and np.allclose(got[..., :2], want[..., :2], rtol=1e-6 if y.dtype == torch.float32 else 1e-12), name
    with ndwt.kernel_trace() as recs:
        dev()
    t = timed_interleaved({"a": lambda: torch_norms(bands, items), "b": host, "bdev": dev})
    gb = nb * N * y.element_size() / 1e9
    what = f"{items} items per band" if items else "band-wide"
    say(f"{name} ({what}): {nb} bands of {N} scalars, {gb * 1e3:.1f} MB in all; launches: " + ", ".join(f"{r.family} x {r.grid[0]}" for r in recs))
    say(f"    (a)  torch, four reductions per band            {t['a']:10.1f} us   {gb / t['a'] * 1e6:7.0f} GB/s of one read")
    say(f"    (b)  ndwt_band_norms{'_items' if items else '      '} (copy + sync)         {t['b']:10.1f} us   {gb / t['b'] * 1e6:7.0f} GB/s   a / b = {t['a'] / t['b']:.2f}")
    say(f"    (b') ndwt_band_norms_dev (enqueue only)         {t['bdev']:10.1f} us   {gb / t['bdev'] * 1e6:7.0f} GB/s   a / b' = {t['a'] / t['bdev']:.2f}")
    floor = gb / args.read_gbs * 1e6 if args.read_gbs > 0 else 0.0
    if floor:
        say(f"    (c)  one read at {args.read_gbs:.0f} GB/s (stream_pattern)      {floor:10.1f} us   b' / c = {t['bdev'] / floor:.2f}")
    say(json.dumps({"shape": name, "items": items, "bands": nb, "scalars": N, "us": {k: round(v, 1) for k, v in t.items()}, "floor_us": round(floor, 1)}))


def noisy(shape, rdt):
    grids = torch.meshgrid(*[torch.linspace(0, 1, n, device="cuda", dtype=rdt) for n in shape], indexing="ij")
    return sum(torch.sin(6.283 * (a + 1) * g) for a, g in enumerate(grids)) + 0.3 * torch.randn(shape, device="cuda", dtype=rdt)


for shape in args.shapes.split(","):
    what, kind, dims = shape.split(":")
    rdt = torch.float32 if kind == "f32" else torch.float64
    if what == "vol":
        n = int(dims)
        plan = ndwt.Plan([n, n, n], ["db4"] * 3, rdt, False, True, "reference", max_level=1)
        level, nb, N, K = 1, 8, n ** 3, 0
        pitch = plan.band_pitch()
        x = noisy((n, n, n), rdt).reshape(-1)
    else:
        K, n = (int(v) for v in dims.split("x"))
        plan = ndwt.Plan([n], ["db4"], rdt, False, True, "reference", max_level=4, howmany=K)
        level, nb, N, pitch = 4, 5, K * n, K * n
        x = noisy((K, n), rdt).reshape(-1)
    y = torch.zeros(nb * pitch, dtype=rdt, device="cuda")
    plan.dec(x.data_ptr(), y.data_ptr(), level, s, band_pitch=0 if pitch == N else pitch)
    torch.cuda.synchronize()
    del x
    norms_lines(shape, plan, y, pitch, nb, N, level, 0)
    if K:
        norms_lines(shape, plan, y, pitch, nb, N, level, K)
    del y, plan
    torch.cuda.empty_cache()

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
