#!/usr/bin/env python3
"""The median of |c| over the last band of a coefficient array on the device, hipEvent timing.  Per shape three lines:

  (a) what a user could do before: torch.median(band.abs()) on the same device band (a second copy of the band, and a sort);
  (b) ndwt_band_select (Plan.band_select): the radix select on the bit pattern, 3 (float) / 6 (double) read-only passes, the copy of the
      result and the synchronisation included;
  (c) the byte floor: passes x band bytes / 8 TB/s.

Shapes: the last band of a level-1 dec of a 512^3 volume (smooth signal + noise), and of a 3-level db4 dec of a 4096 x 4096 batch of
signals, float and double.  Median of 20 timed calls in 4 interleaved rounds of 5 (a, b, a, b, ..) after 5 warm-ups of each line, as
tools/bench1d_denoise.py.  Beside (b): the same call with the grid bounded to num_cus x 4 workgroups (set_tuning) and without the
wave-wide combining of equal digits (set_variant(fwd=9)), and the time of one pass.

--contention: 512^3 float bands of chosen contents -- the coefficients above, values within one first-digit bin ([1, 1.05)), one value
-- with and without the combining: what same-bin contention of the LDS atomics costs.

    python tools/bench_select.py [--shapes vol:f32:512,batch:f32:4096x4096,...] [--contention] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="vol:f32:512,batch:f32:4096x4096,vol:f64:512,batch:f64:4096x4096")
ap.add_argument("--contention", action="store_true")
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


def median_ranks(n):
    return [(n - 1) // 2] if n % 2 else [n // 2 - 1, n // 2]


def select_lines(name, rdt, y, band, nb, N, level, make_plan):
    """y: nb bands of N scalars on the device; times torch.median against band_select on band `band`"""
    passes = 3 if rdt == torch.float32 else 6
    view = y[band * N:(band + 1) * N]
    ks = median_ranks(N)
    plans = {"b": make_plan(), "b4": make_plan(), "b0": make_plan()}
    plans["b4"].set_tuning(target_blocks=CUS * 4)
    plans["b0"].set_variant(fwd=9)
    got = {k: p.band_select(y.data_ptr(), level, band, ks, s) for k, p in plans.items()}
    want = float(torch.median(view.abs()))                      # (an even count: torch returns the lower of the two middle values)
    assert got["b"].tobytes() == got["b4"].tobytes() == got["b0"].tobytes() and float(got["b"][0]) == want, (got, want)
    fns = {"a": lambda: torch.median(view.abs())}
    fns.update({k: (lambda p=p: p.band_select(y.data_ptr(), level, band, ks, s)) for k, p in plans.items()})
    t = timed_interleaved(fns)
    mb = N * view.element_size() / 1e6
    floor = passes * mb / 8e6 * 1e6
    say(f"{name}: band {band} of {nb}, {N} elements ({mb:.1f} MB), {passes} passes; median |c| = {want:.9g}")
    say(f"    (a) torch.median(band.abs())                     {t['a']:10.1f} us")
    say(f"    (b) ndwt_band_select                             {t['b']:10.1f} us   {t['b'] / passes:8.1f} us per pass ({mb / 1e3 / (t['b'] / passes) * 1e6:6.0f} GB/s)   a / b = {t['a'] / t['b']:.2f}")
    say(f"        ... on at most {CUS * 4} workgroups              {t['b4']:10.1f} us   {t['b4'] / passes:8.1f} us per pass")
    say(f"        ... without the combining of equal digits    {t['b0']:10.1f} us   {t['b0'] / passes:8.1f} us per pass")
    say(f"    (c) floor: {passes} x {mb:.1f} MB / 8 TB/s                {floor:10.1f} us   b / c = {t['b'] / floor:.2f}")
    say(json.dumps({"shape": name, "elements": N, "passes": passes, "us": {k: round(v, 1) for k, v in t.items()}, "floor_us": round(floor, 1)}))


def noisy(shape, rdt):
    grids = torch.meshgrid(*[torch.linspace(0, 1, n, device="cuda", dtype=rdt) for n in shape], indexing="ij")
    return sum(torch.sin(6.283 * (a + 1) * g) for a, g in enumerate(grids)) + 0.3 * torch.randn(shape, device="cuda", dtype=rdt)


for shape in args.shapes.split(","):
    what, kind, dims = shape.split(":")
    rdt = torch.float32 if kind == "f32" else torch.float64
    if what == "vol":
        n = int(dims)
        mk = lambda: ndwt.Plan([n, n, n], ["db4"] * 3, rdt, False, True, "reference", max_level=1)   # noqa: E731
        level, nb, N = 1, 8, n ** 3
        x = noisy((n, n, n), rdt).reshape(-1)
    else:
        K, n = (int(v) for v in dims.split("x"))
        mk = lambda: ndwt.Plan([n], ["db4"], rdt, False, True, "reference", max_level=3, howmany=K)   # noqa: E731
        level, nb, N = 3, 4, K * n
        x = noisy((K, n), rdt).reshape(-1)
    y = torch.empty(nb * N, dtype=rdt, device="cuda")
    mk().dec(x.data_ptr(), y.data_ptr(), level, s)
    torch.cuda.synchronize()
    del x
    select_lines(shape, rdt, y, nb - 1, nb, N, level, mk)
    if args.contention and shape == "vol:f32:512":
        say("contention, 512^3 float: one band of chosen contents, ndwt_band_select with (AGG 2) and without (AGG 0) the combining of equal digits")
        band = y[(nb - 1) * N:]
        for cname, fill in (("the coefficients above", None), ("uniform in [1, 1.05): one first-digit bin", lambda: band.uniform_(1.0, 1.05)),
                            ("one value", lambda: band.fill_(1.5))):
            if fill:
                fill()
            p2, p0 = mk(), mk()
            p0.set_variant(fwd=9)
            ks = median_ranks(N)
            assert p2.band_select(y.data_ptr(), level, nb - 1, ks, s).tobytes() == p0.band_select(y.data_ptr(), level, nb - 1, ks, s).tobytes()
            t = timed_interleaved({"agg2": lambda: p2.band_select(y.data_ptr(), level, nb - 1, ks, s),
                                   "agg0": lambda: p0.band_select(y.data_ptr(), level, nb - 1, ks, s)})
            say(f"    {cname:44s} AGG 2 {t['agg2']:9.1f} us ({t['agg2'] / 3:7.1f} per pass)   AGG 0 {t['agg0']:9.1f} us ({t['agg0'] / 3:7.1f} per pass)")
            say(json.dumps({"contention": cname, "us": {k: round(v, 1) for k, v in t.items()}}))
    del y
    torch.cuda.empty_cache()

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
