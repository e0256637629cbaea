#!/usr/bin/env python3
"""The SURE statistics of every band of a coefficient array on the device (count, energy and reciprocal sum at nc candidate thresholds)
and the threshold search on top of them, hipEvent timing.  Per array:

  (n)  ndwt_band_norms on the same array in the same process: one read of it by an existing kernel, copy and synchronisation
       included as in (r); (n') ndwt_band_norms_dev: the launches alone
  (r1) ndwt_band_risk(_items) at nc = 1 and (r8) at nc = 8: the upload of the candidates, one launch over all bands (and RiskFinish),
       the copy of the results and the synchronisation
  (t1) / (t8) torch computing the same sums on the same array, band by band and candidate by candidate: (|c| <= t).sum() and
       (c^2 [|c| <= t]).sum(float64) (complex data: also (1 / |c|)[|c| > t].sum(float64)); the results stay on the device
  (s)  ndwt_sure_thresholds(_items), 3 rounds, end to end
  (x)  torch finding the exact minimiser of the same estimate over all data values of every detail band: a sort of |c|, a running sum of
       the squares in float64, the estimate at every order statistic, argmin (real data; complex data: left out, the reciprocal sum
       needs a second running sum and nobody asked)

Arrays: the 8 level-1 bands of a 512^3 volume on the plan's band pitch, float and double (smooth signal + noise); the 4 level-1 bands of
a complex64 stack of 32 images of 512 x 512; the 5 bands of a 4-level db4 dec of 4096 signals of 4096 samples, float, per item.  Median of
20 timed calls in 4 interleaved rounds of 5 after 5 warm-ups of each line, as tools/bench_norms.py.  The library's counts are checked
against torch's before timing.

    python tools/bench_risk.py [--shapes vol:f32:512,vol:f64:512,stack:c64:512x512x32,batch:f32:4096x4096] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="vol:f32:512,vol:f64:512,stack:c64:512x512x32,batch:f32:4096x4096")
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ndwt_amd as ndwt  # noqa: E402

s = torch.cuda.current_stream().cuda_stream
LINES = []
SIGMA = 0.3


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


def magnitudes(band, cplx):
    return torch.view_as_complex(band.view(-1, 2)).abs() if cplx else band.abs()


def torch_risk(bands, cand, items, cplx):
    """[nb, nc, 3] (items = 0) or [items, nb, nc, 3] doubles on the device, band by band and candidate by candidate"""
    rows = []
    for b, band in enumerate(bands):
        a = magnitudes(band, cplx)
        a = a.view(items, -1) if items else a.view(1, -1)
        sq = a.double() ** 2 if cplx else None
        v = band.view(items if items else 1, -1)
        per = []
        for i in range(cand.shape[-1]):
            t = cand[:, b, i:i + 1] if items else cand[b, i].view(1, 1)
            z = ~(a > t)
            en = (sq * z).sum(dim=1) if cplx else (v * v * z).sum(dim=1, dtype=torch.float64)
            inv = ((1.0 / a.double()) * ~z).nan_to_num(0.0, 0.0, 0.0).sum(dim=1) if cplx else torch.zeros_like(en)
            per.append(torch.stack([z.sum(dim=1).double(), en, inv], dim=-1))
        rows.append(torch.stack(per, dim=-2))
    out = torch.stack(rows, dim=1)
    return out if items else out[0]


def torch_exact(bands, svals, items):
    """the exact minimiser of the estimate over the data values of every detail band (real data): thresholds [nb] / [items, nb]"""
    out = []
    for b, band in enumerate(bands):
        if b == 0:
            out.append(torch.zeros(max(items, 1), dtype=torch.float64, device="cuda"))
            continue
        a = band.abs().view(items if items else 1, -1)
        n = a.shape[1]
        e, _ = torch.sort(a, dim=1)
        ed = e.double()
        k = torch.arange(1, n + 1, device="cuda", dtype=torch.float64)
        s2 = (svals[:, b:b + 1] if items else svals[b].view(1, 1)) ** 2
        est = n * s2 + torch.cumsum(ed * ed, dim=1) + ed * ed * (n - k) - 2.0 * s2 * k
        tmax = torch.sqrt(s2) * math.sqrt(2.0 * math.log(n))
        est = torch.where(ed <= tmax, est, torch.full_like(est, float("inf")))
        at = est.argmin(dim=1, keepdim=True)
        best = torch.gather(est, 1, at)
        out.append(torch.where(best < n * s2, torch.gather(ed, 1, at), torch.zeros_like(best)).view(-1))
    r = torch.stack(out, dim=-1)
    return r if items else r[0]


def risk_lines(name, plan, y, pitch_scalars, nb, N, level, items, cplx):
    """y: nb bands of N scalars at `pitch_scalars` scalars on the device"""
    bands = [y[b * pitch_scalars:b * pitch_scalars + N] for b in range(nb)]
    pitch = 0 if pitch_scalars == N else pitch_scalars // (2 if cplx else 1)   # (elements, as the calls take it; 0: packed)
    K = max(items, 1)
    rng = np.random.default_rng(1)
    thr, _ = plan.sure_thresholds_items(y.data_ptr(), level, [SIGMA] * K, 1, s, band_pitch=pitch) if items else plan.sure_thresholds(y.data_ptr(), level, SIGMA, 1, s, band_pitch=pitch)
    base = np.where(thr > 0, thr, SIGMA)                          # candidates of the size the search uses
    cands = {nc: np.ascontiguousarray(base[..., None] * rng.uniform(0.3, 1.2, base.shape + (nc,))) for nc in (1, 8)}
    rdt = np.float32 if y.dtype == torch.float32 else np.float64
    for nc in (1, 8):
        cands[nc] = cands[nc].astype(rdt).astype(np.float64)      # (exact in the scalar type: both sides compare the same numbers)
    dev_c = {nc: torch.from_numpy(cands[nc].astype(rdt)).cuda() for nc in (1, 8)}
    risk = (lambda nc: plan.band_risk_items(y.data_ptr(), level, cands[nc], s, band_pitch=pitch)) if items else (lambda nc: plan.band_risk(y.data_ptr(), level, cands[nc], s, band_pitch=pitch))
    for nc in (1, 8):
        got, want = risk(nc), torch_risk(bands, dev_c[nc], items, cplx).cpu().numpy()
        if not cplx:                                              # (complex: torch's |c| is hypot, a few magnitudes fall on the other side)
            assert np.array_equal(got[..., 0], want[..., 0]), name
        assert np.allclose(got[..., 1], want[..., 1], rtol=1e-5), name
    out = torch.empty(K * nb * 4, dtype=torch.float64, device="cuda")
    fns = {
        "n": (lambda: plan.band_norms_items(y.data_ptr(), level, s, band_pitch=pitch)) if items else (lambda: plan.band_norms(y.data_ptr(), level, s, band_pitch=pitch)),
        "ndev": lambda: plan.band_norms_dev(y.data_ptr(), level, out.data_ptr(), bool(items), s, band_pitch=pitch),
        "r1": lambda: risk(1), "r8": lambda: risk(8),
        "t1": lambda: torch_risk(bands, dev_c[1], items, cplx), "t8": lambda: torch_risk(bands, dev_c[8], items, cplx),
        "s": (lambda: plan.sure_thresholds_items(y.data_ptr(), level, [SIGMA] * K, 3, s, band_pitch=pitch)) if items else (lambda: plan.sure_thresholds(y.data_ptr(), level, SIGMA, 3, s, band_pitch=pitch)),
    }
    if not cplx:
        g = ndwt.band_gains(plan.dims[:1] if items or len(plan.dims) == 1 else plan.dims, "db4", level, 1)
        sv = torch.from_numpy(SIGMA * np.broadcast_to(g, (K, nb)).copy() if items else SIGMA * g).cuda()
        fns["x"] = lambda: torch_exact(bands, sv, items)
    with ndwt.kernel_trace() as recs:
        risk(8)
    t = timed_interleaved(fns)
    gb = nb * N * y.element_size() / 1e9
    what = f"{items} items per band" if items else "band-wide"
    say(f"{name} ({what}): {nb} bands of {N} scalars, {gb * 1e3:.1f} MB in all; launches: " + ", ".join(f"{r.family} x {r.grid[0]}" for r in recs))
    say(f"    (n)  ndwt_band_norms (copy + sync)              {t['n']:10.1f} us   {gb / t['n'] * 1e6:7.0f} GB/s of one read")
    say(f"    (n') ndwt_band_norms_dev (enqueue only)         {t['ndev']:10.1f} us   {gb / t['ndev'] * 1e6:7.0f} GB/s")
    for nc in (1, 8):
        r, tt = t[f"r{nc}"], t[f"t{nc}"]
        say(f"    (r{nc}) ndwt_band_risk, nc = {nc} (upload, copy + sync)  {r:10.1f} us   {gb / r * 1e6:7.0f} GB/s   r / n = {r / t['n']:.2f}   torch (t{nc}) {tt:10.1f} us   t / r = {tt / r:.1f}")
    line = f"    (s)  ndwt_sure_thresholds, 3 rounds             {t['s']:10.1f} us"
    if "x" in t:
        line += f"   torch sort-based exact minimiser (x) {t['x']:10.1f} us   x / s = {t['x'] / t['s']:.1f}"
    say(line)
    say(json.dumps({"shape": name, "items": items, "bands": nb, "scalars": N, "us": {k: round(v, 1) for k, v in t.items()}}))


def noisy(shape, rdt):
    grids = torch.meshgrid(*[torch.linspace(0, 1, n, device="cuda", dtype=rdt) for n in shape], indexing="ij")
    return sum(torch.sin(6.283 * (a + 1) * g) for a, g in enumerate(grids)) + SIGMA * torch.randn(shape, device="cuda", dtype=rdt)


for shape in args.shapes.split(","):
    what, kind, dims = shape.split(":")
    rdt = torch.float64 if kind == "f64" else torch.float32
    cplx = kind.startswith("c")
    comp = 2 if cplx else 1
    if what == "vol":
        n = int(dims)
        plan = ndwt.Plan([n, n, n], ["db4"] * 3, rdt, cplx, True, "reference", max_level=1)
        level, nb, N, K = 1, 8, n ** 3 * comp, 0
        pitch = plan.band_pitch() * comp
        x = noisy((n, n, n), rdt).reshape(-1)
    elif what == "stack":
        n1, n2, K = (int(v) for v in dims.split("x"))
        plan = ndwt.Plan([n1, n2, K], ["db4", "db4", None], rdt, cplx, True, "reference", max_level=1, axes=(0, 1))
        level, nb, N = 1, 4, n1 * n2 * K * comp
        pitch = N
        x = noisy((K, n2, n1, comp), rdt).reshape(-1)
        K = 0                                                     # (timed band-wide)
    else:
        K, n = (int(v) for v in dims.split("x"))
        plan = ndwt.Plan([n], ["db4"], rdt, cplx, True, "reference", max_level=4, howmany=K)
        level, nb, N, pitch = 4, 5, K * n * comp, K * n * comp
        x = noisy((K, n), rdt).reshape(-1)
    y = torch.zeros(nb * pitch, dtype=rdt, device="cuda")
    plan.dec(x.data_ptr(), y.data_ptr(), level, s, band_pitch=0 if pitch == N else pitch // comp)
    torch.cuda.synchronize()
    del x
    risk_lines(shape, plan, y, pitch, nb, N, level, K, cplx)
    del y, plan
    torch.cuda.empty_cache()

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
